// Vector contours of class maps (unetseg_hip/contours.py, predict.py --polygons; no reference counterpart): the
// crack loops round every connected component, their vertices, signed areas and lengths.
//
// Semantics.  cls int32 [N][H][W]; values are compared for equality only; class 0 is background.  Pixel (y, x)
// covers [x, x+1] x [y, y+1]; a lattice corner is (x, y), 0 <= x <= W, 0 <= y <= H.  A crack is a side of a pixel
// of a non-zero class whose 4-neighbour across that side has another class or lies outside the image.  Side 0 is
// the top (x, y) -> (x+1, y), 1 the right (x+1, y) -> (x+1, y+1), 2 the bottom (x+1, y+1) -> (x, y+1), 3 the left
// (x, y+1) -> (x, y): clockwise on screen, the owner on the right of travel.  Crack id = (y W + x) 4 + side.
// With d(s) the direction of travel of side s, F = owner + d(s) is the pixel ahead on the owner's side and
// D = F + d(s + 3) the pixel ahead on the other side; "in" = inside the image and of the owner's class:
//   connectivity 8: D in -> side s + 3 of D (left turn); else F in -> side s of F (straight on); else side s + 1
//                   of the owner (right turn);
//   connectivity 4: F out -> right turn; else D out -> straight on; else left turn.
// The target is a crack in every case (its far pixel is F, D or the pixel across the crack itself), and the map is
// a bijection, so the cracks fall into closed loops, each inside one component.  A loop's leader is its smallest
// crack id; the loop is its component's outer loop iff leader == 4 root (unetseg_ccl_label's root: the root's top
// side is a crack and the smallest id the component owns).  A vertex is the tail corner of a crack whose side
// differs from its predecessor's.  The shoelace sum over a loop's vertices equals the sum over all its cracks of
// x_tail y_head - x_head y_tail (collinear corners add nothing new), so the doubled area is a plain sum of
// per-crack terms, in 64 bits.
//
// Stages, all on the caller's stream, none waits on another block (kernel boundaries are the only
// synchronisation between blocks; no loop depends on another thread's progress):
//   mask:   one block per kMW x kMH tile, the classes with a one-pixel halo in LDS (0 outside the image: never an
//           owner's class).  Writes the 4-bit crack mask of every pixel and, per 64-pixel row segment (one wave),
//           the number of cracks.  The segments are numbered in raster order, so an exclusive scan of their
//           counts (the caller's, e.g. torch.cumsum) numbers the cracks 0 .. M-1 in crack-id order.
//   link:   number: a wave per segment scans its 64 popcounts and writes off[pixel], the dense index of the
//           pixel's first crack, and gid[d], the crack of the flat batch behind dense index d.  link: a thread
//           per crack evaluates the rule above from cls at F and D and writes succ[d], and flag[succ[d]] = the
//           successor is a vertex.  A target that is no crack or lies outside 0 .. M-1 cannot occur; were the
//           rule wrong it would make the crack its own successor and count in the failure word, so that a bug is
//           a message and never an access out of bounds.
//   rank:   pointer doubling over the dense cracks, R = ceil(log2 M) rounded up to even rounds per phase (a loop
//           has at most M cracks), each round one launch that reads one buffer and writes the other:
//           1. (nxt, mn) <- (nxt[nxt], min(mn, mn[nxt])) from (succ, self): mn becomes the loop's smallest dense
//              index, which is its smallest crack id, at every crack: lead[d];
//           2. the loop is cut before its leader (nxt = -1 where succ == lead) and suffix doubling sums, from each
//              crack to the end of its loop, the cracks, the vertex flags and the shoelace terms.
//   emit:   a thread per loop (the caller's order: leaders sorted by (image, root, leader) and the exclusive scan
//           `first` of their vertex counts) writes its row and leaves `first` at the leader; a thread per crack
//           that is a vertex writes its tail corner to first + (vertices of the loop - vertices from here on).
// Dense order being crack-id order, every value is a function of the input only.  Everything is integer; the one
// atomic is the failure word's.
#include "seg_pixel.h"

namespace {

constexpr int kMW = 64;  // mask tile width: one wave64 per row segment
constexpr int kMH = 32;  // mask tile height: 8 rows per wave; the tile and its halo are 9 KB of LDS
constexpr long kMaxPixels = 1L << 29;  // per image: crack ids stay below 2^31

using MaskTiles = TileGrid<kMW, kMH>;

#define CTR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// direction of travel of a crack of side s
__device__ __forceinline__ int dir_x(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ __forceinline__ int dir_y(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }
// tail corner of side s, from the pixel's (x, y)
__device__ __forceinline__ int tail_x(int s) { return s == 1 || s == 2; }
__device__ __forceinline__ int tail_y(int s) { return s >= 2; }

// the workspace of M cracks, each part rounded up to 256 bytes
struct CtrLayout {
  size_t gid, succ, flag, lead, nxt, a, nv, area, fail, bytes;
  size_t m;
  explicit CtrLayout(long M) : m((size_t)M) {
    gid = 0;                          // int64 [M]: the crack of the flat batch, (n H W + y W + x) 4 + side
    succ = gid + up256(m * 8);        // int32 [M]
    flag = succ + up256(m * 4);       // int32 [M]: 1 = the crack's tail is a vertex
    lead = flag + up256(m * 4);       // int32 [M]: the loop's leader
    nxt = lead + up256(m * 4);        // int32 [2][M]; after rank nxt[1] holds `first` at the leaders (emit)
    a = nxt + 2 * up256(m * 4);       // int32 [2][M]: the running minimum, then the cracks to the loop's end
    nv = a + 2 * up256(m * 4);        // int32 [2][M]: the vertices to the loop's end
    area = nv + 2 * up256(m * 4);     // int64 [2][M]: the shoelace terms to the loop's end
    fail = area + 2 * up256(m * 8);   // uint32
    bytes = fail + 256;
  }
  size_t half4() const { return up256(m * 4); }
  size_t half8() const { return up256(m * 8); }
};

// block = one tile of one image; wave w holds rows w, w + 4, ... of the tile, lane = column
__global__ __launch_bounds__(256) void ctr_mask_kernel(const int* cls, int H, int W, int tiles_x, int tiles_y,
                                                       unsigned char* mask, int* seg) {
  __shared__ int t[kMH + 2][kMW + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const MaskTiles::Pos tp = MaskTiles::pos(tiles_x, tiles_y);
  const long base = tp.img * ((long)H * W);
  for (int i = threadIdx.x; i < (kMH + 2) * (kMW + 2); i += 256) {
    const int r = i / (kMW + 2), c = i - r * (kMW + 2);
    const int y = tp.y0 - 1 + r, x = tp.x0 - 1 + c;
    t[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? cls[base + (long)y * W + x] : 0;
  }
  __syncthreads();
  const int rows = H - tp.y0 < kMH ? H - tp.y0 : kMH;  // rows of the tile inside the image (>= 1)
  const int x = tp.x0 + lane;
  const bool in = x < W;  // lane 0 always is
  for (int r = wave; r < rows; r += 4) {
    const int v = t[r + 1][lane + 1];
    unsigned m = 0;
    if (in && v != 0)
      m = (unsigned)(t[r][lane + 1] != v) | (unsigned)(t[r + 1][lane + 2] != v) << 1 |
          (unsigned)(t[r + 2][lane + 1] != v) << 2 | (unsigned)(t[r + 1][lane] != v) << 3;
    const long row = tp.img * H + tp.y0 + r;
    if (in) mask[row * W + x] = (unsigned char)m;
    int n = __popc(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) seg[row * tiles_x + tp.x0 / kMW] = n;
  }
}

// wave = one 64-pixel segment of one row; base[s] = the cracks of the segments before s
__global__ __launch_bounds__(256) void ctr_number_kernel(const unsigned char* mask, const long* base, int W, int segs_x,
                                                         long segs, long M, int* off, long* gid) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long s = blockIdx.x * 4L + wave; s < segs; s += gridDim.x * 4L) {
    const long row = s / segs_x;
    const int x = (int)(s - row * segs_x) * 64 + lane;
    const bool in = x < W;
    const long pix = row * W + x;
    const unsigned m = in ? mask[pix] : 0u;
    const int n = __popc(m);
    int incl = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    long d = base[s] + (incl - n);
    if (in) {
      off[pix] = (int)d;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((m >> k & 1u) && d < M) gid[d++] = pix * 4 + k;  // d < M holds; the test keeps a wrong base in bounds
    }
  }
}

// thread = one crack
__global__ __launch_bounds__(256) void ctr_link_kernel(const int* cls, const unsigned char* mask, const int* off,
                                                       const long* gid, int H, int W, int conn, long M, int* succ,
                                                       int* flag, unsigned* fail) {
  const long HW = (long)H * W;
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) {
    const long g = gid[d], pix = g >> 2;
    const int s = (int)(g & 3);
    const long img = pix / HW;
    const int p = (int)(pix - img * HW), y = p / W, x = p - y * W;
    const int* c = cls + img * HW;
    const int v = c[p];
    const int fy = y + dir_y(s), fx = x + dir_x(s);
    const int dy = fy + dir_y((s + 3) & 3), dx = fx + dir_x((s + 3) & 3);
    const bool f_in = fy >= 0 && fy < H && fx >= 0 && fx < W && c[fy * W + fx] == v;
    const bool d_in = dy >= 0 && dy < H && dx >= 0 && dx < W && c[dy * W + dx] == v;
    const bool left = conn == 8 ? d_in : f_in && d_in;
    const bool straight = !left && f_in;
    const int ty = left ? dy : straight ? fy : y, tx = left ? dx : straight ? fx : x;
    const int ts = left ? (s + 3) & 3 : straight ? s : (s + 1) & 3;
    const long tpix = img * HW + (long)ty * W + tx;  // inside the image: `in` was tested, or it is the owner
    const unsigned tm = mask[tpix];
    long to = (long)off[tpix] + __popc(tm & ((1u << ts) - 1u));
    int turn = ts != s;
    if (!(tm >> ts & 1u) || to < 0 || to >= M) {
      __hip_atomic_fetch_add(fail, 1u, CTR_RLX_AGENT);
      to = d, turn = 0;
    }
    succ[d] = (int)to;
    flag[to] = turn;  // one writer per crack: the map is a bijection
  }
}

__global__ __launch_bounds__(256) void ctr_rank_init_kernel(const int* succ, long M, int* nxt, int* mn) {
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) nxt[d] = succ[d], mn[d] = (int)d;
}

// one round of the cyclic minimum: every index is a dense index below M
__global__ __launch_bounds__(256) void ctr_min_kernel(const int* nxt_in, const int* mn_in, long M, int* nxt_out,
                                                      int* mn_out) {
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) {
    const int n = nxt_in[d];
    const int a = mn_in[d], b = mn_in[n];
    mn_out[d] = a < b ? a : b;
    nxt_out[d] = nxt_in[n];
  }
}

// mn (the finished minimum, in a[0]) -> lead; the lists of phase 2 in the buffers 0.  a[0] is read and written at
// d only
__global__ __launch_bounds__(256) void ctr_cut_kernel(const int* succ, const int* flag, const long* gid, int H, int W,
                                                      long M, int* lead, int* nxt, int* a, int* nv, long* area) {
  const long HW = (long)H * W;
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) {
    const int l = a[d], n = succ[d];
    lead[d] = l;
    nxt[d] = n == l ? -1 : n;
    a[d] = 1;
    nv[d] = flag[d];
    const long g = gid[d], pix = g >> 2;
    const int s = (int)(g & 3);
    const int p = (int)(pix % HW), y = p / W, x = p - y * W;
    const long x0 = x + tail_x(s), y0 = y + tail_y(s), x1 = x0 + dir_x(s), y1 = y0 + dir_y(s);
    area[d] = x0 * y1 - x1 * y0;
  }
}

// one round of the suffix sums: nxt is -1 at a list's end, else a dense index below M
__global__ __launch_bounds__(256) void ctr_sum_kernel(const int* nxt_in, const int* a_in, const int* nv_in,
                                                      const long* area_in, long M, int* nxt_out, int* a_out,
                                                      int* nv_out, long* area_out) {
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) {
    const int n = nxt_in[d];
    int a = a_in[d], v = nv_in[d], nn = -1;
    long s = area_in[d];
    if (n >= 0) a += a_in[n], v += nv_in[n], s += area_in[n], nn = nxt_in[n];
    nxt_out[d] = nn, a_out[d] = a, nv_out[d] = v, area_out[d] = s;
  }
}

// thread = one loop, in the caller's order
__global__ __launch_bounds__(256) void ctr_loops_kernel(const int* cls, const int* root, const int* leaders,
                                                        const int* first, int L, int H, int W, long M, const long* gid,
                                                        const int* cracks, const int* nv, const long* area, int* at,
                                                        int* loops) {
  const long HW = (long)H * W;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < L; i += gridDim.x * 256) {
    const int d = leaders[i];
    if (d < 0 || d >= M) continue;  // not a dense index: no row rather than a read out of bounds
    const long g = gid[d], pix = g >> 2;
    const long img = pix / HW;
    const long id = g - img * HW * 4;  // the leader's crack id in its image, < 2^31
    const int r = root[pix];
    int* row = loops + (long)i * 8;
    row[0] = (int)img, row[1] = cls[pix], row[2] = r, row[3] = id != 4L * r;
    row[4] = first[i], row[5] = nv[d], row[6] = (int)(area[d] / 2), row[7] = cracks[d];
    at[d] = first[i];
  }
}

// thread = one crack; a vertex writes its tail corner
__global__ __launch_bounds__(256) void ctr_vertices_kernel(const int* flag, const int* lead, const int* nv,
                                                           const int* at, const long* gid, int H, int W, long M, long V,
                                                           int* vertices, unsigned* fail) {
  const long HW = (long)H * W;
  for (long d = blockIdx.x * 256L + threadIdx.x; d < M; d += gridDim.x * 256L) {
    if (!flag[d]) continue;
    const int l = lead[d];
    const long pos = (long)at[l] + (nv[l] - nv[d]);
    if (pos < 0 || pos >= V) {  // cannot occur: first and V are the scan and the sum of the same counts
      __hip_atomic_fetch_add(fail, 1u, CTR_RLX_AGENT);
      continue;
    }
    const long g = gid[d];
    const int s = (int)(g & 3);
    const int p = (int)((g >> 2) % HW), y = p / W, x = p - y * W;
    vertices[2 * pos] = x + tail_x(s);
    vertices[2 * pos + 1] = y + tail_y(s);
  }
}

// the rounds of one phase: the smallest even R with 2^R >= M
inline int ctr_rounds(long M) {
  int r = 0;
  while ((1L << r) < M) ++r;
  return (r + 1) & ~1;
}

// the checks shared by the entry points: 0; 1 with the message set; -1 for an empty batch (nothing to do)
int ctr_geometry(const char* name, int N, int H, int W) {
  US_CHECK_ARG(N >= 0 && H >= 0 && W >= 0, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
  if (N == 0 || H == 0 || W == 0) return -1;
  US_CHECK_ARG((long)H * W <= kMaxPixels, "%s: H * W = %d * %d exceeds the 2^29 pixels of one image", name, H, W);
  US_CHECK_ARG(MaskTiles::shape_ok(N, H, W), "%s: shape N=%d H=%d W=%d is too large", name, N, H, W);
  return 0;
}

int ctr_workspace(const char* name, long M, const void* ws, size_t ws_bytes) {
  US_CHECK_ARG(M >= 1 && M <= INT32_MAX, "%s: %ld cracks outside 1 .. 2^31 - 1", name, M);
  US_CHECK_ARG(ws, "%s: null workspace", name);
  US_CHECK_ARG(ws_bytes >= CtrLayout(M).bytes, "%s: workspace too small", name);
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  return 0;
}

#define CTR_GEOMETRY(name)                          \
  do {                                              \
    const int g_ = ctr_geometry(name, N, H, W);     \
    if (g_ != 0) return g_ < 0 ? 0 : 1;             \
  } while (0)

#define CTR_HIP(name, call)                                                          \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) {                                                          \
      unetseg_set_error("%s: %s failed: %s", name, #call, hipGetErrorString(e_));    \
      return 2;                                                                      \
    }                                                                                \
  } while (0)

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// the tile of the mask kernel (host only)
UNETSEG_API int unetseg_contours_tile(int* tw, int* th) {
  US_CHECK_ARG(tw && th, "contours_tile: null pointer");
  *tw = kMW, *th = kMH;
  return 0;
}

// host only; 0 for a crack count the entry points refuse
UNETSEG_API size_t unetseg_contours_workspace(long M) {
  if (M < 1 || M > INT32_MAX) return 0;
  return CtrLayout(M).bytes;
}

// host only: at[0 .. 8) = the byte offsets in the workspace of gid int64 [M], succ, flag and lead int32 [M], and of
// what unetseg_contours_rank leaves: cracks int32 [M], vertices int32 [M] and doubled areas int64 [M] from each
// crack to the end of its loop (the loop's totals at its leader); at[7] = the failure word (uint32)
UNETSEG_API int unetseg_contours_layout(long M, int64_t* at) {
  US_CHECK_ARG(at, "contours_layout: null pointer");
  US_CHECK_ARG(unetseg_contours_workspace(M) != 0, "contours_layout: %ld cracks outside 1 .. 2^31 - 1", M);
  const CtrLayout lay(M);
  at[0] = (int64_t)lay.gid, at[1] = (int64_t)lay.succ, at[2] = (int64_t)lay.flag, at[3] = (int64_t)lay.lead;
  at[4] = (int64_t)lay.a, at[5] = (int64_t)lay.nv, at[6] = (int64_t)lay.area, at[7] = (int64_t)lay.fail;
  return 0;
}

// mask uint8 [N][H][W] = the crack sides of every pixel (bit s = side s), seg int32 [N][H][ceil(W / 64)] = the
// cracks of every 64-pixel row segment
UNETSEG_API int unetseg_contours_mask(const int32_t* cls, int N, int H, int W, uint8_t* mask, int32_t* seg,
                                      void* stream) {
  US_CHECK_ARG(cls && mask && seg, "contours_mask: null pointer");
  CTR_GEOMETRY("contours_mask");
  const MaskTiles t(N, H, W);
  hipLaunchKernelGGL(ctr_mask_kernel, dim3((unsigned)t.blocks), dim3(256), 0, (hipStream_t)stream, cls, H, W, t.tx,
                     t.ty, mask, seg);
  US_LAUNCH_CHECK("contours_mask");
  return 0;
}

// off int32 [N][H][W] = the dense index of every pixel's first crack, and the workspace's gid, succ and flag, from
// mask (unetseg_contours_mask) and base int64 [N][H][ceil(W / 64)], the exclusive scan of seg, whose total is M
UNETSEG_API int unetseg_contours_link(const int32_t* cls, const uint8_t* mask, const int64_t* base, int N, int H, int W,
                                      int connectivity, long M, int32_t* off, void* ws, size_t ws_bytes,
                                      void* stream) {
  US_CHECK_ARG(cls && mask && base && off, "contours_link: null pointer");
  US_CHECK_ARG(connectivity == 4 || connectivity == 8, "contours_link: connectivity %d is neither 4 nor 8",
               connectivity);
  CTR_GEOMETRY("contours_link");
  if (ctr_workspace("contours_link", M, ws, ws_bytes)) return 1;
  US_CHECK_ARG(M <= 4L * N * H * W, "contours_link: %ld cracks exceed the 4 sides of %d * %d * %d pixels", M, N, H, W);
  const CtrLayout lay(M);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  long* gid = (long*)(w + lay.gid);
  CTR_HIP("contours_link", hipMemsetAsync(w + lay.fail, 0, 4, st));
  // a wrong base could leave cracks unnumbered: a defined gid (crack 0) keeps every later index inside the batch
  CTR_HIP("contours_link", hipMemsetAsync(gid, 0, (size_t)M * 8, st));
  const int segs_x = (W + 63) / 64;
  const long segs = (long)N * H * segs_x;
  hipLaunchKernelGGL(ctr_number_kernel, dim3(grid_for(segs * 64)), dim3(256), 0, st, mask, (const long*)base, W,
                     segs_x, segs, M, off, gid);
  hipLaunchKernelGGL(ctr_link_kernel, dim3(grid_for(M)), dim3(256), 0, st, cls, mask, (const int*)off,
                     (const long*)gid, H, W, connectivity, M, (int*)(w + lay.succ), (int*)(w + lay.flag),
                     (unsigned*)(w + lay.fail));
  US_LAUNCH_CHECK("contours_link");
  return 0;
}

// the workspace's lead, cracks, vertices and doubled areas from its gid, succ and flag (unetseg_contours_link)
UNETSEG_API int unetseg_contours_rank(int N, int H, int W, long M, void* ws, size_t ws_bytes, void* stream) {
  CTR_GEOMETRY("contours_rank");
  if (ctr_workspace("contours_rank", M, ws, ws_bytes)) return 1;
  const CtrLayout lay(M);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  int* nxt[2] = {(int*)(w + lay.nxt), (int*)(w + lay.nxt + lay.half4())};
  int* a[2] = {(int*)(w + lay.a), (int*)(w + lay.a + lay.half4())};
  int* nv[2] = {(int*)(w + lay.nv), (int*)(w + lay.nv + lay.half4())};
  long* area[2] = {(long*)(w + lay.area), (long*)(w + lay.area + lay.half8())};
  const int* succ = (const int*)(w + lay.succ);
  const int rounds = ctr_rounds(M);  // even: both phases end in the buffers 0
  const dim3 grid(grid_for(M)), block(256);
  hipLaunchKernelGGL(ctr_rank_init_kernel, grid, block, 0, st, succ, M, nxt[0], a[0]);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(ctr_min_kernel, grid, block, 0, st, (const int*)nxt[r & 1], (const int*)a[r & 1], M,
                       nxt[~r & 1], a[~r & 1]);
  hipLaunchKernelGGL(ctr_cut_kernel, grid, block, 0, st, succ, (const int*)(w + lay.flag), (const long*)(w + lay.gid),
                     H, W, M, (int*)(w + lay.lead), nxt[0], a[0], nv[0], area[0]);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(ctr_sum_kernel, grid, block, 0, st, (const int*)nxt[r & 1], (const int*)a[r & 1],
                       (const int*)nv[r & 1], (const long*)area[r & 1], M, nxt[~r & 1], a[~r & 1], nv[~r & 1],
                       area[~r & 1]);
  US_LAUNCH_CHECK("contours_rank");
  return 0;
}

// loops int32 [L][8] = (image, class, root, hole, first, count, area, cracks) of the loops led by leaders int32 [L]
// (dense indices, in the order of the rows) and vertices int32 [V][2] = their corners (x, y), loop i's at first[i]
// onward; root = unetseg_ccl_label of cls; the workspace as unetseg_contours_rank left it
UNETSEG_API int unetseg_contours_emit(const int32_t* cls, const int32_t* root, int N, int H, int W, long M,
                                      const int32_t* leaders, const int32_t* first, int L, int32_t* loops,
                                      int32_t* vertices, long V, void* ws, size_t ws_bytes, void* stream) {
  US_CHECK_ARG(cls && root, "contours_emit: null pointer");
  US_CHECK_ARG(L >= 0 && V >= 0, "contours_emit: negative L=%d or V=%ld", L, V);
  CTR_GEOMETRY("contours_emit");
  if (ctr_workspace("contours_emit", M, ws, ws_bytes)) return 1;
  if (L == 0) return 0;
  US_CHECK_ARG(leaders && first && loops && (vertices || V == 0), "contours_emit: null pointer");
  const CtrLayout lay(M);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  const long* gid = (const long*)(w + lay.gid);
  const int* nv = (const int*)(w + lay.nv);
  int* at = (int*)(w + lay.nxt + lay.half4());
  hipLaunchKernelGGL(ctr_loops_kernel, dim3(grid_for(L)), dim3(256), 0, st, cls, root, leaders, first, L, H, W, M, gid,
                     (const int*)(w + lay.a), nv, (const long*)(w + lay.area), at, loops);
  if (V > 0)
    hipLaunchKernelGGL(ctr_vertices_kernel, dim3(grid_for(M)), dim3(256), 0, st, (const int*)(w + lay.flag),
                       (const int*)(w + lay.lead), nv, (const int*)at, gid, H, W, M, V, vertices,
                       (unsigned*)(w + lay.fail));
  US_LAUNCH_CHECK("contours_emit");
  return 0;
}
