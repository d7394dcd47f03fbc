// Connected-component labelling of class maps (unetseg_hip/ccl.py, the cleanup stage of predict.py; no
// reference counterpart): label, per-component area and box, and the relabelling passes of `clean`.
//
// Semantics.  cls int32 [N][H][W]; values are compared for equality only; class 0 is background.
// Two pixels of one image are joined iff they have equal class and are edge neighbours, or diagonal
// neighbours where that class is 8-connected: the non-zero classes have `connectivity` (4 or 8), class 0
// the dual (12 - connectivity).  root[i] is the smallest in-image raster index y * W + x of pixel i's
// component: a canonical name, whatever the launch order, the tile size or the winner of a race.
//
// Label is three launches over one int32 array `parent` (the output itself) that holds a forest with
// parent[j] <= j everywhere and always, all links inside one component:
//   1. tile: one 256-thread block per 64 x 64 tile, classes and parents in LDS.  A wave takes a 64-pixel
//      row segment: the ballot of "differs from my left neighbour" gives every lane its run start by
//      bit arithmetic, so horizontal joins cost no atomic.  Joins with the row above go through a
//      union-find in LDS; every pixel then stores the global index of its tile-local root (the map
//      from tile-local to global raster order is monotone, so that root is the tile-local minimum).
//   2. seam: one thread per pixel on the low side of a tile edge joins it across the edge with a
//      lock-free union in global memory: find both roots, atomicMin the larger root's parent towards
//      the smaller, go on from the returned value when that root had been linked meanwhile.
//   3. flatten: every pixel chases to its root and stores it.
// A link only ever moves to a smaller index of the same component and a component's minimum can be
// linked nowhere, so once every join is made each tree's root is the component's minimum: the result
// does not depend on the order of the unions.  A union that finds parent[a] already lowered to `old`
// lowers it to min(old, b) and then joins old with b itself, so no join is lost.
//
// No block waits on another: kernel boundaries are the only synchronisation between blocks, and every
// loop of find / union ends because an index strictly decreases (see each loop).  All atomics are
// integer, relaxed, agent scope (workgroup scope in LDS); results are bitwise reproducible.
//
// Stats: int32 [4][N][H][W], planes area, ymax, xmin, xmax, meaningful at root positions (area 0
// elsewhere); ymin is the root's own row.  A wave takes a 64-pixel row segment of `root`; one lane per
// run of equal roots adds the run length and the run's extent, not one atomic per pixel.
#include <climits>

#include "elem_util.h"

namespace {

constexpr int kTW = 64;  // tile width: one wave64 per row segment
constexpr int kTH = 64;  // tile height: 16 rows per wave; classes + parents are 32 KB of LDS

#define CCL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define CCL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
// a relaxed access no other wave needs to see at once: an ordinary load / store, named so that a
// concurrent atomic on the same word is no data race
#define CCL_RLX_WAVE __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT

// diagonal neighbours join for this class
__device__ __forceinline__ bool diag8(int v, int conn) { return (v != 0 ? conn : 12 - conn) == 8; }

// ---- union-find in LDS ---------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int i) {
  // ends: par[j] <= j for every j, so i strictly decreases until par[i] == i (index 0 is its own parent)
  for (int p; (p = __hip_atomic_load(par + i, CCL_RLX_WG)) != i;) i = p;
  return i;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b) {
  // ends: every turn returns, or replaces the larger of the two indices by a strictly smaller one
  // (old < a), while find never raises either; indices are bounded below by 0
  for (;;) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, CCL_RLX_WG);
    if (old == a) return;  // a was a root and now hangs below b
    a = old;               // a had been linked to old < a meanwhile: old still has to meet b
  }
}

// ---- the same in global memory, inside one image -------------------------------------------------
__device__ __forceinline__ int glb_find(int* par, int i) {
  // ends: par[j] <= j for every j, so i strictly decreases until par[i] == i
  for (int p; (p = __hip_atomic_load(par + i, CCL_RLX_AGENT)) != i;) i = p;
  return i;
}

__device__ __forceinline__ void glb_union(int* par, int a, int b) {
  // ends: every turn returns, or replaces the larger of the two indices by a strictly smaller one
  // (old < a), while find never raises either; indices are bounded below by 0
  for (;;) {
    a = glb_find(par, a);
    b = glb_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, CCL_RLX_AGENT);
    if (old == a) return;
    a = old;
  }
}

// block = one tile of one image; wave w holds rows w, w + 4, ... of the tile, lane = column
__global__ __launch_bounds__(256) void ccl_tile_kernel(const int* cls, int H, int W, int conn, int tiles_x,
                                                       int tiles_y, int* parent) {
  __shared__ int c[kTH][kTW];
  __shared__ int par[kTH * kTW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long tile = blockIdx.x;
  const long per_image = (long)tiles_x * tiles_y;
  const long img = tile / per_image;
  const int t = (int)(tile - img * per_image);
  const int y0 = (t / tiles_x) * kTH, x0 = (t % tiles_x) * kTW;
  const long base = img * ((long)H * W);
  const int rows = H - y0 < kTH ? H - y0 : kTH;  // rows of the tile inside the image (>= 1)
  const int x = x0 + lane;
  const bool in = x < W;  // lane 0 always is
  for (int r = wave; r < rows; r += 4) {
    const int v = in ? cls[base + (long)(y0 + r) * W + x] : 0;
    c[r][lane] = v;
    const int left = __shfl_up(v, 1, 64);
    const unsigned long long starts = __ballot(in && (lane == 0 || left != v));
    if (in)  // the run start: the highest start bit at or below this lane (bit 0 is set)
      par[r * kTW + lane] = r * kTW + 63 - __clzll(starts & (~0ull >> (63 - lane)));
  }
  __syncthreads();
  for (int r = wave; r < rows; r += 4) {
    if (r == 0 || !in) continue;
    const int v = c[r][lane], up = c[r - 1][lane], me = r * kTW + lane;
    const bool has_l = lane > 0, has_r = lane < kTW - 1 && x + 1 < W;
    if (up == v) {
      // where the pair to the left is of this class too, it makes (or inherits) the same join
      if (!(has_l && c[r][lane - 1] == v && c[r - 1][lane - 1] == v)) lds_union(par, me, me - kTW);
    } else if (diag8(v, conn)) {
      // a diagonal join is needed only where no edge path of the class closes the 2 x 2 square
      if (has_l && c[r - 1][lane - 1] == v && c[r][lane - 1] != v) lds_union(par, me, me - kTW - 1);
      if (has_r && c[r - 1][lane + 1] == v && c[r][lane + 1] != v) lds_union(par, me, me - kTW + 1);
    }
  }
  __syncthreads();
  for (int r = wave; r < rows; r += 4) {
    if (!in) continue;
    const int l = lds_find(par, r * kTW + lane);
    parent[base + (long)(y0 + r) * W + x] = (y0 + l / kTW) * W + x0 + l % kTW;
  }
}

// thread = one pixel of the first column of a tile (x = k * kTW, k >= 1: joins to the left) or of the
// first row of a tile (y = k * kTH, k >= 1: joins upwards); V / S = such pixels per image of the first
// kind / of both
__global__ __launch_bounds__(256) void ccl_seam_kernel(const int* cls, int H, int W, int conn, long V, long S,
                                                       long total, int* parent) {
  const long HW = (long)H * W;
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const long img = it / S, k = it - img * S;
    const int* c = cls + img * HW;
    int* p = parent + img * HW;
    if (k < V) {
      const int x = (int)(k / H + 1) * kTW, y = (int)(k % H);
      const int i = y * W + x, v = c[i], l = c[i - 1];
      const bool above = y > 0, below = y + 1 < H;
      if (l == v) {
        // inside a tile row the pair above, when of this class, makes (or inherits) the same join; on
        // a tile's first row that pair hangs on this one through the other seam, so the join is made
        if (!(y % kTH != 0 && c[i - W] == v && c[i - W - 1] == v)) glb_union(p, i, i - 1);
      } else if (diag8(v, conn)) {
        if (above && c[i - W - 1] == v && c[i - W] != v) glb_union(p, i, i - W - 1);
        if (below && c[i + W - 1] == v && c[i + W] != v) glb_union(p, i, i + W - 1);
      }
    } else {
      const long k2 = k - V;
      const int y = (int)(k2 / W + 1) * kTH, x = (int)(k2 % W);
      const int i = y * W + x, v = c[i], u = c[i - W];
      const bool has_l = x > 0, has_r = x + 1 < W;
      if (u == v) {
        if (!(x % kTW != 0 && c[i - 1] == v && c[i - W - 1] == v)) glb_union(p, i, i - W);
      } else if (diag8(v, conn)) {
        if (has_l && c[i - W - 1] == v && c[i - 1] != v) glb_union(p, i, i - W - 1);
        if (has_r && c[i - W + 1] == v && c[i + 1] != v) glb_union(p, i, i - W + 1);
      }
    }
  }
}

// thread = one pixel: parent[i] = its root.  In place: a pixel another thread has flattened already is
// a shorter way to the same root.
__global__ __launch_bounds__(256) void ccl_flatten_kernel(int H, int W, long total, int* parent) {
  const long HW = (long)H * W;
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const long img = it / HW;
    int* p = parent + img * HW;
    const int i = (int)(it - img * HW);
    int r = i;
    // ends: p[j] <= j for every j, so r strictly decreases until p[r] == r
    for (int q; (q = __hip_atomic_load(p + r, CCL_RLX_WAVE)) != r;) r = q;
    __hip_atomic_store(p + i, r, CCL_RLX_WAVE);
  }
}

__global__ __launch_bounds__(256) void ccl_stats_init_kernel(long planes, int* stats) {
  for (long it = blockIdx.x * 256L + threadIdx.x; it < planes; it += gridDim.x * 256L) {
    stats[it] = 0;                     // area
    stats[planes + it] = 0;            // ymax
    stats[2 * planes + it] = INT_MAX;  // xmin
    stats[3 * planes + it] = 0;        // xmax
  }
}

// wave = one 64-pixel segment of one row; the first lane of each run of equal roots adds the run
__global__ __launch_bounds__(256) void ccl_stats_kernel(const int* root, int H, int W, int segs, long total,
                                                        long planes, int* stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long HW = (long)H * W;
  for (long s = blockIdx.x * 4L + wave; s < total; s += gridDim.x * 4L) {
    const long row = s / segs;
    const int x0 = (int)(s - row * segs) * 64, x = x0 + lane;
    const long img = row / H;
    const int y = (int)(row - img * H);
    const bool in = x < W;
    const int r = in ? root[img * HW + (long)y * W + x] : -1;
    const int left = __shfl_up(r, 1, 64);
    const bool start = in && (lane == 0 || left != r);
    const unsigned long long starts = __ballot(start), valid = __ballot(in);
    if (start) {
      const unsigned long long later = lane == 63 ? 0ull : starts & (~0ull << (lane + 1));
      const int end = (later ? __ffsll((long long)later) - 1 : __popcll(valid)) - 1;  // last lane of the run
      int* at = stats + img * HW + r;
      __hip_atomic_fetch_add(at, end - lane + 1, CCL_RLX_AGENT);
      // the box only ever widens: a value already reached needs no atomic (a stale read costs one)
      if (__hip_atomic_load(at + planes, CCL_RLX_AGENT) < y) __hip_atomic_fetch_max(at + planes, y, CCL_RLX_AGENT);
      if (__hip_atomic_load(at + 2 * planes, CCL_RLX_AGENT) > x)
        __hip_atomic_fetch_min(at + 2 * planes, x, CCL_RLX_AGENT);
      if (__hip_atomic_load(at + 3 * planes, CCL_RLX_AGENT) < x0 + end)
        __hip_atomic_fetch_max(at + 3 * planes, x0 + end, CCL_RLX_AGENT);
    }
  }
}

// thread = one pixel, one writer each.  step 1: a component of a non-zero class below the area
// becomes class 0.  step 2: a class-0 component below the area whose box touches no image border takes
// the class of the pixel above its root (it exists: the root's row is the component's first, not row 0).
__global__ __launch_bounds__(256) void ccl_filter_kernel(const int* cls, const int* root, const int* stats, int H,
                                                         int W, long total, int step, int threshold, int* out) {
  const long HW = (long)H * W;
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    int v = cls[it];
    if (step == 1 ? v != 0 : v == 0) {
      const long img = it / HW;
      const int r = root[it];
      const int* at = stats + img * HW + r;
      if (at[0] < threshold) {
        if (step == 1)
          v = 0;
        else if (r >= W && at[total] < H - 1 && at[2 * total] > 0 && at[3 * total] < W - 1)
          v = cls[img * HW + r - W];
      }
    }
    out[it] = v;
  }
}

// the checked shape shared by the entry points; 0, or 1 with the message set
int ccl_geometry(const char* name, int N, int H, int W, long& total) {
  US_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
  US_CHECK_ARG((long)H * W <= INT32_MAX, "%s: H * W = %d * %d exceeds the 2^31 - 1 pixels of one image", name, H, W);
  // the four stats planes, N * H * W * 4 * 4 bytes, within a signed 64-bit offset
  US_CHECK_ARG(N <= INT64_MAX / 16 / ((long)H * W), "%s: N * H * W * 16 = %d * %d * %d * 16 exceeds 64-bit offsets",
               name, N, H, W);
  total = (long)N * H * W;
  return 0;
}

}  // namespace

// the tile of the label pass (host only): seams lie at multiples of tw / th
UNETSEG_API int unetseg_ccl_tile(int* tw, int* th) {
  US_CHECK_ARG(tw && th, "ccl_tile: null pointer");
  *tw = kTW;
  *th = kTH;
  return 0;
}

// root int32 [N][H][W] = the smallest raster index y * W + x of each pixel's component of cls int32 [N][H][W]
UNETSEG_API int unetseg_ccl_label(const int32_t* cls, int N, int H, int W, int connectivity, int32_t* root,
                                  void* stream) {
  US_CHECK_ARG(cls && root, "ccl_label: null pointer");
  US_CHECK_ARG(connectivity == 4 || connectivity == 8, "ccl_label: connectivity %d is neither 4 nor 8", connectivity);
  long total;
  if (ccl_geometry("ccl_label", N, H, W, total)) return 1;
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const long tiles = (long)tiles_x * tiles_y;
  US_CHECK_ARG(tiles <= INT32_MAX / N, "ccl_label: %d images of %ld tiles exceed the launch grid", N, tiles);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)(N * tiles)), dim3(256), 0, st, cls, H, W, connectivity, tiles_x,
                     tiles_y, root);
  const long V = (long)(tiles_x - 1) * H, S = V + (long)(tiles_y - 1) * W;
  if (S > 0) {
    hipLaunchKernelGGL(ccl_seam_kernel, dim3(grid_for(N * S)), dim3(256), 0, st, cls, H, W, connectivity, V, S, N * S,
                       root);
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3(grid_for(total)), dim3(256), 0, st, H, W, total, root);
  }  // a single tile per image leaves the tile pass's roots final
  US_LAUNCH_CHECK("ccl_label");
  return 0;
}

// stats int32 [4][N][H][W] = area, ymax, xmin, xmax of each component at its root position (area 0
// elsewhere) from root int32 [N][H][W] as unetseg_ccl_label writes it
UNETSEG_API int unetseg_ccl_stats(const int32_t* root, int N, int H, int W, int32_t* stats, void* stream) {
  US_CHECK_ARG(root && stats, "ccl_stats: null pointer");
  long total;
  if (ccl_geometry("ccl_stats", N, H, W, total)) return 1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ccl_stats_init_kernel, dim3(grid_for(total)), dim3(256), 0, st, total, stats);
  const int segs = (W + 63) / 64;
  const long waves = (long)N * H * segs;
  hipLaunchKernelGGL(ccl_stats_kernel, dim3(grid_for(waves * 64)), dim3(256), 0, st, root, H, W, segs, waves, total,
                     stats);
  US_LAUNCH_CHECK("ccl_stats");
  return 0;
}

// out int32 [N][H][W] (not cls) = cls with the components whose area is below `threshold` relabelled:
// step 1 the non-zero classes to 0, step 2 the class-0 components off every image border to the class
// of the pixel above their root; root and stats as the two calls above wrote them for cls
UNETSEG_API int unetseg_ccl_filter(const int32_t* cls, const int32_t* root, const int32_t* stats, int N, int H,
                                   int W, int step, int threshold, int32_t* out, void* stream) {
  US_CHECK_ARG(cls && root && stats && out, "ccl_filter: null pointer");
  US_CHECK_ARG(out != cls, "ccl_filter: out must not be cls (step 2 reads cls at other pixels)");
  US_CHECK_ARG(step == 1 || step == 2, "ccl_filter: step %d is neither 1 (small components) nor 2 (holes)", step);
  US_CHECK_ARG(threshold >= 0, "ccl_filter: negative threshold %d", threshold);
  long total;
  if (ccl_geometry("ccl_filter", N, H, W, total)) return 1;
  hipLaunchKernelGGL(ccl_filter_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, cls, root, stats, H,
                     W, total, step, threshold, out);
  US_LAUNCH_CHECK("ccl_filter");
  return 0;
}
