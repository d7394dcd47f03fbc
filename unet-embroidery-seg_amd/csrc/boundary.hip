// Boundary quality of class maps (unetseg_hip/boundary.py, the boundary metrics of val.py and of the
// evaluate loops; no reference counterpart): edge map, exact squared Euclidean distance transform, and
// the pair counts that boundary F-score, Boundary IoU and HD95 are read from.
//
// Everything is integer, so every result is bitwise reproducible.  No block waits on another: kernel
// boundaries are the only synchronisation between blocks, and every loop is bounded (see each loop).
//
// Edge map.  cls int32 [N][H][W], class c, `ignore` (-1: none).  Pixel p is an edge pixel of c iff
// cls[p] == c, cls[p] is not `ignore`, and one of its four edge neighbours lies inside the image, is not
// `ignore` and has a class != c.  The image frame is no boundary.  One thread per pixel, one launch.
//
// Distance transform.  sites uint8 [N][H][W] (non-zero = site) -> d2 int32 [N][H][W], the minimum over
// the sites (y', x') of the same image of (y - y')^2 + (x - x')^2; kEdtInf = 2^30 where the image has no
// site.  H, W <= 16384, so a real distance is at most 2 * 16383^2 < 2^30.  Separable, three launches over
// the output itself (no scratch); a column distance is kept unsquared in 16 bits, at most 16383, with
// kNone = 32768 for "no site", whose square is kEdtInf exactly: no sum with an infinite term is formed.
//   1. column, local: one thread per column and segment of kSeg rows scans its rows down and up in
//      registers and stores the distance to the nearest site of its own segment in the low half-word.
//   2. column, merge: the same thread finds the nearest site above and below its segment from the low
//      half-words of the last row of the segments above and of the first row of those below (the first
//      that is not kNone), and stores min(local, above, below) in the high half-word.  Low half-words
//      never change in this launch, so what one thread reads there does not depend on what another has
//      stored already.  A single segment per column (H <= kSeg) needs no merge: launch 1 fills both halves.
//   3. row: one block per row stages the row's column distances in LDS as 16-bit values with the minimum
//      of every kSeg-wide chunk beside them.  A thread per pixel then scans outwards, left and right,
//      over x' with (x - x')^2 < best so far, and on entering a chunk skips it whole when
//      min(chunk)^2 + (x - x')^2 >= best: every x' of the chunk is at least as far and has at least
//      that column distance, and best only falls, so no skipped x' can win.  The result is the exact
//      lower envelope min over x' of g[x'] + (x - x')^2.  In place: a block reads its row before it
//      writes it and touches no other row.
// Cost of the row pass per pixel: the window, at most sqrt(d2) reads each way, plus one read per chunk
// skipped.  A single site (or none) in the image lets every chunk but one be skipped: at most
// kSeg + W / kSeg LDS reads per pixel, 160 at W = 6144.  The worst case is the inside of a large region:
// along a chord of a disc of radius R every g[x'] + (x - x')^2 equals R^2, so no chunk is skipped and a
// pixel reads about as many words as it is pixels from the edge, which is what a windowed scan costs by
// nature (tools/boundary_timing.py measures both; DESIGN.md has the figures).
//
// Pair counts.  counts int64 [2 (K + 2) + 2] += over all pixels: the histogram of min(dG, K + 1) over the
// edge pixels of the prediction, the same of dP over the edge pixels of the target, and the Boundary-IoU
// intersection and union of P_d = {pred == c, dP <= biou_d2} and G_d = {target == c, dG <= biou_d2},
// without the pixels whose target is `ignore`.  A block counts in LDS: a wave adds each distinct bin
// once with the number of its lanes that hit it, and the block adds its non-zero bins to `counts` when it
// is done.  LDS holds kBins bins (both histograms at K = 4096); a larger K runs one grid row per window of
// kBins bins, each over all pixels, counting the bins of its window only.
#include "boundary_edt.h"
#include "elem_util.h"

namespace {

constexpr int kSeg = 64;            // rows per column segment = width of a row chunk
constexpr unsigned kNone = 32768u;  // "no site" as a 16-bit column distance; kNone^2 == kEdtInf
constexpr int kBins = 2 * (4096 + 2);  // histogram bins a block holds in LDS (32.8 KB)
constexpr int kMaxK = 65536;

#define BND_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- edge map ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void boundary_edges_kernel(const int* cls, int H, int W, long total, int c,
                                                             int ignore, uint8_t* out) {
  const bool has_ign = ignore != -1;
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const int v = cls[it];
    bool e = false;
    if (v == c && !(has_ign && v == ignore)) {
      const long row = it / W;
      const int x = (int)(it - row * W), y = (int)(row % H);
      // a neighbour of another class that is not `ignore`
      auto other = [&](int u) { return u != c && !(has_ign && u == ignore); };
      e = (x > 0 && other(cls[it - 1])) || (x + 1 < W && other(cls[it + 1])) || (y > 0 && other(cls[it - W])) ||
          (y + 1 < H && other(cls[it + W]));
    }
    out[it] = e ? 1 : 0;
  }
}

// ---- distance transform: columns -------------------------------------------------------------------
// thread = one column x of one segment s of one image; d2[..] = local (| local << 16 when `single`)
__global__ __launch_bounds__(256) void edt_col_local_kernel(const uint8_t* sites, int H, int W, int nseg,
                                                            long total, int single, unsigned* d2) {
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const long q = it / W;
    const int x = (int)(it - q * W), s = (int)(q % nseg);
    const long base = (q / nseg) * ((long)H * W) + x;
    const int y0 = s * kSeg, rows = H - y0 < kSeg ? H - y0 : kSeg;  // rows of the segment inside the image (>= 1)
    unsigned d[kSeg];
    unsigned run = kNone;  // rows since the last site of the segment, going down
#pragma unroll
    for (int r = 0; r < kSeg; ++r) {
      const bool site = r < rows && sites[base + (long)(y0 + r) * W] != 0;
      run = site ? 0u : (run == kNone ? kNone : run + 1);
      d[r] = run;
    }
    run = kNone;  // the same going up; a site is where the down scan left 0
#pragma unroll
    for (int r = kSeg - 1; r >= 0; --r) {
      run = d[r] == 0 ? 0u : (run == kNone ? kNone : run + 1);
      const unsigned m = d[r] < run ? d[r] : run;
      if (r < rows) d2[base + (long)(y0 + r) * W] = single ? (m << 16 | m) : m;
    }
  }
}

// the same thread: high half-word = min(local, nearest site above the segment, nearest below it)
__global__ __launch_bounds__(256) void edt_col_merge_kernel(int H, int W, int nseg, long total, unsigned* d2) {
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const long q = it / W;
    const int x = (int)(it - q * W), s = (int)(q % nseg);
    unsigned* col = d2 + (q / nseg) * ((long)H * W) + x;
    const int y0 = s * kSeg, rows = H - y0 < kSeg ? H - y0 : kSeg;
    int ya = -1, yb = -1;  // row of the nearest site above / below the segment, -1: none
    // ends: k falls to 0.  The last row of a segment above is at or below all of that segment's sites, so
    // its local distance names the segment's last site
    for (int k = s - 1; k >= 0; --k) {
      const int b = k * kSeg + kSeg - 1;
      const unsigned v = __hip_atomic_load(col + (long)b * W, BND_RLX_AGENT) & 0xFFFFu;
      if (v != kNone) {
        ya = b - (int)v;
        break;
      }
    }
    // ends: k rises to nseg - 1.  The first row of a segment below names that segment's first site
    for (int k = s + 1; k < nseg; ++k) {
      const int t = k * kSeg;
      const unsigned v = __hip_atomic_load(col + (long)t * W, BND_RLX_AGENT) & 0xFFFFu;
      if (v != kNone) {
        yb = t + (int)v;
        break;
      }
    }
    for (int r = 0; r < rows; ++r) {
      const int y = y0 + r;
      unsigned* at = col + (long)y * W;
      const unsigned loc = __hip_atomic_load(at, BND_RLX_AGENT) & 0xFFFFu;
      unsigned fin = loc;
      if (ya >= 0 && (unsigned)(y - ya) < fin) fin = (unsigned)(y - ya);
      if (yb >= 0 && (unsigned)(yb - y) < fin) fin = (unsigned)(yb - y);
      // another thread may be reading this word's low half, which keeps its value
      __hip_atomic_store(at, fin << 16 | loc, BND_RLX_AGENT);
    }
  }
}

// ---- distance transform: rows ----------------------------------------------------------------------
// block = one row at a time; LDS: sd[chunks * kSeg] column distances, smin[chunks] their chunk minima
__global__ __launch_bounds__(256) void edt_row_kernel(int W, int chunks, long rows, unsigned* d2) {
  extern __shared__ unsigned short edt_lds[];
  unsigned short* sd = edt_lds;
  unsigned short* smin = edt_lds + chunks * kSeg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    unsigned* line = d2 + row * W;
    for (int ch = wave; ch < chunks; ch += 4) {
      const int x = ch * kSeg + lane;
      const unsigned v = x < W ? line[x] >> 16 : kNone;
      sd[x] = (unsigned short)v;
      unsigned m = v;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(m, o, 64);
        m = t < m ? t : m;
      }
      if (lane == 0) smin[ch] = (unsigned short)m;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 256) {
      const int d0 = sd[x];
      int best = d0 * d0;  // kEdtInf where the column has no site
      int xl = x - 1, xr = x + 1;
      {
        // the pixel's own chunk holds nothing nearer when its minimum is the pixel's own distance
        const int m = smin[x / kSeg];
        if (m * m >= best) {
          xl = x / kSeg * kSeg - 1;
          xr = xl + kSeg + 1;
        }
      }
      // ends: xl falls by at least 1 every turn.  dx2 < best <= 2^30 below, so best - dx2 > 0, and a
      // square of a 16-bit distance is at most 2^30: nothing overflows
      while (xl >= 0) {
        const int dx = x - xl, dx2 = dx * dx;
        if (dx2 >= best) break;
        if (xl % kSeg == kSeg - 1) {  // entering a chunk at its near end
          const int m = smin[xl / kSeg];
          if (m * m >= best - dx2) {
            xl -= kSeg;
            continue;
          }
        }
        const int v = sd[xl], g = v * v;
        if (g < best - dx2) best = g + dx2;
        --xl;
      }
      // ends: xr rises by at least 1 every turn
      while (xr < W) {
        const int dx = xr - x, dx2 = dx * dx;
        if (dx2 >= best) break;
        if (xr % kSeg == 0) {
          const int m = smin[xr / kSeg];
          if (m * m >= best - dx2) {
            xr += kSeg;
            continue;
          }
        }
        const int v = sd[xr], g = v * v;
        if (g < best - dx2) best = g + dx2;
        ++xr;
      }
      line[x] = (unsigned)best;
    }
    __syncthreads();  // the next row overwrites the LDS
  }
}

// ---- pair counts -----------------------------------------------------------------------------------
// every lane of the wave calls this; bins[bin] += 1 for the lanes with `on`, one LDS atomic per distinct bin
__device__ __forceinline__ void wave_count(unsigned* bins, bool on, int bin, int lane) {
  unsigned long long todo = __ballot(on);
  // ends: every turn clears at least the leader's bit of `todo`
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int b = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(on && bin == b);
    if (lane == leader) atomicAdd(bins + b, (unsigned)__popcll(same));
    todo &= ~same;
  }
}

// grid.y = window of kBins histogram bins; grid.x strides over the pixels
__global__ __launch_bounds__(256) void boundary_counts_kernel(const int* pred, const int* target, const uint8_t* eP,
                                                              const uint8_t* eG, const int* dP, const int* dG,
                                                              long total, int c, int ignore, int K, int biou_d2,
                                                              unsigned long long* counts) {
  __shared__ unsigned bins[kBins];
  __shared__ unsigned iou[2];
  const int lane = threadIdx.x & 63;
  const int nb = 2 * (K + 2), w0 = blockIdx.y * kBins;
  const bool has_ign = ignore != -1, first = blockIdx.y == 0;
  for (int i = threadIdx.x; i < kBins; i += 256) bins[i] = 0;
  if (threadIdx.x < 2) iou[threadIdx.x] = 0;
  __syncthreads();
  unsigned inter = 0, uni = 0;
  // the bound is the same for the whole block, so every wave stays whole inside wave_count
  for (long b0 = blockIdx.x * 256L; b0 < total; b0 += gridDim.x * 256L) {
    const long it = b0 + threadIdx.x;
    const bool in = it < total;
    const bool ep = in && eP[it] != 0, eg = in && eG[it] != 0;
    const int dp = in ? dP[it] : 0, dg = in ? dG[it] : 0;
    const int bp = (dg < K + 1 ? dg : K + 1) - w0;            // prediction edge -> target
    const int bg = K + 2 + (dp < K + 1 ? dp : K + 1) - w0;    // target edge -> prediction
    wave_count(bins, ep && bp >= 0 && bp < kBins, bp, lane);
    wave_count(bins, eg && bg >= 0 && bg < kBins, bg, lane);
    if (first && in) {
      const int t = target[it];
      if (!(has_ign && t == ignore)) {
        const bool a = pred[it] == c && dp <= biou_d2, b = t == c && dg <= biou_d2;
        inter += a && b;
        uni += a || b;
      }
    }
  }
  if (first) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      inter += __shfl_xor(inter, o, 64);
      uni += __shfl_xor(uni, o, 64);
    }
    if (lane == 0) {
      atomicAdd(iou, inter);
      atomicAdd(iou + 1, uni);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBins && w0 + i < nb; i += 256)
    if (bins[i]) atomicAdd(counts + w0 + i, (unsigned long long)bins[i]);
  if (first && threadIdx.x < 2 && iou[threadIdx.x])
    atomicAdd(counts + nb + threadIdx.x, (unsigned long long)iou[threadIdx.x]);
}

// the checked shape shared by the entry points; 0, or 1 with the message set
int boundary_geometry(const char* name, int N, int H, int W, long& total) {
  US_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
  US_CHECK_ARG(H <= kEdtMax && W <= kEdtMax, "%s: H=%d W=%d exceed %d (distances must stay below 2^30)", name, H, W,
               kEdtMax);
  total = (long)N * H * W;  // < 2^31 * 2^28
  return 0;
}

}  // namespace

// the launches of the distance transform (boundary_edt.h); arguments checked by the caller
void launch_edt_sqdist(const uint8_t* sites, int N, int H, int W, int32_t* d2, hipStream_t st) {
  unsigned* out = (unsigned*)d2;
  const int nseg = (H + kSeg - 1) / kSeg;
  const long cols = (long)N * nseg * W;
  hipLaunchKernelGGL(edt_col_local_kernel, dim3(grid_for(cols)), dim3(256), 0, st, sites, H, W, nseg, cols,
                     nseg == 1 ? 1 : 0, out);
  if (nseg > 1)
    hipLaunchKernelGGL(edt_col_merge_kernel, dim3(grid_for(cols)), dim3(256), 0, st, H, W, nseg, cols, out);
  const int chunks = (W + kSeg - 1) / kSeg;
  const long rows = (long)N * H;
  const size_t lds = (size_t)(chunks * kSeg + chunks) * sizeof(unsigned short);  // <= 33 KB
  hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)(rows < (1L << 20) ? rows : (1L << 20))), dim3(256), lds, st, W,
                     chunks, rows, out);
}

// the segment of the column pass and the chunk of the row pass (host only): seams lie at its multiples
UNETSEG_API int unetseg_edt_chunk(int* len) {
  US_CHECK_ARG(len, "edt_chunk: null pointer");
  *len = kSeg;
  return 0;
}

// edge uint8 [N][H][W] = 1 at the edge pixels of class c of cls int32 [N][H][W], else 0; ignore -1: none
UNETSEG_API int unetseg_boundary_edges(const int32_t* cls, int N, int H, int W, int c, int ignore, uint8_t* edge,
                                       void* stream) {
  US_CHECK_ARG(cls && edge, "boundary_edges: null pointer");
  long total;
  if (boundary_geometry("boundary_edges", N, H, W, total)) return 1;
  hipLaunchKernelGGL(boundary_edges_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, cls, H, W, total,
                     c, ignore, edge);
  US_LAUNCH_CHECK("boundary_edges");
  return 0;
}

// d2 int32 [N][H][W] = exact squared Euclidean distance to the nearest non-zero pixel of the same image of
// sites uint8 [N][H][W]; UNETSEG_EDT_INF where the image has none.  d2 is the only scratch.
UNETSEG_API int unetseg_edt_sqdist(const uint8_t* sites, int N, int H, int W, int32_t* d2, void* stream) {
  US_CHECK_ARG(sites && d2, "edt_sqdist: null pointer");
  long total;
  if (boundary_geometry("edt_sqdist", N, H, W, total)) return 1;
  launch_edt_sqdist(sites, N, H, W, d2, (hipStream_t)stream);
  US_LAUNCH_CHECK("edt_sqdist");
  return 0;
}

// counts int64 [2 (K + 2) + 2] += the two edge-distance histograms and the Boundary-IoU intersection and
// union (see the head of this file); eP / eG the edge maps of pred / target for class c, dP / dG their
// distance transforms
UNETSEG_API int unetseg_boundary_counts(const int32_t* pred, const int32_t* target, const uint8_t* eP,
                                        const uint8_t* eG, const int32_t* dP, const int32_t* dG, int N, int H, int W,
                                        int c, int ignore, int K, int biou_d2, int64_t* counts, void* stream) {
  US_CHECK_ARG(pred && target && eP && eG && dP && dG && counts, "boundary_counts: null pointer");
  US_CHECK_ARG(K >= 0 && K <= kMaxK, "boundary_counts: K = %d outside 0 .. %d", K, kMaxK);
  US_CHECK_ARG(biou_d2 >= 0 && biou_d2 <= K, "boundary_counts: biou_d2 = %d outside 0 .. K = %d", biou_d2, K);
  long total;
  if (boundary_geometry("boundary_counts", N, H, W, total)) return 1;
  // a block's 32-bit LDS counters hold its share of the pixels: 1024 blocks of up to 2^32 each
  US_CHECK_ARG(total <= (1L << 40), "boundary_counts: N * H * W = %ld exceeds 2^40 pixels", total);
  const int windows = (2 * (K + 2) + kBins - 1) / kBins;
  hipLaunchKernelGGL(boundary_counts_kernel, dim3(grid_for(total, 1024), windows), dim3(256), 0, (hipStream_t)stream,
                     pred, target, eP, eG, dP, dG, total, c, ignore, K, biou_d2, (unsigned long long*)counts);
  US_LAUNCH_CHECK("boundary_counts");
  return 0;
}
