// Score histogram of the binary head (unetseg_hip/curve.py: the operating-point and calibration metrics of
// val.py and of the evaluate loops; no reference counterpart).
//
// hist u64 [2][K] += per valid pixel: row = (tgt == 1), column = bin(z), where z = o0 (nch 1) or o1 - o0
// (nch 2, one fp32 subtraction) and bin(z) = the number of edges theta with z > theta.  The kernel does no
// other arithmetic on z: the bin is decided by comparisons with the caller's edge array alone, so a CPU
// reference that holds the same array reproduces every count.
//
// A block keeps the K - 1 edges and a private u32 [2][K] histogram in LDS (12 K bytes, 48 KB at the largest K).
//   * End bins.  A trained model puts most pixels below the first edge or above the last one.  Those are
//     counted in four registers per thread (!(z > first) and z > last: two comparisons, no LDS access) and
//     reach the block histogram as one LDS add per wave and counter.  A wave all of whose pixels are end-bin
//     pixels skips the search altogether.
//   * Middle bins.  pos = 0; for s = 2^j down to 1: if (pos + s <= K - 1 && z > edge[pos + s - 1]) pos += s.
//     For ascending edges that is the count of edges below z; for any edge array pos stays in 0 .. K - 1,
//     because it only grows under pos + s <= K - 1.  NaN compares false everywhere (bin 0; it never reaches
//     the search), a value equal to an edge stays below it, +-inf end in the end bins.  The steps are the same
//     for every lane, so the wave does not diverge inside the search.  One LDS add per middle pixel.
//   * Flush.  The non-zero block counters are added to the u64 histogram with integer atomics, consecutive
//     lanes on consecutive bins.  At most kCurveGrid blocks run, so a launch sends at most kCurveGrid * 2 K
//     of them, and a block's u32 counters hold its share of the 2^40 pixels a call takes.
// Pixels are taken in groups of four of the flat batch (seg_pixel.h: 16-byte loads where the group's
// addresses are 16-byte aligned, element loads elsewhere, e.g. in the later images of a batch with odd P);
// tgt is compared as int64.  Integer counts and integer atomics only: the result is bitwise reproducible.
#include "seg_pixel.h"

namespace {

constexpr int kCurveMaxBins = 4096;
constexpr int kCurveGrid = 512;  // two blocks per CU; at [16,2,512,512] a block sees 8192 pixels

__global__ __launch_bounds__(256) void curve_hist_kernel(const float* out, int nch, const int64_t* tgt, long P,
                                                         long total, int has_ignore, long ignore,
                                                         const float* edges, int K, int top,
                                                         unsigned long long* hist) {
  extern __shared__ unsigned curve_lds[];
  float* se = reinterpret_cast<float*>(curve_lds);  // [K]: K - 1 edges (the last entry is unused)
  unsigned* sh = curve_lds + K;                     // [2][K]
  const int ne = K - 1;
  for (int i = threadIdx.x; i < ne; i += 256) se[i] = edges[i];
  for (int i = threadIdx.x; i < 2 * K; i += 256) sh[i] = 0;
  __syncthreads();
  const float first = se[0], last = se[ne - 1];
  unsigned c_lo[2] = {0, 0}, c_hi[2] = {0, 0};  // [row]: pixels of bin 0 and of bin K - 1
  const long groups = (total + 3) / 4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;
    long t[4];
    float z[4];
    ld_group(tgt + i0, m, t);
    ld_logit_group(out, nch, P, i0, m, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= m || (has_ignore && t[k] == ignore)) continue;
      const int row = t[k] == 1;
      if (!(z[k] > first)) {  // NaN too
        c_lo[row] += 1;
      } else if (z[k] > last) {
        c_hi[row] += 1;
      } else {
        int pos = 0;
        for (int s = top; s > 0; s >>= 1)
          if (pos + s <= ne && z[k] > se[pos + s - 1]) pos += s;
        atomicAdd(sh + row * K + pos, 1u);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    unsigned lo = c_lo[r], hi = c_hi[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo += __shfl_xor(lo, o, 64), hi += __shfl_xor(hi, o, 64);
    if ((threadIdx.x & 63) == 0) {
      if (lo) atomicAdd(sh + r * K, lo);
      if (hi) atomicAdd(sh + r * K + K - 1, hi);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K; i += 256) {
    const unsigned v = sh[i];
    if (v) atomicAdd(hist + i, (unsigned long long)v);
  }
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// host only: the largest K unetseg_curve_hist takes
UNETSEG_API int unetseg_curve_max_bins(void) { return kCurveMaxBins; }

// hist u64 [2][K] += per pixel whose target is not ignore_index (-1: none): row = (tgt == 1), column = the
// number of edges (device fp32 [K - 1], ascending) below z (see the head of this file)
UNETSEG_API int unetseg_curve_hist(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index,
                                   const float* edges, int K, unsigned long long* hist, void* stream) {
  US_CHECK_ARG(out && tgt && edges && hist, "curve_hist: null pointer");
  US_CHECK_ARG(nch == 1 || nch == 2, "curve_hist: nch %d must be 1 or 2", nch);
  US_CHECK_ARG(K >= 2 && K <= kCurveMaxBins, "curve_hist: K %d outside 2 .. %d", K, kCurveMaxBins);
  US_CHECK_ARG(B >= 0 && P >= 0, "curve_hist: bad shape B=%d P=%ld", B, P);
  constexpr long kMaxPixels = 1L << 40;  // a block's 32-bit counters hold its share (kCurveGrid blocks)
  US_CHECK_ARG(B == 0 || P <= kMaxPixels / B, "curve_hist: B=%d P=%ld is more than 2^40 pixels", B, P);
  const long total = (long)B * P;
  if (total == 0) return 0;
  int top = 1;  // the largest power of two <= K - 1
  while (top * 2 <= K - 1) top *= 2;
  hipLaunchKernelGGL(curve_hist_kernel, dim3(grid_for((total + 3) / 4, kCurveGrid)), dim3(256),
                     (size_t)3 * K * sizeof(unsigned), (hipStream_t)stream, out, nch, tgt, P, total,
                     (int)(ignore_index != -1), ignore_index, edges, K, top, hist);
  US_LAUNCH_CHECK("curve_hist");
  return 0;
}
