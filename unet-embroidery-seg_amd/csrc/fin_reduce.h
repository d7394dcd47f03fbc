// Row-partial reductions: the device helpers and launch geometry of the kernels that reduce
// part[g][q][C] over the row tiles g (the BN finalizes and the bias-gradient column sums in bn.hip).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------
// Per-channel reductions of row partials part[g][q][C] (G row tiles, q = 0 .. nq-1) -- the BN
// finalizes of the forward statistics and of the fused data-gradient post-ops.  They sit on the
// compute stream between a producer and its consumer, so they are latency kernels: one wave per
// channel (NWV = 1, four channels per block, no barrier) when G <= 512, a block of NWV = 4 waves per
// channel above that; every lane issues all its loads (kFinRPL rows x nq) before it adds, and the
// lanes' fp64 partials are combined in a fixed order (deterministic).  Never 1024-thread blocks: beside
// the weight-gradient stream's persistent kernels such a block found no CU until they drained (a
// 12 us colsum took 235 us in the bench trace); 256-thread blocks ran at their isolated speed.
// ------------------------------------------------------------------------------------------
constexpr int kFinRPL = 8;  // rows per lane per round

static inline int fin_waves(int G) { return G > 512 ? 4 : 1; }
static inline unsigned fin_blocks(int C, int nwv) { return nwv > 1 ? (unsigned)C : (unsigned)ceil_div(C, 4); }
static inline unsigned fin_threads(int nwv) { return nwv > 1 ? 64u * nwv : 256u; }
// launch KERNEL<nwv> for the row count G with the finalize geometry
#define FIN_LAUNCH(KERNEL, C, G, stream, ...)                                                                  \
  do {                                                                                                     \
    const int nwv_ = fin_waves(G);                                                                         \
    const dim3 grid_(fin_blocks(C, nwv_)), block_(fin_threads(nwv_));                                      \
    if (nwv_ == 4) hipLaunchKernelGGL(KERNEL<4>, grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL<1>, grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);              \
  } while (0)

// fp64 sum over the wave, the same value in every lane: row rotations on the VALU (each 64-bit value
// moved as two DPP halves) leave every lane of a 16-lane row with the row's total, then the four row
// totals are read lane-uniform and added in a fixed order.  wave_sum_d (__shfl_xor) went through
// ds_bpermute, two LDS round trips per step for a double: the finalize kernels sat on that chain
template <int CTL>
__device__ __forceinline__ double row_rot_add_d(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTL, 0xF, 0xF, false);
  const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTL, 0xF, 0xF, false);
  return v + __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double wave_sum_d_uniform(double v) {
  v = row_rot_add_d<0x128>(v);  // row_ror:8
  v = row_rot_add_d<0x124>(v);  // row_ror:4
  v = row_rot_add_d<0x122>(v);  // row_ror:2
  v = row_rot_add_d<0x121>(v);  // row_ror:1
  const int lo = __double2loint(v), hi = __double2hiint(v);
  double t = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    t += __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * r), __builtin_amdgcn_readlane(lo, 16 * r));
  return t;
}

// sum over the channel's lanes (one wave, or the block's NWV waves through sc[NQ][NWV]); every lane
// gets the same fixed-order total
template <int NWV, int NQ>
__device__ __forceinline__ void fin_group_sum(double (&v)[NQ], double* sc) {
#pragma unroll
  for (int j = 0; j < NQ; ++j) v[j] = wave_sum_d_uniform(v[j]);
  if constexpr (NWV > 1) {
    const int wid = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int j = 0; j < NQ; ++j) sc[j * NWV + wid] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < NWV; ++w) t += sc[j * NWV + w];
      v[j] = t;
    }
  }
}

// t[j] = sum_g part[g * ldrow + (q0 + j) * C + c] for j < nq (NQ >= nq)
template <int NWV, int NQ>
__device__ __forceinline__ void fin_row_sums(const float* part, long ldrow, int C, int c, int G, int nq, int q0,
                                             double (&t)[NQ], double* sc) {
  constexpr int NL = 64 * NWV;
  const int li = NWV == 1 ? (threadIdx.x & 63) : threadIdx.x;
#pragma unroll
  for (int j = 0; j < NQ; ++j) t[j] = 0.0;
  for (int g0 = 0; g0 < G; g0 += kFinRPL * NL) {
    // every load unconditional (a row past G re-reads row G - 1, a quantity past nq the last one) and
    // masked after it: a load under a lane condition got its own branch and a vmcnt(0) behind it, which
    // serialised all kFinRPL x NQ round trips of the lane
    float v[NQ][kFinRPL];
#pragma unroll
    for (int k = 0; k < kFinRPL; ++k) {
      const int g = min(g0 + li + k * NL, G - 1);
#pragma unroll
      for (int j = 0; j < NQ; ++j) v[j][k] = part[g * ldrow + (long)(q0 + min(j, nq - 1)) * C + c];
    }
#pragma unroll
    for (int k = 0; k < kFinRPL; ++k) {
      const bool ok = g0 + li + k * NL < G;
#pragma unroll
      for (int j = 0; j < NQ; ++j) t[j] += (ok && j < nq) ? (double)v[j][k] : 0.0;
    }
  }
  fin_group_sum<NWV, NQ>(t, sc);
}

}  // namespace
