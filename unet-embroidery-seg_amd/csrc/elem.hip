// BatchNorm (train / eval) of the U-Net hot path, NHWC: forward statistics finalize, fold, apply (with
// the ReLU, the residual and the packed ReLU mask), the three backward passes, the ReLU-backward bias
// gradient, and the row-partial finalize family of the fused data-gradient post-ops.
//
// Reference ops replaced:
//   BatchNorm2d      model/resnet_backbone.py:64-70,127,169  model/unet_plain.py:10,13
//                    model/unet_attention.py:17,21,25
//   ReLU / residual  model/resnet_backbone.py:95,100,110,113  model/unet_resnet.py:37,40,73,75
//
// Layout: activations NHWC with an explicit pixel stride ("ld", elements) so channel slices of a
// concat buffer are addressed in place.  Element type T is bf16 or fp32; all arithmetic is fp32.
// Every per-channel reduction is two-stage (per-block partials -> finalize) and deterministic.
#include "elem_util.h"
#include "fin_reduce.h"

namespace {

// ------------------------------------------------------------------------------------------
// BatchNorm finalize (train): partials [G][2][C] = (sum, M2 about the tile mean) with tile
// count min(tile, M - g*tile).  Chan's parallel merge in fp64.  Updates running stats exactly as
// nn.BatchNorm2d (momentum 0.1, unbiased running var) and emits scale/shift for the apply pass.
// ------------------------------------------------------------------------------------------
template <int NWV>
__global__ __launch_bounds__(NWV > 4 ? 64 * NWV : 256) void bn_finalize_kernel(const float* part, int C, int G, long M, int tile,
                                                          const float* gamma, const float* beta, float* rmean,
                                                          float* rvar, long long* nbt, float momentum, float eps,
                                                          float* mean_out, float* invstd_out, float* scale,
                                                          float* shift) {
  __shared__ double sc[NWV];
  constexpr int NL = 64 * NWV;
  const int c = NWV == 1 ? (int)blockIdx.x * 4 + (threadIdx.x >> 6) : (int)blockIdx.x;
  if (NWV == 1 && c >= C) return;  // whole waves: no barrier in the one-wave form
  const int li = NWV == 1 ? (threadIdx.x & 63) : threadIdx.x;
  const long st = 2L * C;
  // the epilogue's operands loaded up front (behind the reductions each was a round trip)
  const float gam = gamma[c], bet = beta[c];
  const float rm0 = (rmean ? rmean : gamma)[c], rv0 = (rmean ? rvar : gamma)[c];  // unused without rmean
  // pass 1 keeps this lane's rows in registers when one round covers G (pass 2 re-reads otherwise)
  float sv[kFinRPL], qv[kFinRPL];
  double tsum[1] = {0.0};
  // unconditional loads (a row past G re-reads row G - 1), masked after: see fin_row_sums
  for (int g0 = 0; g0 < G; g0 += kFinRPL * NL) {
#pragma unroll
    for (int k = 0; k < kFinRPL; ++k) {
      const int g = min(g0 + li + k * NL, G - 1);
      sv[k] = part[g * st + c];
      qv[k] = part[g * st + C + c];
    }
#pragma unroll
    for (int k = 0; k < kFinRPL; ++k) {
      if (g0 + li + k * NL >= G) sv[k] = qv[k] = 0.f;
      tsum[0] += (double)sv[k];
    }
  }
  fin_group_sum<NWV, 1>(tsum, sc);
  const double mean = tsum[0] / (double)M;
  double m2[1] = {0.0};
  const bool one_round = G <= kFinRPL * NL;
  for (int g0 = 0; g0 < G; g0 += kFinRPL * NL) {
    if (!one_round) {
#pragma unroll
      for (int k = 0; k < kFinRPL; ++k) {
        const int g = min(g0 + li + k * NL, G - 1);
        sv[k] = part[g * st + c];
        qv[k] = part[g * st + C + c];
      }
    }
#pragma unroll
    for (int k = 0; k < kFinRPL; ++k) {
      const int g = g0 + li + k * NL;
      if (g < G) {
        const long cnt = min((long)tile, M - (long)g * tile);
        const double mg = (double)sv[k] / (double)cnt;
        m2[0] += (double)qv[k] + (double)cnt * (mg - mean) * (mg - mean);
      }
    }
  }
  fin_group_sum<NWV, 1>(m2, sc);
  if (li == 0) {
    const double m2v = m2[0];
    const double var = m2v / (double)M;
    const double inv = 1.0 / sqrt(var + (double)eps);
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)inv;
    const float sca = (float)(gam * inv);
    scale[c] = sca;
    shift[c] = (float)(bet - mean * gam * inv);
    if (rmean) {
      const double unb = M > 1 ? m2v / (double)(M - 1) : var;
      rmean[c] = (float)((1.0 - momentum) * rm0 + momentum * mean);
      rvar[c] = (float)((1.0 - momentum) * rv0 + momentum * unb);
    }
    if (nbt && c == 0) nbt[0] += 1;
  }
}

// eval-mode BN folded into the preceding conv: kscale = gamma / sqrt(var + eps),
// bias = beta - mean * kscale (+ conv_bias * kscale)
__global__ void bn_fold_kernel(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                               float eps, const float* conv_bias, float* kscale, float* bias) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  // the same float expressions as bn_eval_kernel, so the folded epilogue fmaf(acc, kscale, bias)
  // equals the unfolded BN pass fmaf(y, scale, shift) bit for bit in fp32
  const float inv = 1.0f / sqrtf(rvar[c] + eps);
  const float sc = gamma[c] * inv;
  kscale[c] = sc;
  const float sh = beta[c] - rmean[c] * gamma[c] * inv;
  bias[c] = conv_bias ? sh + conv_bias[c] * sc : sh;
}

__global__ void bn_eval_kernel(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                               float eps, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float inv = 1.0f / sqrtf(rvar[c] + eps);
  scale[c] = gamma[c] * inv;
  shift[c] = beta[c] - rmean[c] * gamma[c] * inv;
}

// out = act(y*sc + sh + res); res: 0 none, 1 raw tensor r, 2 r*sc2 + sh2
// mbits (may be NULL): the ReLU mask of `out` packed one byte per (pixel, V-channel vector), bit e =
// (stored out[c0 + e] > 0), [M][C/V] -- the BN backward reads it instead of the whole activation
template <typename T>
__global__ void bn_apply_kernel(const T* y, int ldy, const float* sc, const float* sh, const T* r, int ldr,
                                const float* sc2, const float* sh2, int res_mode, int relu, T* out, int ldo, long M,
                                int C, uint8_t* mbits) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const long total = M * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / cv;
    const int c0 = (int)(i - pix * cv) * V;
    float v[V], rv[V];
    load_vec(y + pix * ldy + c0, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = fmaf(v[e], sc[c0 + e], sh[c0 + e]);  // == bwd mask recompute
    if (res_mode) {
      load_vec(r + pix * ldr + c0, rv);
      if (res_mode == 2) {
#pragma unroll
        for (int e = 0; e < V; ++e) rv[e] = rv[e] * sc2[c0 + e] + sh2[c0 + e];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] += rv[e];
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    store_vec(out + pix * ldo + c0, v);
    if (mbits) {
      unsigned b = 0u;
#pragma unroll
      for (int e = 0; e < V; ++e) b |= ((float)(T)v[e] > 0.f ? 1u : 0u) << e;
      mbits[i] = (uint8_t)b;  // i == pix * cv + c0 / V
    }
  }
}

// ------------------------------------------------------------------------------------------
// Channel reductions over pixels (BN backward pass 1, ReLU-backward bias gradient).
// Block = 256 threads = tv channel vectors (16 B each) x rows pixel rows; each thread walks its
// pixel rows RU at a time with every load of the group issued before any use (the loads of a
// group are independent, so a wave keeps RU x tensors 16-B requests in flight).  Per-thread sums
// are folded across the wave's pixel rows with xor-shuffles (lanes with equal tx), then across
// the 4 waves through LDS.  Partials: part[k][C][G] (k = quantity), one column per block row.
// ------------------------------------------------------------------------------------------
constexpr int RU = 4;

// sum over the lanes of a wave that share (lane % tv); result valid in every lane
__device__ __forceinline__ float rows_sum(float v, int tv) {
  for (int o = tv; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// NQ quantities x V channels per thread -> part[k][C][G] column blockIdx.x
template <int NQ, int V>
__device__ __forceinline__ void store_partials(float (&s)[NQ][V], int tv, int c0, int C, int G, float* part,
                                               float* red /* [4][NQ][64][V] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, tx = threadIdx.x % tv;
#pragma unroll
  for (int k = 0; k < NQ; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) s[k][e] = rows_sum(s[k][e], tv);
  if (lane < tv) {
#pragma unroll
    for (int k = 0; k < NQ; ++k)
#pragma unroll
      for (int e = 0; e < V; ++e) red[((w * NQ + k) * 64 + tx) * V + e] = s[k][e];
  }
  __syncthreads();
  constexpr int nw = 4;  // waves per block (256 threads)
  const int cb = c0 - tx * V;        // first channel of this block's group
  for (int idx = threadIdx.x; idx < NQ * tv * V; idx += 256) {
    const int k = idx / (tv * V), rem = idx - k * tv * V;
    const int cx = rem / V, e = rem - cx * V;
    float t = 0.f;
    for (int ww = 0; ww < nw; ++ww) t += red[((ww * NQ + k) * 64 + cx) * V + e];
    part[((long)k * C + cb + cx * V + e) * G + blockIdx.x] = t;
  }
}

// BatchNorm backward, pass 1: per-(channel, pixel tile) partials of
//   sum dz, sum dz*xhat1, sum dz*xhat2     where dz = dA * mask
// MASK: 0 none, 1 (A > 0), 2 (y1*msc + msh > 0) -- the ReLU mask recomputed exactly as bn_apply
// produced A, 3 the packed mask bn_apply wrote (A = mbits [M][C/V] bytes).  Y2: second BN branch
// (downsample shortcut) present.
template <typename T, int MASK, bool Y2>
__device__ __forceinline__ void bn_bwd_reduce_body(const T* dA, int ldd, const T* A, int lda, const float* msc,
                                                   const float* msh, const T* y1, int ld1, const float* mean1,
                                                   const float* inv1, const T* y2, int ld2, const float* mean2,
                                                   const float* inv2, long M, int C, int tv, int pix_per_block,
                                                   float* part, int G) {
  constexpr int V = VE<T>;
  constexpr int NQ = Y2 ? 3 : 2;
  __shared__ float red[4 * 3 * 64 * V];
  const int tx = threadIdx.x % tv, ty = threadIdx.x / tv, rows = 256 / tv;
  const int c0 = (blockIdx.y * tv + tx) * V;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  float s[NQ][V], m1[V], i1[V], m2v[V], i2v[V], ms[V], mh[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) s[k][e] = 0.f;
    m1[e] = mean1[c0 + e];
    i1[e] = inv1[c0 + e];
    m2v[e] = Y2 ? mean2[c0 + e] : 0.f;
    i2v[e] = Y2 ? inv2[c0 + e] : 0.f;
    ms[e] = MASK == 2 ? msc[c0 + e] : 0.f;
    mh[e] = MASK == 2 ? msh[c0 + e] : 0.f;
  }
  const uint8_t* mb = reinterpret_cast<const uint8_t*>(A);
  const int cv = C / V;
  auto acc = [&](const uint4& rd, const uint4& rx, const uint4& ra, const uint4& r2) {
    float d[V], x[V];
    cvt16<T>(rd, d);
    cvt16<T>(rx, x);
    if (MASK == 3) {
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = (ra.x >> e) & 1u ? d[e] : 0.f;
    } else if (MASK == 1) {
      float a[V];
      cvt16<T>(ra, a);
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = a[e] > 0.f ? d[e] : 0.f;
    } else if (MASK == 2) {
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = fmaf(x[e], ms[e], mh[e]) > 0.f ? d[e] : 0.f;
    }
    // explicit fmaf: the same rounding in every MASK / Y2 instantiation (the compiler's own
    // contraction choices differed between them)
#pragma unroll
    for (int e = 0; e < V; ++e) {
      s[0][e] += d[e];
      s[1][e] = fmaf(d[e], (x[e] - m1[e]) * i1[e], s[1][e]);
    }
    if (Y2) {
      float x2[V];
      cvt16<T>(r2, x2);
#pragma unroll
      for (int e = 0; e < V; ++e) s[NQ - 1][e] = fmaf(d[e], (x2[e] - m2v[e]) * i2v[e], s[NQ - 1][e]);
    }
  };
  long p = p0 + ty;
  for (; p + (long)(RU - 1) * rows < p1; p += (long)RU * rows) {
    uint4 rd[RU], rx[RU], ra[RU], r2[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const long q = p + (long)u * rows;
      rd[u] = *reinterpret_cast<const uint4*>(dA + q * ldd + c0);
      rx[u] = *reinterpret_cast<const uint4*>(y1 + q * ld1 + c0);
      if (MASK == 1) ra[u] = *reinterpret_cast<const uint4*>(A + q * lda + c0);
      if (MASK == 3) ra[u].x = mb[q * cv + c0 / V];
      if (Y2) r2[u] = *reinterpret_cast<const uint4*>(y2 + q * ld2 + c0);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) acc(rd[u], rx[u], ra[u], r2[u]);
  }
  for (; p < p1; p += rows) {
    uint4 rd = *reinterpret_cast<const uint4*>(dA + p * ldd + c0), ra = rd, r2 = rd;
    const uint4 rx = *reinterpret_cast<const uint4*>(y1 + p * ld1 + c0);
    if (MASK == 1) ra = *reinterpret_cast<const uint4*>(A + p * lda + c0);
    if (MASK == 3) ra.x = mb[p * cv + c0 / V];
    if (Y2) r2 = *reinterpret_cast<const uint4*>(y2 + p * ld2 + c0);
    acc(rd, rx, ra, r2);
  }
  store_partials<NQ, V>(s, tv, c0, C, G, part, red);
}

#define BN_RED_PARAMS                                                                                             \
  const T *dA, int ldd, const T *A, int lda, const float *msc, const float *msh, const T *y1, int ld1,            \
      const float *mean1, const float *inv1, const T *y2, int ld2, const float *mean2, const float *inv2, long M, \
      int C, int tv, int pix_per_block, float *part, int G
#define BN_RED_ARGS dA, ldd, A, lda, msc, msh, y1, ld1, mean1, inv1, y2, ld2, mean2, inv2, M, C, tv, pix_per_block, part, G
template <typename T, int MASK, bool Y2>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BN_RED_PARAMS) {
  bn_bwd_reduce_body<T, MASK, Y2>(BN_RED_ARGS);
}
// the packed-mask variant (one branch) with a register budget of four waves per SIMD: under the
// default target the scheduler serialised its main loop -- each of the 12 loads of an RU group waited on
// before the next was issued: 19.7 -> 14.5 us (C2's call), 17.1 -> 10.2 (C5's two).  With the second
// branch (Y2) the budget measured slower (12.2 -> 13.9 us): that one keeps the plain kernel
template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void bn_bwd_reduce_bits_kernel(
    BN_RED_PARAMS) {
  bn_bwd_reduce_body<T, 3, false>(BN_RED_ARGS);
}
#undef BN_RED_PARAMS
#undef BN_RED_ARGS

// pass 2: coefficients.  For branch b (1 or 2): dgamma_b += sum dz*xhat_b, dbeta_b += sum dz;
// coef[b][0][c] = gamma_b*invstd_b, coef[b][1][c] = mean(dz), coef[b][2][c] = mean(dz*xhat_b)
__global__ void bn_bwd_finalize_kernel(const float* part, int C, int G, long M, int nbranch, const float* g1,
                                       const float* inv1, float* dg1, float* db1, const float* g2, const float* inv2,
                                       float* dg2, float* db2, float* coef) {
  __shared__ double sc[16];
  const int c = blockIdx.x;
  double t[3] = {0, 0, 0};
  for (int k = 0; k < 1 + nbranch; ++k) {
    double acc = 0.0;
    for (int g = threadIdx.x; g < G; g += blockDim.x) acc += part[((long)k * C + c) * G + g];
    t[k] = block_sum(acc, sc);
  }
  if (threadIdx.x == 0) {
    const double sdz = t[0];
    dg1[c] += (float)t[1];
    db1[c] += (float)sdz;
    coef[0 * C + c] = g1[c] * inv1[c];
    coef[1 * C + c] = (float)(sdz / (double)M);
    coef[2 * C + c] = (float)(t[1] / (double)M);
    if (nbranch == 2) {
      dg2[c] += (float)t[2];
      db2[c] += (float)sdz;
      coef[3 * C + c] = g2[c] * inv2[c];
      coef[4 * C + c] = (float)(sdz / (double)M);
      coef[5 * C + c] = (float)(t[2] / (double)M);
    }
  }
}

// pass 3: dy_b = coef_a*(dz - mean(dz) - xhat_b*mean(dz*xhat_b)); optional dzout (+)= dz.
// Same block geometry as pass 1 (fixed channels per thread): the per-channel coefficients are
// folded once into dy_b = P_b*dz + Q_b*(y_b - mean_b) + R_b and kept in registers.  DZ: 0 none, 1 store,
// 2 accumulate.
template <typename T, int MASK, bool Y2, int DZ>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* dA, int ldd, const T* A, int lda,
                                                           const float* msc, const float* msh, const T* y1, int ld1,
                                                           const float* mean1, const float* inv1, T* dy1, int ldo1,
                                                           const T* y2, int ld2, const float* mean2, const float* inv2,
                                                           T* dy2, int ldo2, const float* coef, T* dzout, int ldz,
                                                           long M, int C, int tv, int pix_per_block) {
  constexpr int V = VE<T>;
  const int tx = threadIdx.x % tv, ty = threadIdx.x / tv, rows = 256 / tv;
  const int c0 = (blockIdx.y * tv + tx) * V;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  float P1[V], Q1[V], R1[V], M1[V], P2[V], Q2[V], R2[V], M2[V], ms[V], mh[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int c = c0 + e;
    const float k1 = coef[c], cx1 = coef[2 * C + c] * inv1[c];
    P1[e] = k1;
    Q1[e] = -k1 * cx1;
    R1[e] = -k1 * coef[C + c];
    M1[e] = mean1[c];
    if (Y2) {
      const float k2 = coef[3 * C + c], cx2 = coef[5 * C + c] * inv2[c];
      P2[e] = k2;
      Q2[e] = -k2 * cx2;
      R2[e] = -k2 * coef[4 * C + c];
      M2[e] = mean2[c];
    }
    ms[e] = MASK == 2 ? msc[c] : 0.f;
    mh[e] = MASK == 2 ? msh[c] : 0.f;
  }
  const uint8_t* mb = reinterpret_cast<const uint8_t*>(A);
  const int cv = C / V;
  auto one = [&](long q, const uint4& rd, const uint4& rx, const uint4& ra, const uint4& r2, const uint4& rz) {
    float d[V], x[V], o[V];
    cvt16<T>(rd, d);
    cvt16<T>(rx, x);
    if (MASK == 3) {
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = (ra.x >> e) & 1u ? d[e] : 0.f;
    } else if (MASK == 1) {
      float a[V];
      cvt16<T>(ra, a);
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = a[e] > 0.f ? d[e] : 0.f;
    } else if (MASK == 2) {
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = fmaf(x[e], ms[e], mh[e]) > 0.f ? d[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = fmaf(P1[e], d[e], fmaf(Q1[e], x[e] - M1[e], R1[e]));
    store_vec(dy1 + q * ldo1 + c0, o);
    if (Y2) {
      cvt16<T>(r2, x);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = fmaf(P2[e], d[e], fmaf(Q2[e], x[e] - M2[e], R2[e]));
      store_vec(dy2 + q * ldo2 + c0, o);
    }
    if (DZ == 2) {
      cvt16<T>(rz, o);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] += d[e];
      store_vec(dzout + q * ldz + c0, o);
    } else if (DZ == 1) {
      store_vec(dzout + q * ldz + c0, d);
    }
  };
  long p = p0 + ty;
  for (; p + (long)(RU - 1) * rows < p1; p += (long)RU * rows) {
    uint4 rd[RU], rx[RU], ra[RU], r2[RU], rz[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const long q = p + (long)u * rows;
      rd[u] = *reinterpret_cast<const uint4*>(dA + q * ldd + c0);
      rx[u] = *reinterpret_cast<const uint4*>(y1 + q * ld1 + c0);
      if (MASK == 1) ra[u] = *reinterpret_cast<const uint4*>(A + q * lda + c0);
      if (MASK == 3) ra[u].x = mb[q * cv + c0 / V];
      if (Y2) r2[u] = *reinterpret_cast<const uint4*>(y2 + q * ld2 + c0);
      if (DZ == 2) rz[u] = *reinterpret_cast<const uint4*>(dzout + q * ldz + c0);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) one(p + (long)u * rows, rd[u], rx[u], ra[u], r2[u], rz[u]);
  }
  for (; p < p1; p += rows) {
    const uint4 rd = *reinterpret_cast<const uint4*>(dA + p * ldd + c0);
    const uint4 rx = *reinterpret_cast<const uint4*>(y1 + p * ld1 + c0);
    uint4 ra = rd, r2 = rd, rz = rd;
    if (MASK == 1) ra = *reinterpret_cast<const uint4*>(A + p * lda + c0);
    if (MASK == 3) ra.x = mb[p * cv + c0 / V];
    if (Y2) r2 = *reinterpret_cast<const uint4*>(y2 + p * ld2 + c0);
    if (DZ == 2) rz = *reinterpret_cast<const uint4*>(dzout + p * ldz + c0);
    one(p, rd, rx, ra, r2, rz);
  }
}

// dY = dA * (A > 0) and per-tile column sums of dY (bias gradient partials [C][G])
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_bias_kernel(const T* dA, int ldd, const T* A, int lda, T* dY, int ldy,
                                                            long M, int C, int tv, int pix_per_block, float* part,
                                                            int G) {
  constexpr int V = VE<T>;
  __shared__ float red[4 * 64 * V];
  const int tx = threadIdx.x % tv, ty = threadIdx.x / tv, rows = 256 / tv;
  const int c0 = (blockIdx.y * tv + tx) * V;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  float s[1][V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[0][e] = 0.f;
  auto one = [&](long q, const uint4& rd, const uint4& ra) {
    float d[V], a[V];
    cvt16<T>(rd, d);
    cvt16<T>(ra, a);
    // round like the stored gradient so db == sum of the dY actually fed to wgrad
    T tmp[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      tmp[e] = (T)(a[e] > 0.f ? d[e] : 0.f);
      s[0][e] += (float)tmp[e];
    }
    *reinterpret_cast<uint4*>(dY + q * ldy + c0) = *reinterpret_cast<uint4*>(tmp);
  };
  long p = p0 + ty;
  for (; p + (long)(RU - 1) * rows < p1; p += (long)RU * rows) {
    uint4 rd[RU], ra[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const long q = p + (long)u * rows;
      rd[u] = *reinterpret_cast<const uint4*>(dA + q * ldd + c0);
      ra[u] = *reinterpret_cast<const uint4*>(A + q * lda + c0);
    }
#pragma unroll
    for (int u = 0; u < RU; ++u) one(p + (long)u * rows, rd[u], ra[u]);
  }
  for (; p < p1; p += rows)
    one(p, *reinterpret_cast<const uint4*>(dA + p * ldd + c0), *reinterpret_cast<const uint4*>(A + p * lda + c0));
  store_partials<1, V>(s, tv, c0, C, G, part, red);
}

// The same coefficients from the row partials of a fused data-gradient post-op
// (unetseg_conv2d_dgrad_post): part[g][2][C] = (sum dz, sum dz*xhat) per row tile.
template <int NWV>
__global__ __launch_bounds__(NWV > 4 ? 64 * NWV : 256) void bn_bwd_finalize_rows_kernel(const float* part, int C, int G, long M,
                                                                   const float* g1, const float* inv1, float* dg1,
                                                                   float* db1, float* coef) {
  __shared__ double sc[2 * NWV];
  const int c = NWV == 1 ? (int)blockIdx.x * 4 + (threadIdx.x >> 6) : (int)blockIdx.x;
  if (NWV == 1 && c >= C) return;
  // the epilogue's operands loaded up front: behind the reduction each was another round trip
  const float pg = dg1[c], pb = db1[c], k1 = g1[c] * inv1[c];
  double t[2];
  fin_row_sums<NWV, 2>(part, 2L * C, C, c, G, 2, 0, t, sc);
  if ((NWV == 1 ? (threadIdx.x & 63) : threadIdx.x) == 0) {
    const double a0 = t[0], a1 = t[1];
    dg1[c] = pg + (float)a1;
    db1[c] = pb + (float)a0;
    coef[0 * C + c] = k1;
    coef[1 * C + c] = (float)(a0 / (double)M);
    coef[2 * C + c] = (float)(a1 / (double)M);
  }
}

// The two-branch form for the residual post-op (unetseg_conv2d_dgrad_post_res): part[g][1+nbranch][C] =
// (sum dz, sum dz*xhat1 [, sum dz*xhat2]) per row tile; coefficients as bn_bwd_finalize_kernel.
template <int NWV>
__global__ __launch_bounds__(NWV > 4 ? 64 * NWV : 256) void bn_bwd_finalize_rows_res_kernel(const float* part, int C, int G, long M,
                                                                       int nbranch, const float* g1,
                                                                       const float* inv1, float* dg1, float* db1,
                                                                       const float* g2, const float* inv2, float* dg2,
                                                                       float* db2, float* coef) {
  __shared__ double sc[3 * NWV];
  const int c = NWV == 1 ? (int)blockIdx.x * 4 + (threadIdx.x >> 6) : (int)blockIdx.x;
  if (NWV == 1 && c >= C) return;
  const int nq = 1 + nbranch;
  const float pg1 = dg1[c], pb1 = db1[c], k1 = g1[c] * inv1[c];
  float pg2 = 0.f, pb2 = 0.f, k2 = 0.f;
  if (nbranch == 2) {
    pg2 = dg2[c];
    pb2 = db2[c];
    k2 = g2[c] * inv2[c];
  }
  double t[3];
  fin_row_sums<NWV, 3>(part, (long)nq * C, C, c, G, nq, 0, t, sc);
  if ((NWV == 1 ? (threadIdx.x & 63) : threadIdx.x) == 0) {
    const double sdz = t[0];
    dg1[c] = pg1 + (float)t[1];
    db1[c] = pb1 + (float)sdz;
    coef[0 * C + c] = k1;
    coef[1 * C + c] = (float)(sdz / (double)M);
    coef[2 * C + c] = (float)(t[1] / (double)M);
    if (nbranch == 2) {
      dg2[c] = pg2 + (float)t[2];
      db2[c] = pb2 + (float)sdz;
      coef[3 * C + c] = k2;
      coef[4 * C + c] = (float)(sdz / (double)M);
      coef[5 * C + c] = (float)(t[2] / (double)M);
    }
  }
}

// out[c] (+)= sum_g part[g][k][c] for part [G][2][C] (bias gradient from the fused ReLU post-op)
template <int NWV>
__global__ __launch_bounds__(NWV > 4 ? 64 * NWV : 256) void colsum_rows_kernel(const float* part, int C, int G, int k, float* out,
                                                          int accumulate) {
  __shared__ double sc[NWV];
  const int c = NWV == 1 ? (int)blockIdx.x * 4 + (threadIdx.x >> 6) : (int)blockIdx.x;
  if (NWV == 1 && c >= C) return;
  const float prev = accumulate ? out[c] : 0.f;
  double t[1];
  if (G > 0) {
    fin_row_sums<NWV, 1>(part, 2L * C, C, c, G, 1, k, t, sc);
  } else {
    t[0] = 0.0;
  }
  if ((NWV == 1 ? (threadIdx.x & 63) : threadIdx.x) == 0) out[c] = accumulate ? prev + (float)t[0] : (float)t[0];
}

// out[c] (+)= sum_g part[c][g]   (fp64 accumulation, fixed order)
__global__ void colsum_finalize_kernel(const float* part, int C, int G, float* out, int accumulate) {
  __shared__ double sc[16];
  const int c = blockIdx.x;
  double acc = 0.0;
  for (int g = threadIdx.x; g < G; g += blockDim.x) acc += part[(long)c * G + g];
  acc = block_sum(acc, sc);
  if (threadIdx.x == 0) out[c] = accumulate ? out[c] + (float)acc : (float)acc;
}

// Row partials [G][nq][C] -> [ceil(G/R)][nq][C], R consecutive rows merged (ahead of a finalize when G
// is large: the one-channel-per-block finalize then reads strided rows on only C blocks).  CHAN: the
// rows are (sum, M2 about the row's mean) of `tile` pixels each (the last min(tile, M - g*tile)),
// merged by Chan's formula in fp64; otherwise plain fp64 sums per quantity.  One wave per output row
// and 64 channels, all R x nq loads issued before the adds (clamped, masked after).
template <bool CHAN, int NQ, int R>
__global__ __launch_bounds__(256) void fin_merge_rows_kernel(const float* part, int C, int G, long M, int tile, int nq,
                                                             float* out, int G2) {
  const int g2 = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int c = (int)blockIdx.y * 64 + (threadIdx.x & 63);
  if (g2 >= G2) return;
  const int cc = min(c, C - 1);
  float v[R][NQ];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int g = min(g2 * R + r, G - 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[r][q] = part[((long)g * nq + min(q, nq - 1)) * C + cc];
  }
  if (c >= C) return;
  if constexpr (CHAN) {
    double n = 0.0, s = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long g = (long)g2 * R + r;
      if (g < G) {
        n += (double)min((long)tile, M - g * tile);
        s += (double)v[r][0];
      }
    }
    const double mean = s / n;
    double m2 = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long g = (long)g2 * R + r;
      if (g < G) {
        const double cnt = (double)min((long)tile, M - g * tile);
        const double d = (double)v[r][0] / cnt - mean;
        m2 += (double)v[r][1] + cnt * d * d;
      }
    }
    out[(long)g2 * 2 * C + c] = (float)s;
    out[(long)g2 * 2 * C + C + c] = (float)m2;
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q >= nq) break;
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) t += g2 * R + r < G ? (double)v[r][q] : 0.0;
      out[((long)g2 * nq + q) * C + c] = (float)t;
    }
  }
}

// How the BN backward gets the mask of the ReLU behind it (the MASK of the kernels above): the stored
// activation A (lda > 0) or the packed bytes bn_apply_mask wrote (A with lda == 0), else recomputed from
// the (msc, msh) coefficients, else none.
int bn_relu_mask_mode(const void* A, int lda, const float* msc) { return A ? (lda == 0 ? 3 : 1) : (msc ? 2 : 0); }

// f(MASK, Y2) with the mask mode and the presence of the second branch as compile-time constants:
// the one (mask, Y2) dispatch of the reduce and the apply pass.  False when the mode is none of 0 .. 3.
template <typename F>
bool bn_bwd_dispatch(int mask, bool y2, F&& f) {
  return with_const<0, 1, 2, 3>(mask, [&](auto mk) { with_const<0, 1>(y2, [&](auto b) { f(mk, b); }); });
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_bn_finalize(const float* part, int C, int G, long M, int tile, const float* gamma,
                                    const float* beta, float* rmean, float* rvar, long long* nbt, float momentum,
                                    float eps, float* mean, float* invstd, float* scale, float* shift, void* stream) {
  US_CHECK_ARG(part && gamma && beta && mean && invstd && scale && shift && M > 0, "bn_finalize: bad args");
  US_CHECK_ARG(C > 0 && G > 0 && tile > 0, "bn_finalize: bad sizes");
  FIN_LAUNCH(bn_finalize_kernel, C, G, stream, part, C, G, M, tile, gamma, beta, rmean, rvar, nbt, momentum, eps, mean,
             invstd, scale, shift);
  US_LAUNCH_CHECK("bn_finalize");
  return 0;
}

UNETSEG_API int unetseg_bn_fold(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                float eps, const float* conv_bias, float* kscale, float* bias, void* stream) {
  US_CHECK_ARG(C > 0 && gamma && beta && rmean && rvar && kscale && bias, "bn_fold: bad args");
  hipLaunchKernelGGL(bn_fold_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, C, gamma, beta, rmean,
                     rvar, eps, conv_bias, kscale, bias);
  US_LAUNCH_CHECK("bn_fold");
  return 0;
}

UNETSEG_API int unetseg_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* rmean,
                                       const float* rvar, float eps, float* scale, float* shift, void* stream) {
  hipLaunchKernelGGL(bn_eval_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, C, gamma, beta, rmean,
                     rvar, eps, scale, shift);
  US_LAUNCH_CHECK("bn_eval");
  return 0;
}

UNETSEG_API int unetseg_bn_apply(int dtype, const void* y, int ldy, const float* sc, const float* sh, const void* r,
                                 int ldr, const float* sc2, const float* sh2, int res_mode, int relu, void* out,
                                 int ldo, long M, int C, void* stream) {
  CHECK_VEC(dtype, C, "bn_apply");
  US_CHECK_ARG(y && sc && sh && out && M >= 0, "bn_apply: null pointer or negative M");
  US_CHECK_ARG(res_mode >= 0 && res_mode <= 2, "bn_apply: res_mode %d (0 none, 1 identity, 2 BN'd residual)", res_mode);
  US_CHECK_ARG(res_mode == 0 || r, "bn_apply: res_mode %d needs the residual", res_mode);
  US_CHECK_ARG(res_mode != 2 || (sc2 && sh2), "bn_apply: res_mode 2 needs the residual's BN coefficients");
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(M * C / VE<T>)), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)y, ldy, sc, sh, (const T*)r, ldr, sc2, sh2,
                                       res_mode, relu, (T*)out, ldo, M, C, nullptr));
  US_LAUNCH_CHECK("bn_apply");
  return 0;
}

UNETSEG_API int unetseg_bn_apply_mask(int dtype, const void* y, int ldy, const float* sc, const float* sh,
                                      const void* r, int ldr, const float* sc2, const float* sh2, int res_mode,
                                      void* out, int ldo, long M, int C, uint8_t* mbits, void* stream) {
  CHECK_VEC(dtype, C, "bn_apply_mask");
  US_CHECK_ARG(mbits != nullptr, "bn_apply_mask: mbits required");
  DISPATCH_T(dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for(M * C / VE<T>)), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)y, ldy, sc, sh, (const T*)r, ldr, sc2, sh2,
                                       res_mode, 1, (T*)out, ldo, M, C, mbits));
  US_LAUNCH_CHECK("bn_apply_mask");
  return 0;
}

// pixel-tile geometry of the per-channel kernels: ~target blocks over (pixel tiles x channel
// groups), at least 2 unrolled groups of rows per thread
static int tile_geom(int dtype, long M, int C, long target, int* tv_out, int* ppb_out) {
  const int V = vec_elems(dtype);
  if (C <= 0 || C % V != 0 || M < 0) {  // no 16-B channel vectors: no reduction geometry (host ASan driver)
    unetseg_set_error("reduce_tiles: C=%d must be a positive multiple of %d", C, V);
    return -1;
  }
  const int cv = C / V;
  const int tv = pow2_le(cv, 64);
  const int rows = 256 / tv;
  const int groups = cv / tv;
  target /= groups;
  if (target < 64) target = 64;
  long per = (M + rows * target - 1) / (rows * target);
  per = (per + RU - 1) / RU * RU;
  if (per < 2 * RU) per = 2 * RU;
  if (per > 256) per = 256;
  const int ppb = rows * (int)per;
  if (tv_out) *tv_out = tv;
  if (ppb_out) *ppb_out = ppb;
  return ceil_div(M, ppb);
}

// a block-count knob, read at every call (tests change it inside one process)
static long env_target(const char* name, long dflt) {
  const char* te = getenv(name);
  return te ? atol(te) : dflt;
}

// geometry of the channel-reduction kernels (also used by the host to size partial buffers).
// ~1024 blocks: against 2048, the BN-backward reductions at the unet_resnet50 B=16 shapes took
// 39.0 -> 30.5 us (65536 x 512), 63.5 -> 58.5 (1M x 64 packed mask), the finalize reads half the
// partials (tools/gpu_elem_geom.sh).  UNETSEG_RED_TARGET (tests; read at every call): another block
// count, i.e. another summation order of the same partials
UNETSEG_API int unetseg_reduce_tiles(int dtype, long M, int C, int* tv_out, int* ppb_out) {
  return tile_geom(dtype, M, C, env_target("UNETSEG_RED_TARGET", 1024), tv_out, ppb_out);
}

// the BN-backward apply pass has no partials, so it takes its own block count: ~4096 blocks
// (262144 x 256: 78.4 -> 72.3 us against 2048; 1024 gave 84.5).  UNETSEG_APPLY_TARGET: read at every call
static int apply_tiles(int dtype, long M, int C, int* tv_out, int* ppb_out) {
  return tile_geom(dtype, M, C, env_target("UNETSEG_APPLY_TARGET", 4096), tv_out, ppb_out);
}

UNETSEG_API int unetseg_bn_bwd_reduce(int dtype, const void* dA, int ldd, const void* A, int lda, const float* msc,
                                      const float* msh, const void* y1, int ld1, const float* mean1,
                                      const float* inv1, const void* y2, int ld2, const float* mean2,
                                      const float* inv2, long M, int C, float* part, int G, void* stream) {
  CHECK_VEC(dtype, C, "bn_bwd_reduce");
  US_CHECK_ARG(dA && y1 && mean1 && inv1 && part && M >= 0, "bn_bwd_reduce: null pointer or negative M");
  int tv, ppb;
  const int g = unetseg_reduce_tiles(dtype, M, C, &tv, &ppb);
  US_CHECK_ARG(g == G, "bn_bwd_reduce: G mismatch (%d vs %d)", G, g);
  const dim3 grid(G, C / vec_elems(dtype) / tv);
  hipStream_t st = (hipStream_t)stream;
  bool launched = false;
  DISPATCH_T(dtype, launched = bn_bwd_dispatch(bn_relu_mask_mode(A, lda, msc), y2 != nullptr, [&](auto mk, auto b2) {
    constexpr int MK = decltype(mk)::value;
    constexpr bool Y2 = decltype(b2)::value != 0;
    // one branch with the packed mask: the variant with the register budget (see bn_bwd_reduce_bits_kernel)
    if constexpr (MK == 3 && !Y2)
      hipLaunchKernelGGL((bn_bwd_reduce_bits_kernel<T>), grid, dim3(256), 0, st, (const T*)dA, ldd, (const T*)A, lda,
                         msc, msh, (const T*)y1, ld1, mean1, inv1, (const T*)y2, ld2, mean2, inv2, M, C, tv, ppb, part,
                         G);
    else
      hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, MK, Y2>), grid, dim3(256), 0, st, (const T*)dA, ldd, (const T*)A,
                         lda, msc, msh, (const T*)y1, ld1, mean1, inv1, (const T*)y2, ld2, mean2, inv2, M, C, tv, ppb,
                         part, G);
  }));
  US_CHECK_ARG(launched, "bn_bwd_reduce: no kernel for this mask mode");
  US_LAUNCH_CHECK("bn_bwd_reduce");
  return 0;
}

UNETSEG_API int unetseg_bn_bwd_finalize(const float* part, int C, int G, long M, int nbranch, const float* g1,
                                        const float* inv1, float* dg1, float* db1, const float* g2, const float* inv2,
                                        float* dg2, float* db2, float* coef, void* stream) {
  US_CHECK_ARG(nbranch == 1 || nbranch == 2, "bn_bwd_finalize: nbranch %d must be 1 or 2", nbranch);
  US_CHECK_ARG(part && g1 && inv1 && coef && C > 0 && G > 0 && M > 0, "bn_bwd_finalize: bad args");
  US_CHECK_ARG(nbranch == 1 || (g2 && inv2), "bn_bwd_finalize: the second branch needs its gamma / invstd");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, part, C, G, M, nbranch, g1,
                     inv1, dg1, db1, g2, inv2, dg2, db2, coef);
  US_LAUNCH_CHECK("bn_bwd_finalize");
  return 0;
}

UNETSEG_API int unetseg_bn_bwd_apply(int dtype, const void* dA, int ldd, const void* A, int lda, const float* msc,
                                     const float* msh, const void* y1, int ld1, const float* mean1, const float* inv1,
                                     void* dy1, int ldo1,
                                     const void* y2, int ld2, const float* mean2, const float* inv2, void* dy2,
                                     int ldo2, const float* coef, void* dzout, int ldz, int dz_acc, long M, int C,
                                     void* stream) {
  CHECK_VEC(dtype, C, "bn_bwd_apply");
  int tv, ppb;
  const int G = apply_tiles(dtype, M, C, &tv, &ppb);
  const dim3 grid(G, C / vec_elems(dtype) / tv);
  const int dzm = dzout ? (dz_acc ? 2 : 1) : 0;
  hipStream_t st = (hipStream_t)stream;
  bool launched = false;
  DISPATCH_T(dtype, bn_bwd_dispatch(bn_relu_mask_mode(A, lda, msc), y2 != nullptr, [&](auto mk, auto b2) {
    launched = with_const<0, 1, 2>(dzm, [&](auto dz) {
      hipLaunchKernelGGL((bn_bwd_apply_kernel<T, decltype(mk)::value, decltype(b2)::value != 0, decltype(dz)::value>),
                         grid, dim3(256), 0, st, (const T*)dA, ldd, (const T*)A, lda, msc, msh, (const T*)y1, ld1,
                         mean1, inv1, (T*)dy1, ldo1, (const T*)y2, ld2, mean2, inv2, (T*)dy2, ldo2, coef, (T*)dzout,
                         ldz, M, C, tv, ppb);
    });
  }));
  US_CHECK_ARG(launched, "bn_bwd_apply: no kernel for this mask / dz mode");
  US_LAUNCH_CHECK("bn_bwd_apply");
  return 0;
}

UNETSEG_API int unetseg_relu_bwd_bias(int dtype, const void* dA, int ldd, const void* A, int lda, void* dY, int ldy,
                                      long M, int C, float* part, int G, void* stream) {
  CHECK_VEC(dtype, C, "relu_bwd_bias");
  int tv, ppb;
  const int g = unetseg_reduce_tiles(dtype, M, C, &tv, &ppb);
  US_CHECK_ARG(g == G, "relu_bwd_bias: G mismatch");
  const dim3 grid(G, C / vec_elems(dtype) / tv);
  DISPATCH_T(dtype, hipLaunchKernelGGL(relu_bwd_bias_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream,
                                       (const T*)dA, ldd, (const T*)A, lda, (T*)dY, ldy, M, C, tv, ppb, part, G));
  US_LAUNCH_CHECK("relu_bwd_bias");
  return 0;
}

constexpr int kFinMergeR = 16;
UNETSEG_API int unetseg_fin_merge_rows(const float* part, int C, int G, long M, int tile, int nq, float* out,
                                       void* stream) {
  US_CHECK_ARG(part && out && C > 0 && G > 0 && nq >= 1 && nq <= 3, "fin_merge_rows: bad args");
  US_CHECK_ARG(tile == 0 || (nq == 2 && M > 0), "fin_merge_rows: a statistics merge needs nq == 2 and M");
  const int G2 = ceil_div(G, kFinMergeR);
  const dim3 grid(ceil_div(G2, 4), ceil_div(C, 64));
  if (tile > 0)
    hipLaunchKernelGGL((fin_merge_rows_kernel<true, 2, kFinMergeR>), grid, dim3(256), 0, (hipStream_t)stream, part, C,
                       G, M, tile, nq, out, G2);
  else if (nq == 3)
    hipLaunchKernelGGL((fin_merge_rows_kernel<false, 3, kFinMergeR>), grid, dim3(256), 0, (hipStream_t)stream, part,
                       C, G, M, tile, nq, out, G2);
  else
    hipLaunchKernelGGL((fin_merge_rows_kernel<false, 2, kFinMergeR>), grid, dim3(256), 0, (hipStream_t)stream, part,
                       C, G, M, tile, nq, out, G2);
  US_LAUNCH_CHECK("fin_merge_rows");
  return 0;
}

UNETSEG_API int unetseg_bn_bwd_finalize_rows(const float* part, int C, int G, long M, const float* g1,
                                             const float* inv1, float* dg1, float* db1, float* coef, void* stream) {
  US_CHECK_ARG(part && g1 && inv1 && dg1 && db1 && coef && M > 0, "bn_bwd_finalize_rows: bad args");
  US_CHECK_ARG(C > 0 && G > 0, "bn_bwd_finalize_rows: bad sizes");
  FIN_LAUNCH(bn_bwd_finalize_rows_kernel, C, G, stream, part, C, G, M, g1, inv1, dg1, db1, coef);
  US_LAUNCH_CHECK("bn_bwd_finalize_rows");
  return 0;
}

UNETSEG_API int unetseg_bn_bwd_finalize_rows_res(const float* part, int C, int G, long M, int nbranch, const float* g1,
                                                 const float* inv1, float* dg1, float* db1, const float* g2,
                                                 const float* inv2, float* dg2, float* db2, float* coef, void* stream) {
  US_CHECK_ARG(part && g1 && inv1 && dg1 && db1 && coef && M > 0 && C > 0 && G > 0 && (nbranch == 1 || nbranch == 2),
               "bn_bwd_finalize_rows_res: bad args");
  US_CHECK_ARG(nbranch == 1 || (g2 && inv2 && dg2 && db2), "bn_bwd_finalize_rows_res: branch 2 needs its pointers");
  FIN_LAUNCH(bn_bwd_finalize_rows_res_kernel, C, G, stream, part, C, G, M, nbranch, g1, inv1, dg1, db1, g2, inv2, dg2,
             db2, coef);
  US_LAUNCH_CHECK("bn_bwd_finalize_rows_res");
  return 0;
}

UNETSEG_API int unetseg_colsum_rows(const float* part, int C, int G, int k, float* out, int accumulate, void* stream) {
  US_CHECK_ARG(part && out && C > 0 && G >= 0 && (k == 0 || k == 1), "colsum_rows: bad args");
  FIN_LAUNCH(colsum_rows_kernel, C, G, stream, part, C, G, k, out, accumulate);
  US_LAUNCH_CHECK("colsum_rows");
  return 0;
}

UNETSEG_API int unetseg_colsum_finalize(const float* part, int C, int G, float* out, int accumulate, void* stream) {
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, part, C, G, out, accumulate);
  US_LAUNCH_CHECK("colsum_finalize");
  return 0;
}
