// Per-pixel NHWC kernels of the U-Net hot path: input packing, the 1x1 convs with few outputs (the
// two-class heads and the attention psi conv, and their C-way generalisation), the attention gate
// and the residual add.  Layout and element types as bn.hip.
//
// Reference ops replaced:
//   final / seg_head / psi 1x1   model/unet_resnet.py:78  model/unet_plain.py:69  model/unet_attention.py:25
//   outc / final 1x1 (C > 2)     model/unet_resnet.py:78, model/unet_plain.py:69, model/unet_dualdense.py:88
//   AttentionGate                model/unet_attention.py:30-35
//   residual add                 model/resnet_backbone.py:95,100,110,113
#include "elem_util.h"

namespace {

// NCHW fp32 [N][3][H][W] -> NHWC T [N][H][W][Cpad] (zero padded)
template <typename T>
__global__ void pack_input_kernel(const float* x, int N, int C, int H, int W, int Cpad, T* y) {
  const long total = (long)N * H * W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long n = i / ((long)H * W), hw = i - n * H * W;
    T* o = y + i * Cpad;
    for (int c = 0; c < Cpad; ++c) o[c] = (T)(c < C ? x[(n * C + c) * (long)H * W + hw] : 0.f);
  }
}

// ------------------------------------------------------------------------------------------
// 1x1 conv with tiny Cout (final 64->2, seg_head 64->1, attention psi inter->1).
// Forward: one wave per 64/ (C/V) pixels; output fp32 planar [N][K][HW] (== [M] for K=1);
// optional BN partial stats of channel 0 per block (for psi: [G][2][1], tile = pixels/block).
// ------------------------------------------------------------------------------------------
template <typename T, int K>
__global__ void pw_small_fwd_kernel(const T* x, int ldx, long M, int HW, int C, const float* w, const float* b,
                                    float* y, float* stats, int pix_per_block) {
  constexpr int V = VE<T>;
  __shared__ double sred[16];
  const int cv = C / V;  // lanes per pixel (C/V <= 64, power of two)
  const int ppw = 64 / cv;  // pixels per wave pass
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int sub = lane / cv, v = lane % cv;
  const int ppb = pix_per_block < 0 ? -pix_per_block : pix_per_block;
  const long p0 = (long)blockIdx.x * ppb;
  const long p1 = min(M, p0 + ppb);
  float wv[K][V];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) wv[k][e] = w[k * C + v * V + e];
  double lsum = 0.0;
  if (cv == 8 && !stats && pix_per_block > 0) {
    // 8 lanes per pixel: four pixel groups per iteration (four 16-B loads in flight per lane),
    // 8-lane sums by DPP (xor 1, xor 2 within quads, then row_half_mirror: lane 0 of each 8-lane
    // group adds lane 7, i.e. the other quad's sum) instead of LDS-routed shuffles
    constexpr int U = 4;
    for (long pbase = p0 + (long)wid * 8 * U; pbase < p1; pbase += (long)nw * 8 * U) {
      float acc[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // unconditional (clamped) load: a load under the lane condition got a branch and a vmcnt(0)
        // of its own, which serialised the four groups; past-the-end pixels are never stored
        const long pc = min(pbase + u * 8 + sub, p1 - 1);
        float xv[V];
        load_vec(x + pc * ldx + v * V, xv);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          float a0 = 0.f;
#pragma unroll
          for (int e = 0; e < V; ++e) a0 += xv[e] * wv[k][e];
          acc[u][k] = a0;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) {
          float t = acc[u][k];
          t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0xB1, 0xF, 0xF, false));
          t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0x4E, 0xF, 0xF, false));
          t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0x141, 0xF, 0xF, false));
          acc[u][k] = t;
        }
      if (v == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long p = pbase + u * 8 + sub;
          if (p < p1) {
            const long n = p / HW, hw = p - n * HW;
#pragma unroll
            for (int k = 0; k < K; ++k) y[(n * K + k) * HW + hw] = acc[u][k] + (b ? b[k] : 0.f);
          }
        }
      }
    }
    return;
  }
  // pass 1: outputs.  Four wave passes per iteration with their loads issued first at clamped (valid)
  // pixels: the one load under `p < p1` got a branch and a vmcnt(0) of its own, one exposed round trip
  // per pass (the attention psi conv at 8 x 512^2: 57 us for 142 MB).  The dot products are spelled out
  // as the one-pass loop compiled them -- rounded products (v_pk_mul_f32), then adds in channel order --
  // so the outputs stay bit-identical whatever the unrolled code would have been contracted to
  // (the bias is loaded once up front: read under the store's lane condition it was another branch
  // with a vmcnt(0) behind it)
  constexpr int U = 4;
  const long wstep = (long)nw * ppw;
  float bk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) bk[k] = b ? b[k] : 0.f;
  for (long pbase = p0 + (long)wid * ppw; pbase < p1; pbase += U * wstep) {
    uint4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long pc = min(pbase + u * wstep + sub, p1 - 1);
      raw[u] = *reinterpret_cast<const uint4*>(x + pc * ldx + v * V);
    }
    // keep the four loads together: the scheduler otherwise started unpacking the first one before the
    // others were issued (a vmcnt(0) right behind it)
    __builtin_amdgcn_sched_barrier(0);
    float xv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) cvt16<T>(raw[u], xv[u]);
    float acc[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma clang fp contract(off)
        acc[u][k] = 0.f;
#pragma unroll
        for (int e = 0; e < V; ++e) acc[u][k] += xv[u][e] * wv[k][e];
      }
    for (int o = 1; o < cv; o <<= 1)
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[u][k] += __shfl_xor(acc[u][k], o, 64);
    if (v == 0)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long p = pbase + u * wstep + sub;
        if (p < p1) {
          const long n = p / HW, hw = p - n * HW;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const float val = acc[u][k] + bk[k];
            y[(n * K + k) * HW + hw] = val;
            if (k == 0) lsum += val;
          }
        }
      }
  }
  if (!stats) return;
  const double tot = block_sum(lsum, sred);
  const long cnt = p1 - p0;
  const double mean = tot / (double)cnt;
  __syncthreads();
  double lm2 = 0.0;
  for (long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
    const long n = p / HW, hw = p - n * HW;
    const double d = (double)y[(n * K) * HW + hw] - mean;
    lm2 += d * d;
  }
  const double m2 = block_sum(lm2, sred);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = (float)tot;  // [G][2][1]
    stats[2 * blockIdx.x + 1] = (float)m2;
  }
}

// Backward of the tiny-Cout 1x1 conv.  dy fp32 planar [N][K][HW].
//   dx (+)= dy . W  (T, NHWC, ld), partials for dW [K][C][G] and db [K][G]
// MASK: x is the output of a ReLU whose backward is fused here (this conv is x's sole consumer):
// dx = (x > 0) ? dy . W : 0, and part_d[G][2][C] (slot 0) gets the column sums of the stored
// (rounded) dx -- the producer conv's bias-gradient partials, as the TN dgrad post-op writes them.
template <typename T, int K, bool MASK = false>
__global__ void pw_small_bwd_kernel(const float* dy, const T* x, int ldx, long M, int HW, int C, const float* w,
                                    T* dx, int lddx, int dx_acc, float* part_w, float* part_b, int G,
                                    int pix_per_block, float* part_d = nullptr) {
  constexpr int V = VE<T>;
  __shared__ float red[256][V];
  __shared__ float redb[256];
  const int cv = C / V;
  const int tv = cv, rows = blockDim.x / tv;
  const int tx = threadIdx.x % tv, ty = threadIdx.x / tv;
  const int c0 = tx * V;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  float wv[K][V];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) wv[k][e] = w[k * C + c0 + e];
  float sw[K][V], sb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    sb[k] = 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) sw[k][e] = 0.f;
  }
  float sd[V];
#pragma unroll
  for (int e = 0; e < V; ++e) sd[e] = 0.f;
  for (long p = p0 + ty; p < p1; p += rows) {
    const long n = p / HW, hw = p - n * HW;
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = dy[(n * K + k) * HW + hw];
    float xv[V], o[V];
    load_vec(x + p * ldx + c0, xv);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      // explicit product then fma (no contraction choice left to the compiler)
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        s = k == 0 ? g[0] * wv[0][e] : fmaf(g[k], wv[k][e], s);
        sw[k][e] += g[k] * xv[e];
      }
      o[e] = s;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sb[k] += g[k];
    if (MASK) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        o[e] = xv[e] > 0.f ? (float)(T)o[e] : 0.f;  // the stored value, rounded
        sd[e] += o[e];
      }
    }
    if (dx) {
      T* dp = dx + p * lddx + c0;
      if (dx_acc) {
        float old[V];
        load_vec(dp, old);
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] += old[e];
      }
      store_vec(dp, o);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < V; ++e) red[threadIdx.x][e] = sw[k][e];
    redb[threadIdx.x] = sb[k];
    __syncthreads();
    if (ty == 0) {
      float s[V];
      float bs = 0.f;
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] = 0.f;
      for (int r = 0; r < rows; ++r) {
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += red[r * tv + tx][e];
        bs += redb[r * tv + tx];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) part_w[((long)k * C + c0 + e) * G + blockIdx.x] = s[e];
      if (tx == 0) part_b[(long)k * G + blockIdx.x] = bs;
    }
  }
  if (MASK) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < V; ++e) red[threadIdx.x][e] = sd[e];
    __syncthreads();
    if (ty == 0) {
      float s[V];
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] = 0.f;
      for (int r = 0; r < rows; ++r)
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += red[r * tv + tx][e];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        part_d[(long)blockIdx.x * 2 * C + c0 + e] = s[e];
        part_d[(long)blockIdx.x * 2 * C + C + c0 + e] = 0.f;
      }
    }
  }
}

constexpr int kHeadTile = 256;

// ------------------------------------------------------------------------------------------
// 1x1 head with K in (2, 32] outputs: y[n][k][hw] = sum_c x[p][c] w[k][c] + b[k] (fp32 out).
// Thread per pixel, weights in LDS (broadcast reads), K accumulators in registers.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pw_head_fwd_kernel(const T* x, int ldx, long M, int HW, int C, int K,
                                                          const float* w, const float* b, float* y) {
  extern __shared__ float sw[];  // [K][C]
  for (int i = threadIdx.x; i < K * C; i += blockDim.x) sw[i] = w[i];
  __syncthreads();
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= M) return;
  float acc[kMaxC];
#pragma unroll
  for (int k = 0; k < kMaxC; ++k) acc[k] = 0.f;
  constexpr int V = 16 / sizeof(T);
  for (int c0 = 0; c0 < C; c0 += V) {
    float xv[V];
    load_vec(x + p * ldx + c0, xv);
#pragma unroll
    for (int k = 0; k < kMaxC; ++k) {
      if (k < K) {
        float s = acc[k];
#pragma unroll
        for (int e = 0; e < V; ++e) s += xv[e] * sw[k * C + c0 + e];
        acc[k] = s;
      }
    }
  }
  const long n = p / HW, hw = p - n * HW;
#pragma unroll
  for (int k = 0; k < kMaxC; ++k)
    if (k < K) y[(n * K + k) * HW + hw] = acc[k] + (b ? b[k] : 0.f);
}

// Backward: dx (+)= dy . W (NHWC, T), dW / db partials part_w [K][C][G], part_b [K][G] over pixel
// tiles of ppb pixels.  Thread (tx = channel, ty = pixel row); dy in planar fp32.
template <typename T>
__global__ __launch_bounds__(256) void pw_head_bwd_kernel(const float* dy, const T* x, int ldx, long M, int HW, int C,
                                                          int K, const float* w, T* dx, int lddx, int dx_acc,
                                                          float* part_w, float* part_b, int G, int ppb) {
  extern __shared__ float sm[];  // [K][C] weights, then [256] reduction scratch
  float* swt = sm;
  float* red = sm + K * C;
  for (int i = threadIdx.x; i < K * C; i += blockDim.x) swt[i] = w[i];
  __syncthreads();
  const int rows = blockDim.x / C;  // C divides 256 (host check)
  const int tx = threadIdx.x % C, ty = threadIdx.x / C;
  const long p0 = (long)blockIdx.x * ppb, p1 = min(M, p0 + ppb);
  float sw[kMaxC], sb[kMaxC];
#pragma unroll
  for (int k = 0; k < kMaxC; ++k) sw[k] = sb[k] = 0.f;
  for (long p = p0 + ty; p < p1; p += rows) {
    const long n = p / HW, hw = p - n * HW;
    const float xv = (float)x[p * ldx + tx];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxC; ++k) {
      if (k < K) {
        const float g = dy[(n * K + k) * HW + hw];
        s += g * swt[k * C + tx];
        sw[k] += g * xv;
        sb[k] += g;
      }
    }
    if (dx) {
      T* dp = dx + p * lddx + tx;
      *dp = (T)(dx_acc ? s + (float)*dp : s);
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxC; ++k) {
    if (k < K) {  // uniform
      __syncthreads();
      red[threadIdx.x] = sw[k];
      __syncthreads();
      if (ty == 0) {
        float t = 0.f;
        for (int r = 0; r < rows; ++r) t += red[r * C + tx];
        part_w[((long)k * C + tx) * G + blockIdx.x] = t;
      }
      __syncthreads();
      red[threadIdx.x] = sb[k];
      __syncthreads();
      if (threadIdx.x == 0) {
        float t = 0.f;
        for (int r = 0; r < rows; ++r) t += red[r * C];  // column 0 threads carry the full sum
        part_b[(long)k * G + blockIdx.x] = t;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Attention gate (model/unet_attention.py:30-35):
//   alpha = sigmoid(psi*sc + sh) (per pixel), gated = skip * alpha
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void attn_apply_kernel(const T* skip, int lds_, const float* psi, const float* sc, const float* sh,
                                  float* alpha, T* gated, int ldg, long M, int C) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const long total = M * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long p = i / cv;
    const int c0 = (int)(i - p * cv) * V;
    const float z = psi[p] * sc[0] + sh[0];
    const float al = 1.f / (1.f + expf(-z));
    if (c0 == 0) alpha[p] = al;
    float v[V];
    load_vec(skip + p * lds_ + c0, v);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] *= al;
    store_vec(gated + p * ldg + c0, v);
  }
}

// backward 1: d_skip (+)= dg * alpha ; dpsibn[p] = (sum_c dg*skip) * alpha*(1-alpha);
// partials [2][1][G]: sum dpsibn, sum dpsibn * xhat(psi).  ACC: d_skip accumulates onto its buffer
template <typename T, bool ACC>
__global__ void attn_bwd1_kernel(const T* dg, int ldg, const T* skip, int lds_, const float* alpha, const float* psi,
                                 const float* mean, const float* inv, T* dskip, int ldds, float* dpsibn,
                                 long M, int C, int pix_per_block, float* part, int G) {
  constexpr int V = VE<T>;
  __shared__ double sred[16];
  const int cvt = C / V;                 // vectors per pixel
  const int cv = cvt < 64 ? cvt : 64;    // lanes per pixel (power of two)
  const int nchunk = cvt / cv;
  const int ppw = 64 / cv;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int sub = lane / cv, v = lane % cv;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  const float mu = mean[0], iv = inv[0];
  double s0 = 0.0, s1 = 0.0;
  if (nchunk == 1) {
    // one vector per lane per pixel, four pixel groups per wave in flight.  Every load of the four
    // groups is unconditional (a pixel past the block's end re-reads its last one; only the stores are
    // masked) and the lane reductions of the four run interleaved: a load under a lane condition got
    // its own branch and a vmcnt(0) behind it, which serialised the groups
    constexpr int U = 4;
    const int c0 = v * V;
    const long step = (long)nw * ppw;
    for (long pb = p0 + (long)wid * ppw; pb < p1; pb += U * step) {
      float g[U][V], sk[U][V], old[U][V], al[U], ps[U], dot[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long pc = min(pb + u * step + sub, p1 - 1);
        al[u] = alpha[pc];
        ps[u] = psi[pc];
        load_vec(dg + pc * ldg + c0, g[u]);
        load_vec(skip + pc * lds_ + c0, sk[u]);
        if (ACC) load_vec(dskip + pc * ldds + c0, old[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long p = pb + u * step + sub;
        float o[V];
        dot[u] = 0.f;
#pragma unroll
        for (int e = 0; e < V; ++e) {
          dot[u] += g[u][e] * sk[u][e];
          o[e] = ACC ? g[u][e] * al[u] + old[u][e] : g[u][e] * al[u] + 0.f;
        }
        if (p < p1) store_vec(dskip + p * ldds + c0, o);
      }
#pragma unroll
      for (int sh = 1; sh < 64; sh <<= 1)
        if (sh < cv)
#pragma unroll
          for (int u = 0; u < U; ++u) dot[u] += __shfl_xor(dot[u], sh, 64);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long p = pb + u * step + sub;
        if (p < p1 && v == 0) {
          const float d = dot[u] * al[u] * (1.f - al[u]);
          dpsibn[p] = d;
          s0 += d;
          s1 += (double)d * (ps[u] - mu) * iv;
        }
      }
    }
  } else
  for (long pbase = p0 + (long)wid * ppw; pbase < p1; pbase += (long)nw * ppw) {
    const long p = pbase + sub;
    float dot = 0.f;
    float al = 0.f;
    if (p < p1) {
      al = alpha[p];
      for (int ch = 0; ch < nchunk; ++ch) {
        const int c0 = (ch * cv + v) * V;
        float g[V], sk[V], o[V];
        load_vec(dg + p * ldg + c0, g);
        load_vec(skip + p * lds_ + c0, sk);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          dot += g[e] * sk[e];
          o[e] = g[e] * al;
        }
        T* dp = dskip + p * ldds + c0;
        if (ACC) {
          float old[V];
          load_vec(dp, old);
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] += old[e];
        }
        store_vec(dp, o);
      }
    }
    for (int o = 1; o < cv; o <<= 1) dot += __shfl_xor(dot, o, 64);
    if (p < p1 && v == 0) {
      const float d = dot * al * (1.f - al);
      dpsibn[p] = d;
      s0 += d;
      s1 += (double)d * (psi[p] - mu) * iv;
    }
  }
  s0 = block_sum(s0, sred);
  s1 = block_sum(s1, sred);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = (float)s0;
    part[G + blockIdx.x] = (float)s1;
  }
}

// backward 2: dpsi = coef0*(dpsibn - coef1 - xhat*coef2); dz_f = dpsi * w_psi * (f > 0);
// partials: dW_psi [C][G] = sum dpsi * f, db_psi [G] = sum dpsi
template <typename T>
__global__ void attn_bwd2_kernel(const float* dpsibn, const float* psi, const float* mean, const float* inv,
                                 const float* coef, const T* f, int ldf, const float* wpsi, T* dzf, int lddz, long M,
                                 int C, int tv, int pix_per_block, float* part_w, float* part_b, int G) {
  constexpr int V = VE<T>;
  __shared__ float red[256][V];
  __shared__ float redb[256];
  const int tx = threadIdx.x % tv, ty = threadIdx.x / tv, rows = blockDim.x / tv;
  const int c0 = tx * V;
  const long p0 = (long)blockIdx.x * pix_per_block;
  const long p1 = min(M, p0 + pix_per_block);
  float wv[V], sw[V];
  float sb = 0.f;
#pragma unroll
  for (int e = 0; e < V; ++e) { wv[e] = wpsi[c0 + e]; sw[e] = 0.f; }
  const float mu = mean[0], iv = inv[0], k0 = coef[0], k1 = coef[1], k2 = coef[2];
  // the contractions spelled out (fmaf): unrolled, the compiler packed some products into
  // v_pk_mul_f32 + add, which rounds twice where the one-pixel loop's fma rounded once
  auto one = [&](long p, float ps, float db, const float (&fv)[V]) {
    const float xh = (ps - mu) * iv;
    const float dp = k0 * fmaf(-xh, k2, db - k1);
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      sw[e] = fmaf(dp, fv[e], sw[e]);
      o[e] = fv[e] > 0.f ? dp * wv[e] : 0.f;
    }
    if (tx == 0) sb += dp;
    store_vec(dzf + p * lddz + c0, o);
  };
  // four pixels per thread per round, all their loads issued first (one pixel per round left each
  // round's load latency exposed); the sums run in the same pixel order as before
  constexpr int U = 4;
  long p = p0 + ty;
  for (; p + (long)(U - 1) * rows < p1; p += (long)U * rows) {
    float ps[U], db[U], fv[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long q = p + (long)u * rows;
      ps[u] = psi[q];
      db[u] = dpsibn[q];
      load_vec(f + q * ldf + c0, fv[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) one(p + (long)u * rows, ps[u], db[u], fv[u]);
  }
  for (; p < p1; p += rows) {
    float fv[V];
    load_vec(f + p * ldf + c0, fv);
    one(p, psi[p], dpsibn[p], fv);
  }
#pragma unroll
  for (int e = 0; e < V; ++e) red[threadIdx.x][e] = sw[e];
  redb[threadIdx.x] = sb;
  __syncthreads();
  if (ty == 0) {
    float s[V];
    float bs = 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] += red[r * tv + tx][e];
      bs += redb[r * tv + tx];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) part_w[(long)(c0 + e) * G + blockIdx.x] = s[e];
    if (tx == 0) part_b[blockIdx.x] = bs;
  }
}

// elementwise add of NHWC tensors: out (+)= x
template <typename T>
__global__ void add_kernel(const T* x, int ldx, T* out, int ldo, long M, int C) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const long total = M * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long p = i / cv;
    const int c0 = (int)(i - p * cv) * V;
    float a[V], b[V];
    load_vec(x + p * ldx + c0, a);
    load_vec(out + p * ldo + c0, b);
#pragma unroll
    for (int e = 0; e < V; ++e) b[e] += a[e];
    store_vec(out + p * ldo + c0, b);
  }
}

// f(K) with the pw_small kernels' output count as a compile-time constant: K = 1, anything else runs
// the K = 2 kernels (the entry points that need it check k themselves)
template <typename F>
void pw_small_dispatch_k(int k, F&& f) {
  if (k == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}

}  // namespace

// The argument checks shared by the strided entry points below (include/unetseg_hip.h, "the pointwise
// contract").  Sizes and strides are checked first, then M == 0 returns 0 (nothing to do, no launch, no
// pointer looked at), then the required pointers.
// ld (elements between pixels) of an operand the kernel reads or writes in 16-B vectors
#define CHECK_LD_VEC(dtype, ld, c, name, what)                                                                  \
  US_CHECK_ARG((ld) >= (c) && (ld) % vec_elems(dtype) == 0,                                                     \
               "%s: %s (%d) must be at least c (%d) and a multiple of the 16-B vector", name, what, (int)(ld),  \
               (int)(c))
// M pixels in planar images of hw pixels
#define CHECK_PIXELS(M, hw, name) \
  US_CHECK_ARG((M) >= 0 && ((M) == 0 || (hw) > 0), "%s: bad pixel counts (M=%ld, hw=%d)", name, (long)(M), (int)(hw))

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_pack_input(int dtype, const float* x, int n, int c, int h, int w, int cpad, void* y,
                                   void* stream) {
  US_CHECK_DTYPE(dtype, "pack_input");
  US_CHECK_ARG(cpad >= c && c > 0 && n >= 0 && h >= 0 && w >= 0, "pack_input: bad sizes (c=%d, cpad=%d < c?)", c, cpad);
  if ((long)n * h * w == 0) return 0;
  US_CHECK_ARG(x && y, "pack_input: null pointer");
  DISPATCH_T(dtype, hipLaunchKernelGGL(pack_input_kernel<T>, dim3(grid_for((long)n * h * w)), dim3(256), 0,
                                       (hipStream_t)stream, x, n, c, h, w, cpad, (T*)y));
  US_LAUNCH_CHECK("pack_input");
  return 0;
}

// NCHW fp32 image -> width-padded stem layout bf16 [N][H][W+8][8]: image column w at packed column
// w+3, channels >= C and the 3 + 5 border columns zero (see unetseg_stem_fwd)
__global__ void pack_input_stem_kernel(const float* x, int N, int C, int H, int W, bf16* y) {
  const int WP = W + 8;
  const long total = (long)N * H * WP;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / WP;
    const int wp = (int)(i - row * WP), w = wp - 3;
    const long n = row / H, h = row - n * H;
    // all eight loads unconditional (clamped into the image; channels past C re-read channel C - 1,
    // the same cache line) and masked after: conditional loads were waited on one at a time
    const int wc = min(max(w, 0), W - 1);
    float xv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) xv[c] = x[((n * C + min(c, C - 1)) * H + h) * (long)W + wc];
    bf16 v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (bf16)((c < C && w >= 0 && w < W) ? xv[c] : 0.f);
    *reinterpret_cast<uint4*>(y + i * 8) = *reinterpret_cast<uint4*>(v);
  }
}

UNETSEG_API int unetseg_pack_input_stem(const float* x, int n, int c, int h, int w, void* y, void* stream) {
  US_CHECK_ARG(c >= 1 && c <= 8 && n >= 0 && h >= 0 && w >= 0, "pack_input_stem: bad sizes (n=%d c=%d h=%d w=%d, 1 <= c <= 8)",
               n, c, h, w);
  if ((long)n * h * w == 0) return 0;  // an empty image: nothing is written, the border columns included
  US_CHECK_ARG(x && y, "pack_input_stem: null pointer");
  hipLaunchKernelGGL(pack_input_stem_kernel, dim3(grid_for((long)n * h * (w + 8))), dim3(256), 0, (hipStream_t)stream,
                     x, n, c, h, w, (bf16*)y);
  US_LAUNCH_CHECK("pack_input_stem");
  return 0;
}

// pixel tile of the small-Cout 1x1 / attention-psi kernels: 2048, halved (down to 128) while that
// leaves fewer than 512 blocks (the 64^2 gate's 32 K pixels had 16 blocks at 2048)
static long pw_tile(long M) {
  static const bool fixed = getenv("UNETSEG_PW_TILE_FIXED") != nullptr;  // A/B: always 2048; latched on first use
  long t = 2048;
  if (fixed) return t;
  while (t > 128 && (M + t - 1) / t < 512) t >>= 1;
  return t;
}
UNETSEG_API int unetseg_pw_small_tile(long M) { return (int)pw_tile(M); }
UNETSEG_API int unetseg_pw_small_tiles(long M) { return ceil_div(M, pw_tile(M)); }

// y fp32 planar [n][k][hw]; stats (k==1 only, may be NULL): [G][2], G = unetseg_pw_small_tiles(M), tile unetseg_pw_small_tile(M) px
UNETSEG_API int unetseg_pw_small_fwd(int dtype, const void* x, int ldx, long M, int hw, int c, int k, const float* w,
                                     const float* b, float* y, float* stats, void* stream) {
  CHECK_VEC(dtype, c, "pw_small_fwd");
  const int cv = c / vec_elems(dtype);
  US_CHECK_ARG(cv <= 64 && (cv & (cv - 1)) == 0, "pw_small_fwd: C/V must be a power of two <= 64");
  US_CHECK_ARG(k == 1 || k == 2, "pw_small_fwd: k must be 1 or 2");
  US_CHECK_ARG(!stats || k == 1, "pw_small_fwd: stats only for k==1");
  CHECK_LD_VEC(dtype, ldx, c, "pw_small_fwd", "ldx");
  CHECK_PIXELS(M, hw, "pw_small_fwd");
  if (M == 0) return 0;
  US_CHECK_ARG(x && w && y, "pw_small_fwd: null pointer (x, w and y are required)");
  // without statistics the tile only sets the grid (every pixel's output is its own): 128-pixel blocks,
  // twice the resident waves of pw_tile's for the latency-bound head -- the attention U-Net's 64 -> 2
  // head at 8 x 512^2: 105.6 (2048) / 95.7 (512) / 87.7 (256) / 82.0 us (128).  UNETSEG_PW_FWD_TILE = T
  // sets it (0: pw_tile; latched on first use); the statistics' partial rows keep pw_tile, which the BN
  // finalize is sized by
  static const long nostat_tile = getenv("UNETSEG_PW_FWD_TILE") ? atol(getenv("UNETSEG_PW_FWD_TILE")) : 128;
  const long tile = (!stats && nostat_tile > 0) ? nostat_tile : pw_tile(M);
  const int G = (int)ceil_div(M, tile);
  hipStream_t st = (hipStream_t)stream;
  static const int pw_sign = getenv("UNETSEG_PW_GENERIC") ? -1 : 1;  // A/B: generic shuffle path; latched on first use
  DISPATCH_T(dtype, pw_small_dispatch_k(k, [&](auto kc) {
    hipLaunchKernelGGL((pw_small_fwd_kernel<T, decltype(kc)::value>), dim3(G), dim3(256), 0, st, (const T*)x, ldx, M,
                       hw, c, w, b, y, stats, (int)tile * pw_sign);
  }));
  US_LAUNCH_CHECK("pw_small_fwd");
  return 0;
}

// dx (may be NULL) (+)= dy . W ; part_w [k][c][G], part_b [k][G]  (G = unetseg_pw_small_tiles(M))
UNETSEG_API int unetseg_pw_small_bwd(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c, int k,
                                     const float* w, void* dx, int lddx, int dx_acc, float* part_w, float* part_b,
                                     void* stream) {
  CHECK_VEC(dtype, c, "pw_small_bwd");
  const int cv = c / vec_elems(dtype);
  US_CHECK_ARG(cv <= 256 && 256 % cv == 0, "pw_small_bwd: bad C");
  US_CHECK_ARG(k == 1 || k == 2, "pw_small_bwd: k must be 1 or 2");
  CHECK_LD_VEC(dtype, ldx, c, "pw_small_bwd", "ldx");
  if (dx) CHECK_LD_VEC(dtype, lddx, c, "pw_small_bwd", "lddx");
  CHECK_PIXELS(M, hw, "pw_small_bwd");
  if (M == 0) return 0;
  US_CHECK_ARG(dy && x && w && part_w && part_b, "pw_small_bwd: null pointer (only dx may be NULL)");
  const int G = unetseg_pw_small_tiles(M);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, pw_small_dispatch_k(k, [&](auto kc) {
    hipLaunchKernelGGL((pw_small_bwd_kernel<T, decltype(kc)::value>), dim3(G), dim3(256), 0, st, dy, (const T*)x, ldx,
                       M, hw, c, w, (T*)dx, lddx, dx_acc, part_w, part_b, G, (int)pw_tile(M));
  }));
  US_LAUNCH_CHECK("pw_small_bwd");
  return 0;
}

// pw_small_bwd with the backward of the ReLU that produced x fused in (x = that ReLU's output, this
// conv its sole consumer): dx = (x > 0) ? dy . W : 0 (no accumulate), part_d [G][2][c] with slot 0
// = column sums of dx (the producer conv's bias-gradient partials; unetseg_colsum_rows reduces them)
UNETSEG_API int unetseg_pw_small_bwd_relu(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c,
                                          int k, const float* w, void* dx, int lddx, float* part_w, float* part_b,
                                          float* part_d, void* stream) {
  US_CHECK_ARG(dtype == DT_BF16, "pw_small_bwd_relu: bf16 only");
  CHECK_VEC(dtype, c, "pw_small_bwd_relu");
  US_CHECK_ARG(c / 8 <= 256 && 256 % (c / 8) == 0, "pw_small_bwd_relu: bad C");
  US_CHECK_ARG(k == 1 || k == 2, "pw_small_bwd_relu: k must be 1 or 2");
  CHECK_LD_VEC(dtype, ldx, c, "pw_small_bwd_relu", "ldx");
  CHECK_LD_VEC(dtype, lddx, c, "pw_small_bwd_relu", "lddx");
  CHECK_PIXELS(M, hw, "pw_small_bwd_relu");
  if (M == 0) return 0;
  US_CHECK_ARG(dx != nullptr && part_d != nullptr, "pw_small_bwd_relu: dx and part_d required");
  US_CHECK_ARG(dy && x && w && part_w && part_b, "pw_small_bwd_relu: null pointer");
  const int G = unetseg_pw_small_tiles(M);
  hipStream_t st = (hipStream_t)stream;
  pw_small_dispatch_k(k, [&](auto kc) {
    hipLaunchKernelGGL((pw_small_bwd_kernel<bf16, decltype(kc)::value, true>), dim3(G), dim3(256), 0, st, dy,
                       (const bf16*)x, ldx, M, hw, c, w, (bf16*)dx, lddx, 0, part_w, part_b, G, (int)pw_tile(M), part_d);
  });
  US_LAUNCH_CHECK("pw_small_bwd_relu");
  return 0;
}

UNETSEG_API int unetseg_pw_head_tiles(long M) { return ceil_div(M, (long)kHeadTile * 8); }

UNETSEG_API int unetseg_pw_head_fwd(int dtype, const void* x, int ldx, long M, int hw, int c, int k, const float* w,
                                    const float* b, float* y, void* stream) {
  US_CHECK_DTYPE(dtype, "pw_head_fwd");
  US_CHECK_ARG(k >= 1 && k <= kMaxC && c > 0 && c % vec_elems(dtype) == 0,
               "pw_head_fwd: bad args (k=%d <= %d, c=%d multiple of the 16-B vector)", k, kMaxC, c);
  CHECK_LD_VEC(dtype, ldx, c, "pw_head_fwd", "ldx");
  CHECK_PIXELS(M, hw, "pw_head_fwd");
  if (M == 0) return 0;
  US_CHECK_ARG(x && w && y, "pw_head_fwd: null pointer (x, w and y are required)");
  const size_t lds = (size_t)k * c * sizeof(float);
  DISPATCH_T(dtype, hipLaunchKernelGGL(pw_head_fwd_kernel<T>, dim3(ceil_div(M, 256)), dim3(256), lds,
                                       (hipStream_t)stream, (const T*)x, ldx, M, hw, c, k, w, b, y));
  US_LAUNCH_CHECK("pw_head_fwd");
  return 0;
}

// dx (may be NULL) (+)= dy . W ; part_w [k][c][G], part_b [k][G], G = unetseg_pw_head_tiles(M)
UNETSEG_API int unetseg_pw_head_bwd(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c, int k,
                                    const float* w, void* dx, int lddx, int dx_acc, float* part_w, float* part_b,
                                    void* stream) {
  US_CHECK_DTYPE(dtype, "pw_head_bwd");
  US_CHECK_ARG(k >= 1 && k <= kMaxC && c > 0 && c <= 256 && 256 % c == 0,
               "pw_head_bwd: bad args (k=%d, c=%d must divide 256)", k, c);
  // element-wise accesses: any ld >= c
  US_CHECK_ARG(ldx >= c && (!dx || lddx >= c), "pw_head_bwd: ldx (%d) and lddx (%d) must be at least c (%d)", ldx, lddx, c);
  CHECK_PIXELS(M, hw, "pw_head_bwd");
  if (M == 0) return 0;
  US_CHECK_ARG(dy && x && w && part_w && part_b, "pw_head_bwd: null pointer (only dx may be NULL)");
  const int G = unetseg_pw_head_tiles(M);
  const size_t lds = ((size_t)k * c + 256) * sizeof(float);
  DISPATCH_T(dtype, hipLaunchKernelGGL(pw_head_bwd_kernel<T>, dim3(G), dim3(256), lds, (hipStream_t)stream, dy,
                                       (const T*)x, ldx, M, hw, c, k, w, (T*)dx, lddx, dx_acc, part_w, part_b, G,
                                       kHeadTile * 8));
  US_LAUNCH_CHECK("pw_head_bwd");
  return 0;
}

UNETSEG_API int unetseg_attn_apply(int dtype, const void* skip, int lds_, const float* psi, const float* sc,
                                   const float* sh, float* alpha, void* gated, int ldg, long M, int c, void* stream) {
  CHECK_VEC(dtype, c, "attn_apply");
  CHECK_LD_VEC(dtype, lds_, c, "attn_apply", "lds");
  CHECK_LD_VEC(dtype, ldg, c, "attn_apply", "ldg");
  CHECK_PIXELS(M, 1, "attn_apply");
  if (M == 0) return 0;
  US_CHECK_ARG(skip && psi && sc && sh && alpha && gated, "attn_apply: null pointer");
  DISPATCH_T(dtype, hipLaunchKernelGGL(attn_apply_kernel<T>, dim3(grid_for(M * c / VE<T>)), dim3(256), 0,
                                       (hipStream_t)stream, (const T*)skip, lds_, psi, sc, sh, alpha, (T*)gated, ldg, M,
                                       c));
  US_LAUNCH_CHECK("attn_apply");
  return 0;
}

// 128-pixel tiles: the 64^2 x 512-channel gate has 32 K pixels, 2048-pixel tiles left 16 blocks
constexpr int kAttnBwd1Tile = 128;
UNETSEG_API int unetseg_attn_bwd1_tiles(long M) { return ceil_div(M, (long)kAttnBwd1Tile); }

UNETSEG_API int unetseg_attn_bwd1(int dtype, const void* dg, int ldg, const void* skip, int lds_, const float* alpha,
                                  const float* psi, const float* mean, const float* inv, void* dskip, int ldds,
                                  int ds_acc, float* dpsibn, long M, int c, float* part, void* stream) {
  CHECK_VEC(dtype, c, "attn_bwd1");
  const int cv = c / vec_elems(dtype);
  US_CHECK_ARG((cv & (cv - 1)) == 0, "attn_bwd1: C/V must be a power of two");
  CHECK_LD_VEC(dtype, ldg, c, "attn_bwd1", "ldg");
  CHECK_LD_VEC(dtype, lds_, c, "attn_bwd1", "lds");
  CHECK_LD_VEC(dtype, ldds, c, "attn_bwd1", "ldds");
  CHECK_PIXELS(M, 1, "attn_bwd1");
  if (M == 0) return 0;
  US_CHECK_ARG(dg && skip && alpha && psi && mean && inv && dskip && dpsibn && part, "attn_bwd1: null pointer");
  const int G = unetseg_attn_bwd1_tiles(M);
  if (ds_acc)
    DISPATCH_T(dtype, hipLaunchKernelGGL((attn_bwd1_kernel<T, true>), dim3(G), dim3(256), 0, (hipStream_t)stream,
                                         (const T*)dg, ldg, (const T*)skip, lds_, alpha, psi, mean, inv, (T*)dskip,
                                         ldds, dpsibn, M, c, kAttnBwd1Tile, part, G));
  else
    DISPATCH_T(dtype, hipLaunchKernelGGL((attn_bwd1_kernel<T, false>), dim3(G), dim3(256), 0, (hipStream_t)stream,
                                         (const T*)dg, ldg, (const T*)skip, lds_, alpha, psi, mean, inv, (T*)dskip,
                                         ldds, dpsibn, M, c, kAttnBwd1Tile, part, G));
  US_LAUNCH_CHECK("attn_bwd1");
  return 0;
}

UNETSEG_API int unetseg_attn_bwd2(int dtype, const float* dpsibn, const float* psi, const float* mean,
                                  const float* inv, const float* coef, const void* f, int ldf, const float* wpsi,
                                  void* dzf, int lddz, long M, int c, float* part_w, float* part_b, void* stream) {
  CHECK_VEC(dtype, c, "attn_bwd2");
  const int cv = c / vec_elems(dtype);
  US_CHECK_ARG(cv <= 256 && 256 % cv == 0, "attn_bwd2: bad C");
  CHECK_LD_VEC(dtype, ldf, c, "attn_bwd2", "ldf");
  CHECK_LD_VEC(dtype, lddz, c, "attn_bwd2", "lddz");
  CHECK_PIXELS(M, 1, "attn_bwd2");
  if (M == 0) return 0;
  US_CHECK_ARG(dpsibn && psi && mean && inv && coef && f && wpsi && dzf && part_w && part_b, "attn_bwd2: null pointer");
  const int G = unetseg_pw_small_tiles(M);
  DISPATCH_T(dtype, hipLaunchKernelGGL(attn_bwd2_kernel<T>, dim3(G), dim3(256), 0, (hipStream_t)stream, dpsibn, psi,
                                       mean, inv, coef, (const T*)f, ldf, wpsi, (T*)dzf, lddz, M, c, cv, (int)pw_tile(M), part_w,
                                       part_b, G));
  US_LAUNCH_CHECK("attn_bwd2");
  return 0;
}

UNETSEG_API int unetseg_add(int dtype, const void* x, int ldx, void* out, int ldo, long M, int c, void* stream) {
  CHECK_VEC(dtype, c, "add");
  US_CHECK_ARG(x && out && M >= 0 && ldx >= c && ldo >= c, "add: bad args");
  DISPATCH_T(dtype, hipLaunchKernelGGL(add_kernel<T>, dim3(grid_for(M * c / VE<T>)), dim3(256), 0, (hipStream_t)stream,
                                       (const T*)x, ldx, (T*)out, ldo, M, c));
  US_LAUNCH_CHECK("add");
  return 0;
}
