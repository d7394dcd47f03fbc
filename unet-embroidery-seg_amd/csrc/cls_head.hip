// The multitask model's classification head: global average pooling, the linear layers (ReLU /
// dropout) and their cross entropy.
//
//   CE + cls head  model/unet_multitask.py:73-80,109-139
#include "elem_util.h"

namespace {

// ------------------------------------------------------------------------------------------
// multitask classification head (model/unet_multitask.py:73-80)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void gap_kernel(const T* x, int ldx, int B, int HW, int C, float* g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C;
  double s = 0.0;
  for (int p = 0; p < HW; ++p) s += (float)x[((long)b * HW + p) * ldx + c];
  g[i] = (float)(s / HW);
}

template <typename T>
__global__ void gap_bwd_kernel(const float* dg, int B, int HW, int C, T* dx, int ldx, int accumulate) {
  const long total = (long)B * HW * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long pix = i / C;
    const int c = (int)(i - pix * C);
    const int b = (int)(pix / HW);
    T* o = dx + pix * ldx + c;
    float v = dg[(long)b * C + c] / (float)HW;
    if (accumulate) v += (float)(*o);
    *o = (T)v;
  }
}

__device__ __forceinline__ float hash_u01(unsigned long long seed, unsigned long long i) {
  unsigned long long z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// y[b][o] = act(sum_i x[b][i] W[o][i] + bias[o]); act: 0 none, 1 relu, 2 relu + dropout(p)
// one wave per output element
__global__ void linear_fwd_kernel(const float* x, const float* W, const float* bias, int B, int I, int O, int act,
                                  float p_drop, unsigned long long seed, const float* mask_in, float* mask_out,
                                  float* pre, float* y) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= B * O) return;
  const int b = wave / O, o = wave - b * O;
  float s = 0.f;
  // eight rounds' loads in flight (the plain loop waited out one round trip per 64 inputs); the
  // products are added in the same i order
  constexpr int U = 8;
  int i = lane;
  for (; i + 64 * (U - 1) < I; i += 64 * U) {
    float xv[U], wv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xv[u] = x[(long)b * I + i + 64 * u];
      wv[u] = W[(long)o * I + i + 64 * u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s = fmaf(xv[u], wv[u], s);  // explicit: as the plain loop's contraction
  }
  for (; i < I; i += 64) s += x[(long)b * I + i] * W[(long)o * I + i];
  s = wave_sum(s);
  if (lane == 0) {
    s += bias ? bias[o] : 0.f;
    if (pre) pre[wave] = s;
    if (act >= 1) s = fmaxf(s, 0.f);
    if (act == 2) {
      float keep;
      if (mask_in) keep = mask_in[wave];
      else keep = hash_u01(seed, (unsigned long long)wave) >= p_drop ? 1.f : 0.f;
      if (mask_out) mask_out[wave] = keep;
      s = s * keep / (1.f - p_drop);
    }
    y[wave] = s;
  }
}

// backward of linear (+ act): dyp = dy * act'(pre) ; dx[b][i] = sum_o dyp W[o][i] ; dW += ; db +=
__global__ void linear_act_bwd_kernel(const float* dy, const float* pre, const float* mask, float p_drop, int act,
                                      int B, int O, float* dyp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * O) return;
  float g = dy[i];
  if (act >= 1 && pre[i] <= 0.f) g = 0.f;
  if (act == 2) g = g * mask[i] / (1.f - p_drop);
  dyp[i] = g;
}

__global__ void linear_bwd_x_kernel(const float* dyp, const float* W, int B, int I, int O, float* dx) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * I) return;
  const int b = t / I, i = t - b * I;
  float s = 0.f;
  // 32 outputs' loads in flight per round (one round trip per load left the 2048 -> 512 FC's
  // backward at ~100 us); the products are added in the same o order as the plain loop
  constexpr int U = 32;
  int o = 0;
  for (; o + U <= O; o += U) {
    float d[U], w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      d[u] = dyp[(long)b * O + o + u];
      w[u] = W[(long)(o + u) * I + i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) s = fmaf(d[u], w[u], s);  // explicit: the packed-multiply form rounds twice
  }
  for (; o < O; ++o) s += dyp[(long)b * O + o] * W[(long)o * I + i];
  dx[t] = s;
}

__global__ void linear_bwd_w_kernel(const float* dyp, const float* x, int B, int I, int O, float* dW, float* db) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= O * I) return;
  const int o = t / I, i = t - o * I;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += dyp[(long)b * O + o] * x[(long)b * I + i];
  dW[t] += s;
  if (i == 0 && db) {
    float sb = 0.f;
    for (int b = 0; b < B; ++b) sb += dyp[(long)b * O + o];
    db[o] += sb;
  }
}

// cross entropy (mean) over B rows of K logits; dlog = (softmax - onehot)/B (unscaled)
// nn.CrossEntropyLoss() (mean, ignore_index -100): rows whose target is -100 contribute nothing and
// the mean runs over the others; any other target outside [0, K) makes the loss and its gradient
// NaN (torch raises; no out-of-range read here either way).
__global__ void ce_kernel(const float* logits, const int64_t* tgt, int B, int K, float* loss, float* dlog) {
  __shared__ double sred[16];
  __shared__ int cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  int nvalid = 0, nbad = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const long long t = tgt[b];
    nvalid += (t >= 0 && t < K) ? 1 : 0;
    nbad += (t != -100 && (t < 0 || t >= K)) ? 1 : 0;
  }
  atomicAdd(&cnt[0], nvalid);  // LDS atomics
  atomicAdd(&cnt[1], nbad);
  __syncthreads();
  const float denom = (float)max(cnt[0], 1);
  const bool bad = cnt[1] > 0;
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const float* l = logits + (long)b * K;
    const long long t = tgt[b];
    const bool ok = t >= 0 && t < K;
    float mx = l[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, l[k]);
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(l[k] - mx);
    const float lse = mx + logf(se);
    if (ok) s += (double)(lse - l[t]);
    for (int k = 0; k < K; ++k)
      dlog[(long)b * K + k] = bad ? NAN : ok ? (expf(l[k] - lse) - (k == t ? 1.f : 0.f)) / denom : 0.f;
  }
  s = block_sum(s, sred);
  if (threadIdx.x == 0) loss[0] = bad ? NAN : cnt[0] == 0 ? NAN : (float)(s / (double)cnt[0]);
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_gap_fwd(int dtype, const void* x, int ldx, int B, int HW, int C, float* g, void* stream) {
  US_CHECK_DTYPE(dtype, "gap_fwd");
  US_CHECK_ARG(B >= 0 && HW > 0 && C > 0 && ldx >= C, "gap_fwd: bad sizes (B=%d HW=%d C=%d; ldx=%d must be at least C)", B, HW, C, ldx);
  if (B == 0) return 0;
  US_CHECK_ARG(x && g, "gap_fwd: null pointer");
  DISPATCH_T(dtype, hipLaunchKernelGGL(gap_kernel<T>, dim3(ceil_div(B * C, 256)), dim3(256), 0, (hipStream_t)stream,
                                       (const T*)x, ldx, B, HW, C, g));
  US_LAUNCH_CHECK("gap_fwd");
  return 0;
}

UNETSEG_API int unetseg_gap_bwd(int dtype, const float* dg, int B, int HW, int C, void* dx, int ldx, int accumulate,
                                void* stream) {
  US_CHECK_DTYPE(dtype, "gap_bwd");
  US_CHECK_ARG(B >= 0 && HW >= 0 && C > 0 && ldx >= C, "gap_bwd: bad sizes (B=%d HW=%d C=%d; ldx=%d must be at least C)", B, HW, C, ldx);
  if ((long)B * HW == 0) return 0;
  US_CHECK_ARG(dg && dx, "gap_bwd: null pointer");
  const long n = (long)B * HW * C;
  DISPATCH_T(dtype, hipLaunchKernelGGL(gap_bwd_kernel<T>, dim3(grid_for(n, 8192)), dim3(256), 0,
                                       (hipStream_t)stream, dg, B, HW, C, (T*)dx, ldx, accumulate));
  US_LAUNCH_CHECK("gap_bwd");
  return 0;
}

UNETSEG_API int unetseg_linear_fwd(const float* x, const float* W, const float* bias, int B, int I, int O, int act,
                                   float p_drop, unsigned long long seed, const float* mask_in, float* mask_out,
                                   float* pre, float* y, void* stream) {
  US_CHECK_ARG(x && W && y && B > 0 && I > 0 && O > 0, "linear_fwd: null pointer or empty shape");
  US_CHECK_ARG(act >= 0 && act <= 2 && (act != 2 || p_drop < 1.f), "linear_fwd: act %d / p_drop %g", act, p_drop);
  const long threads = (long)B * O * 64;
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream, x, W, bias, B,
                     I, O, act, p_drop, seed, mask_in, mask_out, pre, y);
  US_LAUNCH_CHECK("linear_fwd");
  return 0;
}

// dx (may be NULL) = dyp . W ; dW += dyp^T x ; db += sum dyp ; scratch: B*O floats
UNETSEG_API int unetseg_linear_bwd(const float* dy, const float* pre, const float* mask, float p_drop, int act,
                                   const float* x, const float* W, int B, int I, int O, float* dx, float* dW, float* db,
                                   float* scratch, void* stream) {
  US_CHECK_ARG(dy && x && W && dW && db && scratch && B > 0 && I > 0 && O > 0, "linear_bwd: null pointer or empty shape");
  US_CHECK_ARG(act >= 0 && act <= 2 && (act == 0 || pre) && (act != 2 || (mask && p_drop < 1.f)),
               "linear_bwd: act %d needs pre (and the dropout mask)", act);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(linear_act_bwd_kernel, dim3(ceil_div(B * O, 256)), dim3(256), 0, st, dy, pre, mask, p_drop, act, B,
                     O, scratch);
  if (dx) hipLaunchKernelGGL(linear_bwd_x_kernel, dim3(ceil_div(B * I, 256)), dim3(256), 0, st, scratch, W, B, I, O, dx);
  hipLaunchKernelGGL(linear_bwd_w_kernel, dim3(ceil_div(O * I, 256)), dim3(256), 0, st, scratch, x, B, I, O, dW, db);
  US_LAUNCH_CHECK("linear_bwd");
  return 0;
}

UNETSEG_API int unetseg_ce_fwd(const float* logits, const int64_t* tgt, int B, int K, float* loss, float* dlog,
                               void* stream) {
  US_CHECK_ARG(logits && tgt && loss && dlog && B > 0 && K > 0, "ce_fwd: null pointer or empty shape");
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, tgt, B, K, loss, dlog);
  US_LAUNCH_CHECK("ce_fwd");
  return 0;
}
