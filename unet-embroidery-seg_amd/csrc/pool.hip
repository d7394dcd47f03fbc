// Max-pool forward and backward, NHWC (layout and element types as bn.hip).
//
// Reference ops replaced:
//   MaxPool2d        model/resnet_backbone.py:131 (3x3/s2 ceil)  model/unet_plain.py:25 (2x2)
#include "elem_util.h"

namespace {

// ------------------------------------------------------------------------------------------
// Max pool (pad 0), NHWC.  idx = argmax position inside the k x k window (first max wins, the
// scan order of ATen's CPU kernel), stored as uint8.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void maxpool_fwd_kernel(const T* x, int ldx, int N, int H, int W, int C, int k, int s, int P, int Q, T* y,
                                   int ldy, uint8_t* idx) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const long total = (long)N * P * Q * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const int v = (int)(t % cv); t /= cv;
    const int q = (int)(t % Q); t /= Q;
    const int p = (int)(t % P);
    const int n = (int)(t / P);
    const int c0 = v * V;
    float best[V];
    uint8_t bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    for (int r = 0; r < k; ++r) {
      const int h = p * s + r;
      if (h >= H) break;
      for (int u = 0; u < k; ++u) {
        const int w = q * s + u;
        if (w >= W) break;
        float xv[V];
        load_vec(x + ((long)(n * H + h) * W + w) * ldx + c0, xv);
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (xv[e] > best[e] || isnan(xv[e])) {
            if (!isnan(best[e])) { best[e] = xv[e]; bi[e] = (uint8_t)(r * k + u); }
          }
      }
    }
    const long opix = ((long)(n * P + p) * Q + q);
    store_vec(y + opix * ldy + c0, best);
#pragma unroll
    for (int e = 0; e < V; ++e) idx[opix * C + c0 + e] = bi[e];
  }
}

// The ResNet stem's pool (model/resnet_backbone.py:135: 3x3, stride 2, ceil mode) with the window
// compile-time: unrolled taps, 32-bit indexing, the 8 (bf16) argmax bytes of a pixel stored with one
// 8-B store.  Same comparisons in the same order as maxpool_fwd_kernel (bit-identical).
template <typename T>
__global__ void maxpool_fwd_k3s2_kernel(const T* x, int ldx, int N, int H, int W, int C, int P, int Q, T* y, int ldy,
                                        uint8_t* idx) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const int total = N * P * Q * cv;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int t = i;
    const int v = t % cv; t /= cv;
    const int q = t % Q; t /= Q;
    const int p = t % P;
    const int n = t / P;
    const int c0 = v * V;
    float best[V];
    uint8_t bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int h = p * 2 + r;
      if (h >= H) break;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int w = q * 2 + u;
        if (w >= W) break;
        float xv[V];
        load_vec(x + (size_t)((n * H + h) * W + w) * ldx + c0, xv);
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (xv[e] > best[e] || isnan(xv[e])) {
            if (!isnan(best[e])) { best[e] = xv[e]; bi[e] = (uint8_t)(r * 3 + u); }
          }
      }
    }
    const size_t opix = (size_t)((n * P + p) * Q + q);
    store_vec(y + opix * ldy + c0, best);
    if constexpr (V == 8) {
      uint2 pk;
      __builtin_memcpy(&pk, bi, 8);
      *reinterpret_cast<uint2*>(idx + opix * C + c0) = pk;
    } else {
      unsigned pk;
      __builtin_memcpy(&pk, bi, 4);
      *reinterpret_cast<unsigned*>(idx + opix * C + c0) = pk;
    }
  }
}

// Its gradient: one thread per 2x2 input block (h = 2i + a, w = 2j + b) and V channels.  The windows
// that contain the block are (i-1 | i) x (j-1 | j); window (p, q) reaches row a of the block as window
// row r = a + 2 (p = i - 1, a = 0 only) or r = a (p = i), likewise columns.  Each window's dy and
// argmax bytes are loaded once per block (the per-pixel gather loaded them up to 9 times and the
// bytes one at a time); every pixel sums its windows in the same (p, q) order as maxpool_bwd_kernel.
template <typename T>
__global__ void maxpool_bwd_k3s2_kernel(const T* dy, int ldy, const uint8_t* idx, int N, int H, int W, int C, int P,
                                        int Q, T* dx, int ldx, int accumulate) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const int Hh = (H + 1) >> 1, Wh = (W + 1) >> 1;
  const int total = N * Hh * Wh * cv;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int t = i;
    const int v = t % cv; t /= cv;
    const int bj = t % Wh; t /= Wh;
    const int bi = t % Hh;
    const int n = t / Hh;
    const int c0 = v * V;
    float acc[4][V];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < V; ++e) acc[k][e] = 0.f;
    // the four windows' dy and argmax bytes loaded first, at clamped (valid) windows: under the
    // window-range conditions each window's loads were a branch with a vmcnt(0) behind it; windows out
    // of range are skipped below, in the same (p, q) order
    uint4 graw[4];
    uint2 iraw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = min(max(bi - 1 + (k >> 1), 0), P - 1), q = min(max(bj - 1 + (k & 1), 0), Q - 1);
      const size_t opix = (size_t)((n * P + p) * Q + q);
      graw[k] = *reinterpret_cast<const uint4*>(dy + opix * ldy + c0);
      if constexpr (V == 8) iraw[k] = *reinterpret_cast<const uint2*>(idx + opix * C + c0);
      else iraw[k].x = *reinterpret_cast<const unsigned*>(idx + opix * C + c0);
    }
#pragma unroll
    for (int dp = 0; dp < 2; ++dp) {
      const int p = bi - 1 + dp;
      if (p < 0 || p >= P) continue;
#pragma unroll
      for (int dq = 0; dq < 2; ++dq) {
        const int q = bj - 1 + dq;
        if (q < 0 || q >= Q) continue;
        float g[V];
        cvt16<T>(graw[dp * 2 + dq], g);
        uint8_t ib[V];
        __builtin_memcpy(ib, &iraw[dp * 2 + dq], V);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int r = dp ? a : a + 2;
          if (r >= 3) continue;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int u = dq ? b : b + 2;
            if (u >= 3) continue;
            const uint8_t want = (uint8_t)(r * 3 + u);
#pragma unroll
            for (int e = 0; e < V; ++e)
              if (ib[e] == want) acc[a * 2 + b][e] += g[e];
          }
        }
      }
    }
    uint4 oraw[4];  // the block's old gradient (accumulate), likewise loaded up front at clamped pixels
    if (accumulate)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int h = min(2 * bi + (k >> 1), H - 1), w = min(2 * bj + (k & 1), W - 1);
        oraw[k] = *reinterpret_cast<const uint4*>(dx + (size_t)((n * H + h) * W + w) * ldx + c0);
      }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int h = 2 * bi + a;
      if (h >= H) continue;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int w = 2 * bj + b;
        if (w >= W) continue;
        T* o = dx + (size_t)((n * H + h) * W + w) * ldx + c0;
        if (accumulate) {
          float old[V];
          cvt16<T>(oraw[a * 2 + b], old);
#pragma unroll
          for (int e = 0; e < V; ++e) acc[a * 2 + b][e] += old[e];
        }
        store_vec(o, acc[a * 2 + b]);
      }
    }
  }
}

// The U-Net encoders' 2x2 / stride-2 pool (model/unet_plain.py:25, model/unet_attention.py) when the
// windows tile the input exactly (h = 2P, w = 2Q): one thread per window and V channels, the four
// loads issued together (the generic kernel's loop waited on each), the same comparisons in the same
// order as maxpool_fwd_kernel (bit-identical), the argmax bytes stored with one 8-B store.
template <typename T>
__global__ void maxpool_fwd_k2s2_kernel(const T* x, int ldx, int N, int H, int W, int C, int P, int Q, T* y, int ldy,
                                        uint8_t* idx) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const int total = N * P * Q * cv;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int t = i;
    const int v = t % cv; t /= cv;
    const int q = t % Q; t /= Q;
    const int p = t % P;
    const int n = t / P;
    const int c0 = v * V;
    float xv[4][V];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int u = 0; u < 2; ++u) load_vec(x + (size_t)((n * H + 2 * p + r) * W + 2 * q + u) * ldx + c0, xv[r * 2 + u]);
    float best[V];
    uint8_t bi[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (xv[j][e] > best[e] || isnan(xv[j][e])) {
          if (!isnan(best[e])) { best[e] = xv[j][e]; bi[e] = (uint8_t)j; }
        }
    const size_t opix = (size_t)((n * P + p) * Q + q);
    store_vec(y + opix * ldy + c0, best);
    if constexpr (V == 8) {
      uint2 pk;
      __builtin_memcpy(&pk, bi, 8);
      *reinterpret_cast<uint2*>(idx + opix * C + c0) = pk;
    } else {
      unsigned pk;
      __builtin_memcpy(&pk, bi, 4);
      *reinterpret_cast<unsigned*>(idx + opix * C + c0) = pk;
    }
  }
}

// Its gradient: each input pixel lies in exactly one window, so one thread per window writes the
// window's four pixels from one dy load and one argmax load (the generic gather loaded the argmax
// bytes one at a time); values as maxpool_bwd_kernel's (0 + dy where the argmax matches, then + old).
template <typename T>
__global__ void maxpool_bwd_k2s2_kernel(const T* dy, int ldy, const uint8_t* idx, int N, int H, int W, int C, int P,
                                        int Q, T* dx, int ldx, int accumulate) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const int total = N * P * Q * cv;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int t = i;
    const int v = t % cv; t /= cv;
    const int q = t % Q; t /= Q;
    const int p = t % P;
    const int n = t / P;
    const int c0 = v * V;
    const size_t opix = (size_t)((n * P + p) * Q + q);
    float g[V];
    load_vec(dy + opix * ldy + c0, g);
    uint8_t ib[V];
    if constexpr (V == 8) {
      const uint2 pk = *reinterpret_cast<const uint2*>(idx + opix * C + c0);
      __builtin_memcpy(ib, &pk, 8);
    } else {
      const unsigned pk = *reinterpret_cast<const unsigned*>(idx + opix * C + c0);
      __builtin_memcpy(ib, &pk, 4);
    }
    float old[4][V];
    if (accumulate)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        load_vec(dx + (size_t)((n * H + 2 * p + (j >> 1)) * W + 2 * q + (j & 1)) * ldx + c0, old[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        o[e] = 0.f;
        if (ib[e] == (uint8_t)j) o[e] += g[e];
        if (accumulate) o[e] += old[j][e];
      }
      store_vec(dx + (size_t)((n * H + 2 * p + (j >> 1)) * W + 2 * q + (j & 1)) * ldx + c0, o);
    }
  }
}

// gather form: dx[h][w] (+)= sum over windows containing (h,w) whose argmax is (h,w)
template <typename T>
__global__ void maxpool_bwd_kernel(const T* dy, int ldy, const uint8_t* idx, int N, int H, int W, int C, int k, int s,
                                   int P, int Q, T* dx, int ldx, int accumulate) {
  constexpr int V = VE<T>;
  const int cv = C / V;
  const long total = (long)N * H * W * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const int v = (int)(t % cv); t /= cv;
    const int w = (int)(t % W); t /= W;
    const int h = (int)(t % H);
    const int n = (int)(t / H);
    const int c0 = v * V;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    const int plo = max(0, (h - k + s) / s), phi = min(P - 1, h / s);
    const int qlo = max(0, (w - k + s) / s), qhi = min(Q - 1, w / s);
    for (int p = plo; p <= phi; ++p) {
      const int r = h - p * s;
      if (r < 0 || r >= k) continue;
      for (int q = qlo; q <= qhi; ++q) {
        const int u = w - q * s;
        if (u < 0 || u >= k) continue;
        const long opix = ((long)(n * P + p) * Q + q);
        const uint8_t want = (uint8_t)(r * k + u);
        float g[V];
        load_vec(dy + opix * ldy + c0, g);
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (idx[opix * C + c0 + e] == want) acc[e] += g[e];
      }
    }
    T* o = dx + ((long)(n * H + h) * W + w) * ldx + c0;
    if (accumulate) {
      float old[V];
      load_vec(o, old);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += old[e];
    }
    store_vec(o, acc);
  }
}

// Which kernel pair a pool runs: the 2x2 / stride-2 one when the windows tile the input exactly, the
// 3x3 / stride-2 one, else the generic one.  The two special forms index in 32 bits, so every extent
// (input of pixel stride ld_in, pooled tensor of pixel stride ld_out) must fit.  UNETSEG_MAXPOOL_GENERIC
// (tests; read at every call) forces the generic kernels.
enum PoolKind { kPoolGeneric, kPoolK2S2, kPoolK3S2 };
PoolKind pool_kind(int n, int h, int w, int c, int k, int s, int p, int q, int ld_in, int ld_out) {
  const bool fits = (long)n * h * w * c < (1L << 31) && (long)n * h * w * ld_in < (1L << 31) &&
                    (long)n * p * q * ld_out < (1L << 31) && !getenv("UNETSEG_MAXPOOL_GENERIC");
  if (k == 2 && s == 2 && h == 2 * p && w == 2 * q && fits) return kPoolK2S2;
  if (k == 3 && s == 2 && fits) return kPoolK3S2;
  return kPoolGeneric;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_maxpool_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c, int k, int s,
                                    int ceil_mode, void* y, int ldy, uint8_t* idx, int* p_out, int* q_out,
                                    void* stream) {
  CHECK_VEC(dtype, c, "maxpool_fwd");
  US_CHECK_ARG(x && y && idx, "maxpool_fwd: null pointer");
  US_CHECK_ARG(k >= 1 && k <= 16 && s >= 1 && n >= 0 && h >= k && w >= k, "maxpool_fwd: bad window k=%d s=%d on %dx%d", k,
               s, h, w);
  int p = ceil_mode ? (h - k + s - 1) / s + 1 : (h - k) / s + 1;
  int q = ceil_mode ? (w - k + s - 1) / s + 1 : (w - k) / s + 1;
  if (ceil_mode) {  // last window must start inside the input (ATen pooling_output_shape)
    if ((p - 1) * s >= h) --p;
    if ((q - 1) * s >= w) --q;
  }
  if (p_out) *p_out = p;
  if (q_out) *q_out = q;
  if (!y) return 0;  // shape query (unreachable: the null-pointer check above already rejects a null y)
  const dim3 grid(grid_for((long)n * p * q * c / vec_elems(dtype)));
  hipStream_t st = (hipStream_t)stream;
  switch (pool_kind(n, h, w, c, k, s, p, q, ldx, ldy)) {
    case kPoolK2S2:
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_fwd_k2s2_kernel<T>, grid, dim3(256), 0, st, (const T*)x, ldx, n, h,
                                           w, c, p, q, (T*)y, ldy, idx));
      break;
    case kPoolK3S2:
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_fwd_k3s2_kernel<T>, grid, dim3(256), 0, st, (const T*)x, ldx, n, h,
                                           w, c, p, q, (T*)y, ldy, idx));
      break;
    case kPoolGeneric:
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_fwd_kernel<T>, grid, dim3(256), 0, st, (const T*)x, ldx, n, h, w, c,
                                           k, s, p, q, (T*)y, ldy, idx));
      break;
  }
  US_LAUNCH_CHECK("maxpool_fwd");
  return 0;
}

UNETSEG_API int unetseg_maxpool_bwd(int dtype, const void* dy, int ldy, const uint8_t* idx, int n, int h, int w,
                                    int c, int k, int s, int p, int q, void* dx, int ldx, int accumulate,
                                    void* stream) {
  CHECK_VEC(dtype, c, "maxpool_bwd");
  US_CHECK_ARG(dy && idx && dx && k >= 1 && s >= 1 && n >= 0 && h >= 0 && w >= 0, "maxpool_bwd: bad args");
  const int V = vec_elems(dtype);
  hipStream_t st = (hipStream_t)stream;
  switch (pool_kind(n, h, w, c, k, s, p, q, ldx, ldy)) {
    case kPoolK2S2:  // one thread per window
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_bwd_k2s2_kernel<T>, dim3(grid_for((long)n * p * q * c / V)),
                                           dim3(256), 0, st, (const T*)dy, ldy, idx, n, h, w, c, p, q, (T*)dx, ldx,
                                           accumulate));
      break;
    case kPoolK3S2:  // one thread per 2x2 input block
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_bwd_k3s2_kernel<T>,
                                           dim3(grid_for((long)n * ((h + 1) / 2) * ((w + 1) / 2) * c / V)), dim3(256),
                                           0, st, (const T*)dy, ldy, idx, n, h, w, c, p, q, (T*)dx, ldx, accumulate));
      break;
    case kPoolGeneric:  // one thread per input pixel
      DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid_for((long)n * h * w * c / V)), dim3(256), 0,
                                           st, (const T*)dy, ldy, idx, n, h, w, c, k, s, p, q, (T*)dx, ldx,
                                           accumulate));
      break;
  }
  US_LAUNCH_CHECK("maxpool_bwd");
  return 0;
}
