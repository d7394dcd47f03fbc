// Adam on the flat fp32 parameter arena, plain and capturable (hipGraph replay), each also fused with an
// exponential moving average (EMA) of the weights, and the exact in-place exchange of two fp32 arrays that puts
// the average into the arena for evaluation.
//
//   Adam           train.py:62-78 (torch.optim.Adam, coupled L2 weight decay)
#include "elem_util.h"

namespace {

// torch.optim.Adam single step on one element (coupled L2 weight decay): updates the moments in place and returns
// the new parameter.  The one definition of the update: the plain and the EMA kernels, scalar or four elements to
// a thread, give the same bits.  Which products the compiler fuses with the sum behind them depends on the code
// around the expression (it pairs the scalar loop's multiplications into packed ones and then fuses none of them,
// and fuses them all in a four-element body), so the choice is written out: every product and sum of gr, m' and
// v' rounds on its own and only the final update is one fused multiply-add -- what the scalar kernels have always
// computed.
__device__ __forceinline__ float adam_elem(float pv, float g, float& mv, float& vv, float inv_scale, float lr,
                                           float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
  float gr = g * inv_scale;
  if (wd != 0.f) gr = gr + wd * pv;
  mv = mv + (1.f - beta1) * (gr - mv);
  vv = vv * beta2 + (1.f - beta2) * gr * gr;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  return __builtin_fmaf(-(lr / bc1), mv / denom, pv);
}

// ema' = ema + (1 - d) (p' - ema), in this order: the difference rounds, the product and the sum are one fused op
__device__ __forceinline__ float ema_elem(float e, float pn, float omd) {
#pragma clang fp contract(off)
  return __builtin_fmaf(omd, pn - e, e);
}

// The bias coefficients of the capturable kernels, formed in double from the device step count (the update uses
// *step + 1) by thread 0: k[0] = 1 - b1^t, k[1] = sqrt(1 - b2^t) and, for the EMA form, k[2] = 1 - d_t with
// d_t = min(decay, (1 + t) / (10 + t)) under warm-up, decay otherwise.
__device__ __forceinline__ void dev_coeffs(float* k, const int* step, float beta1, float beta2) {
  const double t = (double)(step[0] + 1);
  const double bc1 = 1.0 - pow((double)beta1, t);
  const double bc2 = 1.0 - pow((double)beta2, t);
  k[0] = (float)bc1;
  k[1] = (float)sqrt(bc2);
}

__device__ __forceinline__ float dev_one_minus_decay(const int* step, float decay, int warmup) {
  const double t = (double)(step[0] + 1);
  double d = (double)decay;
  if (warmup) d = fmin(d, (1.0 + t) / (10.0 + t));
  return (float)(1.0 - d);
}

__global__ void adam_kernel(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                            float eps, float wd, float bc1, float bc2_sqrt, const float* grad_scale) {
  const float inv_scale = grad_scale ? 1.0f / grad_scale[0] : 1.0f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float mv = m[i], vv = v[i];
    const float pn = adam_elem(p[i], g[i], mv, vv, inv_scale, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
    m[i] = mv;
    v[i] = vv;
    p[i] = pn;
  }
}

// Capturable form (hipGraph replay): lr and the step count live in device memory, so a replayed
// step uses the current values.  hyper[0] = lr; *step is the count of steps already taken (the
// update uses *step + 1; adam_step_commit advances it afterwards).
__global__ void adam_dev_kernel(float* p, const float* g, float* m, float* v, long n, const float* hyper,
                                const int* step, float beta1, float beta2, float eps, float wd,
                                const float* grad_scale) {
  __shared__ float k[2];
  if (threadIdx.x == 0) dev_coeffs(k, step, beta1, beta2);
  __syncthreads();
  const float bc1 = k[0], bc2_sqrt = k[1], lr = hyper[0];
  const float inv_scale = grad_scale ? 1.0f / grad_scale[0] : 1.0f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float mv = m[i], vv = v[i];
    const float pn = adam_elem(p[i], g[i], mv, vv, inv_scale, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt);
    m[i] = mv;
    v[i] = vv;
    p[i] = pn;
  }
}

__global__ void adam_step_commit_kernel(int* step) { step[0] += 1; }

// ---- Adam + EMA in one pass: 5 reads and 4 writes per element (9 streams; Adam alone has 7) -----------------------
// A bucket slice starts at any element of its 256-B-aligned allocation, and the five arrays are cut at the same
// element: `head` elements (0..3) up to the first 16-B boundary, then 16-B vectors, then up to 3 tail elements.
// The host passes head = n (no vector body) when the five addresses are not congruent modulo 16.
struct AdamCoef {
  float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, inv_scale, omd;
};

__device__ __forceinline__ void adam_ema_one(float* p, const float* g, float* m, float* v, float* ema, long i,
                                             const AdamCoef& c) {
  float mv = m[i], vv = v[i];
  const float pn = adam_elem(p[i], g[i], mv, vv, c.inv_scale, c.lr, c.beta1, c.beta2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
  m[i] = mv;
  v[i] = vv;
  p[i] = pn;
  ema[i] = ema_elem(ema[i], pn, c.omd);
}

__device__ __forceinline__ void adam_ema_span(float* p, const float* g, float* m, float* v, float* ema, long n,
                                              long head, const AdamCoef& c) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;
  const long nvec = (n - head) / 4;
  for (long i = tid; i < head; i += nthr) adam_ema_one(p, g, m, v, ema, i, c);
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  float4* e4 = reinterpret_cast<float4*>(ema + head);
  for (long k = tid; k < nvec; k += nthr) {
    const float4 pq = p4[k], gq = g4[k];
    float4 mq = m4[k], vq = v4[k], eq = e4[k];
    float4 pn;
    pn.x = adam_elem(pq.x, gq.x, mq.x, vq.x, c.inv_scale, c.lr, c.beta1, c.beta2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    pn.y = adam_elem(pq.y, gq.y, mq.y, vq.y, c.inv_scale, c.lr, c.beta1, c.beta2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    pn.z = adam_elem(pq.z, gq.z, mq.z, vq.z, c.inv_scale, c.lr, c.beta1, c.beta2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    pn.w = adam_elem(pq.w, gq.w, mq.w, vq.w, c.inv_scale, c.lr, c.beta1, c.beta2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    eq.x = ema_elem(eq.x, pn.x, c.omd);
    eq.y = ema_elem(eq.y, pn.y, c.omd);
    eq.z = ema_elem(eq.z, pn.z, c.omd);
    eq.w = ema_elem(eq.w, pn.w, c.omd);
    m4[k] = mq;
    v4[k] = vq;
    p4[k] = pn;
    e4[k] = eq;
  }
  for (long i = head + 4 * nvec + tid; i < n; i += nthr) adam_ema_one(p, g, m, v, ema, i, c);
}

__global__ void adam_ema_kernel(float* p, const float* g, float* m, float* v, float* ema, long n, long head, float lr,
                                float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt, float omd,
                                const float* grad_scale) {
  const AdamCoef c{lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale ? 1.0f / grad_scale[0] : 1.0f, omd};
  adam_ema_span(p, g, m, v, ema, n, head, c);
}

__global__ void adam_ema_dev_kernel(float* p, const float* g, float* m, float* v, float* ema, long n, long head,
                                    const float* hyper, const int* step, float beta1, float beta2, float eps, float wd,
                                    float decay, int warmup, const float* grad_scale) {
  __shared__ float k[3];
  if (threadIdx.x == 0) {
    dev_coeffs(k, step, beta1, beta2);
    k[2] = dev_one_minus_decay(step, decay, warmup);
  }
  __syncthreads();
  const AdamCoef c{hyper[0], beta1, beta2, eps, wd, k[0], k[1], grad_scale ? 1.0f / grad_scale[0] : 1.0f, k[2]};
  adam_ema_span(p, g, m, v, ema, n, head, c);
}

// exact exchange of two fp32 arrays (bit patterns, no arithmetic); head as above
__global__ void swap_f32_kernel(unsigned* a, unsigned* b, long n, long head) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long nthr = (long)gridDim.x * blockDim.x;
  const long nvec = (n - head) / 4;
  for (long i = tid; i < head; i += nthr) {
    const unsigned x = a[i];
    a[i] = b[i];
    b[i] = x;
  }
  uint4* a4 = reinterpret_cast<uint4*>(a + head);
  uint4* b4 = reinterpret_cast<uint4*>(b + head);
  for (long k = tid; k < nvec; k += nthr) {
    const uint4 x = a4[k], y = b4[k];
    a4[k] = y;
    b4[k] = x;
  }
  for (long i = head + 4 * nvec + tid; i < n; i += nthr) {
    const unsigned x = a[i];
    a[i] = b[i];
    b[i] = x;
  }
}

// elements in front of the first 16-B boundary when every array sits at the same offset from one (bucket slices of
// 256-B-aligned allocations do); n, i.e. no vector body, otherwise.  Arrays are 4-byte aligned (checked).
template <typename... Ptr>
inline long vec_head(long n, const void* first, Ptr... rest) {
  const uintptr_t lo = (uintptr_t)first & 15;
  if (((((uintptr_t)rest & 15) != lo) || ...)) return n;
  const long head = (long)(((16 - lo) & 15) / 4);
  return head < n ? head : n;
}

template <typename... Ptr>
inline bool aligned4(Ptr... ptrs) {
  return ((((uintptr_t)ptrs & 3) == 0) && ...);
}

// 16-B vectors per thread: a quarter of the threads, so the cap that makes the stride loop wrap at the same
// element count as the scalar kernels' 16384 blocks
inline int vec_grid(long n, long head) { return head == n ? grid_for(n) : grid_for((n - head) / 4 + 1, 4096); }

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_adam(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                             float eps, float wd, int step, const float* grad_scale, void* stream) {
  US_CHECK_ARG(p && g && m && v && n >= 0, "adam: null pointer or negative size");
  US_CHECK_ARG(step >= 1, "adam: step must be >= 1");
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                     beta2, eps, wd, (float)bc1, (float)sqrt(bc2), grad_scale);
  US_LAUNCH_CHECK("adam");
  return 0;
}

UNETSEG_API int unetseg_adam_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step,
                                 float beta1, float beta2, float eps, float wd, const float* grad_scale,
                                 void* stream) {
  US_CHECK_ARG(p && g && m && v && n >= 0, "adam_dev: null pointer or negative size");
  US_CHECK_ARG(hyper && step, "adam_dev: hyper and step must be device pointers");
  hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, hyper, step,
                     beta1, beta2, eps, wd, grad_scale);
  hipLaunchKernelGGL(adam_step_commit_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
  US_LAUNCH_CHECK("adam_dev");
  return 0;
}

UNETSEG_API int unetseg_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr,
                                 float beta1, float beta2, float eps, float wd, int step, float one_minus_decay,
                                 const float* grad_scale, void* stream) {
  US_CHECK_ARG(p && g && m && v && ema && n >= 0, "adam_ema: null pointer or negative size");
  US_CHECK_ARG(aligned4(p, g, m, v, ema), "adam_ema: arrays must be 4-byte aligned");
  US_CHECK_ARG(step >= 1, "adam_ema: step must be >= 1");
  US_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "adam_ema: one_minus_decay (%g) must be in [0, 1]",
               (double)one_minus_decay);
  if (n == 0) return 0;
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  const long head = vec_head(n, p, g, m, v, ema);
  hipLaunchKernelGGL(adam_ema_kernel, dim3(vec_grid(n, head)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n,
                     head, lr, beta1, beta2, eps, wd, (float)bc1, (float)sqrt(bc2), one_minus_decay, grad_scale);
  US_LAUNCH_CHECK("adam_ema");
  return 0;
}

UNETSEG_API int unetseg_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, long n,
                                     const float* hyper, int* step, float beta1, float beta2, float eps, float wd,
                                     float decay, int warmup, const float* grad_scale, void* stream) {
  US_CHECK_ARG(p && g && m && v && ema && n >= 0, "adam_ema_dev: null pointer or negative size");
  US_CHECK_ARG(aligned4(p, g, m, v, ema), "adam_ema_dev: arrays must be 4-byte aligned");
  US_CHECK_ARG(hyper && step, "adam_ema_dev: hyper and step must be device pointers");
  US_CHECK_ARG(decay >= 0.f && decay <= 1.f, "adam_ema_dev: decay (%g) must be in [0, 1]", (double)decay);
  if (n == 0) return 0;  // nothing launched: *step stays too
  const long head = vec_head(n, p, g, m, v, ema);
  hipLaunchKernelGGL(adam_ema_dev_kernel, dim3(vec_grid(n, head)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema,
                     n, head, hyper, step, beta1, beta2, eps, wd, decay, warmup, grad_scale);
  hipLaunchKernelGGL(adam_step_commit_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
  US_LAUNCH_CHECK("adam_ema_dev");
  return 0;
}

UNETSEG_API int unetseg_swap_f32(float* a, float* b, long n, void* stream) {
  US_CHECK_ARG(a && b && n >= 0, "swap_f32: null pointer or negative size");
  US_CHECK_ARG(aligned4(a, b), "swap_f32: arrays must be 4-byte aligned");
  if (n == 0) return 0;
  const long head = vec_head(n, a, b);
  hipLaunchKernelGGL(swap_f32_kernel, dim3(vec_grid(n, head)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<unsigned*>(a), reinterpret_cast<unsigned*>(b), n, head);
  US_LAUNCH_CHECK("swap_f32");
  return 0;
}
