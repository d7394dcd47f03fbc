// Multiclass segmentation kernels: the fused CE / Focal / Dice losses and the multiclass confusion
// histogram.  (The C-way 1x1 head is in pointwise.hip, predict.py's softmax -> crop -> resize ->
// argmax in tiles.hip.)
//
// Reference ops replaced:
//   CE_Loss / Focal_Loss / Dice_loss   model/unet_training.py:9-91
//   pixel_accuracy / mean_accuracy / mean_iou / frequency_weighted_iou   utils/train_and_eval.py:20-103
//
// Logits are fp32 planar [B][C][P] (the reference's NCHW output).
// Every reduction is two-stage (per-block partials -> one finalize block), hence deterministic.
#include <cmath>

#include "elem_util.h"

namespace {

// ------------------------------------------------------------------------------------------
// Fused multiclass loss.  Per pixel i (image b, position p), logits x_c, target t:
//   CE    (nn.CrossEntropyLoss(weight, ignore_index)): w_t (lse - x_t), mean = sum / sum w_t
//   Focal (reduction none, then alpha, gamma, mean over ALL pixels): logpt = -w_t nll (0 if ignored),
//         pt = exp(logpt), L = -(1-pt)^gamma * alpha * logpt
//   Dice  on softmax p and a float one-hot target [B][P][ct] (first C channels):
//         tp_c = sum t p, S_c = sum p, T_c = sum t; score_c = ((1+b^2) tp + s) / ((1+b^2) tp + b^2 fn + fp + s)
// Partials per block: [0] sum w*nll, [1] sum w, [2] sum focal, then tp[C], S[C], T[C].
// ------------------------------------------------------------------------------------------
struct McArgs {
  const float* out;
  const int64_t* tgt;
  const float* cls_w;   // [C] or NULL (= ones)
  const float* dice_t;  // [B][P][ct] float or NULL (no Dice)
  int B, C, ct;
  long P;
  long ignore;          // ignore_index
  int focal;            // main term: 0 CE, 1 Focal, 2 none (Dice only)
  float alpha, gamma;   // Focal (alpha < 0: None)
  float beta, smooth;   // Dice
};

__device__ __forceinline__ void softmax_pixel(const McArgs& a, long i, float (&x)[kMaxC], float& lse) {
  const long b = i / a.P, p = i - b * a.P;
  const float* base = a.out + b * a.C * a.P + p;
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c)
    if (c < a.C) {
      x[c] = base[(long)c * a.P];
      m = fmaxf(m, x[c]);
    }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c)
    if (c < a.C) s += expf(x[c] - m);
  lse = m + logf(s);
}

__global__ __launch_bounds__(256) void mc_loss_partial_kernel(McArgs a, float* part, int G) {
  const int NP = 3 + 3 * a.C;
  __shared__ float red[256];
  float acc_wnll = 0.f, acc_w = 0.f, acc_f = 0.f;
  float tp[kMaxC], S[kMaxC], T[kMaxC];
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) tp[c] = S[c] = T[c] = 0.f;
  const long total = (long)a.B * a.P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float x[kMaxC], lse;
    softmax_pixel(a, i, x, lse);
    const long t = (a.tgt && a.focal != 2) ? a.tgt[i] : -1;
    const bool valid = t != a.ignore && t >= 0 && t < a.C;
    const float wt = valid ? (a.cls_w ? a.cls_w[t] : 1.f) : 0.f;
    float xt = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c == t) xt = x[c];
    const float nll = valid ? lse - xt : 0.f;
    acc_wnll += wt * nll;
    acc_w += wt;
    if (a.tgt && a.focal != 2 && t != a.ignore && !valid) {
      // a target that is neither a class nor ignore_index: nn.CrossEntropyLoss (the reference's CE_Loss
      // / Focal_Loss, model/unet_training.py:9-59) refuses it; here loss and gradient become NaN
      acc_w += __builtin_nanf("");
      acc_f += __builtin_nanf("");
    }
    if (a.focal == 1) {
      const float logpt = -(wt * nll);
      const float pt = expf(logpt);
      const float lp = a.alpha >= 0.f ? logpt * a.alpha : logpt;
      acc_f += -powf(1.f - pt, a.gamma) * lp;
    }
    if (a.dice_t) {
      const float* tt = a.dice_t + i * a.ct;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < a.C) {
          const float pc = expf(x[c] - lse), tc = tt[c];
          tp[c] += tc * pc;
          S[c] += pc;
          T[c] += tc;
        }
    }
  }
  auto reduce = [&](float v, int slot) {
    const float s = block_sum(v, red);
    if (threadIdx.x == 0) part[(long)blockIdx.x * NP + slot] = s;
  };
  reduce(acc_wnll, 0);
  reduce(acc_w, 1);
  reduce(acc_f, 2);
  if (a.dice_t)
    for (int c = 0; c < a.C; ++c) {
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
      for (int cc = 0; cc < kMaxC; ++cc)
        if (cc == c) v0 = tp[cc], v1 = S[cc], v2 = T[cc];
      reduce(v0, 3 + c);
      reduce(v1, 3 + a.C + c);
      reduce(v2, 3 + 2 * a.C + c);
    }
}

// sums (fp64, fixed order) -> loss[0] total, [1] main (CE or Focal), [2] Dice (0 if off);
// coef: [0] sum w (CE denominator), [1] B*P, then per class A_c, Bd_c (Dice numerator/denominator)
__global__ void mc_loss_finalize_kernel(McArgs a, const float* part, int G, float* loss, double* coef) {
  const int NP = 3 + 3 * a.C;
  __shared__ double s[3 + 3 * kMaxC];
  for (int j = threadIdx.x; j < NP; j += blockDim.x) {
    double t = 0.0;
    for (int g = 0; g < G; ++g) t += (double)part[(long)g * NP + j];
    s[j] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = (double)a.B * (double)a.P;
  const double main = a.focal == 2 ? 0.0 : a.focal == 1 ? s[2] / n : s[0] / s[1];
  double dice = 0.0;
  const bool bad = s[1] != s[1];  // an invalid target poisoned the weight sum (partial kernel)
  coef[0] = s[1];
  coef[1] = bad ? s[1] : n;
  if (a.dice_t) {
    const double b2 = (double)a.beta * a.beta;
    double mean = 0.0;
    for (int c = 0; c < a.C; ++c) {
      const double tp = s[3 + c], S = s[3 + a.C + c], T = s[3 + 2 * a.C + c];
      const double fp = S - tp, fn = T - tp;
      const double A = (1.0 + b2) * tp + a.smooth, D = (1.0 + b2) * tp + b2 * fn + fp + a.smooth;
      coef[2 + 2 * c] = A;
      coef[3 + 2 * c] = D;
      mean += A / D;
    }
    dice = 1.0 - mean / a.C;
  }
  loss[0] = (float)(bad ? s[1] : main + dice);
  loss[1] = (float)(bad ? s[1] : main);
  loss[2] = (float)dice;
}

// dout[b][c][p] = gscale * d(total)/dx_c
__global__ __launch_bounds__(256) void mc_loss_bwd_kernel(McArgs a, const double* coef, const float* gscale,
                                                          float* dout) {
  const long total = (long)a.B * a.P;
  const float g = gscale ? gscale[0] : 1.f;
  const float inv_w = (float)(1.0 / coef[0]), inv_n = (float)(1.0 / coef[1]);
  const float poison = 0.f * inv_n;  // NaN when an invalid target poisoned the sums, else 0
  const double b2 = (double)a.beta * a.beta;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    float x[kMaxC], lse;
    softmax_pixel(a, i, x, lse);
    float pr[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) pr[c] = c < a.C ? expf(x[c] - lse) : 0.f;
    const long t = (a.tgt && a.focal != 2) ? a.tgt[i] : -1;
    const bool valid = t != a.ignore && t >= 0 && t < a.C;
    const float wt = valid ? (a.cls_w ? a.cls_w[t] : 1.f) : 0.f;
    // main loss: dL/dx_c = k * (p_c - [c == t])
    float k = 0.f;
    if (valid) {
      if (a.focal == 0) {
        k = wt * inv_w;
      } else {
        float xt = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
          if (c == t) xt = x[c];
        const float logpt = -(wt * (lse - xt));
        const float pt = expf(logpt);
        const float al = a.alpha >= 0.f ? a.alpha : 1.f;
        // L = -al (1-pt)^gm logpt ; dL/dlogpt = al [gm (1-pt)^(gm-1) pt logpt - (1-pt)^gm]
        const float om = 1.f - pt;
        // gm = 0: (1-pt)^0 is constant, its term is 0 (torch's pow backward) -- not 0 * 0^-1 = NaN at pt == 1
        const float dpow = a.gamma == 0.f ? 0.f : a.gamma * powf(om, a.gamma - 1.f);
        const float dldl = al * (dpow * pt * logpt - powf(om, a.gamma));
        k = -dldl * wt * inv_n;  // dlogpt/dx_c = -wt (p_c - [c==t])
      }
    }
    float d[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) d[c] = k * (pr[c] - (c == t ? 1.f : 0.f)) + poison;
    if (a.dice_t) {
      const float* tt = a.dice_t + i * a.ct;
      float gp[kMaxC], dot = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        gp[c] = 0.f;
        if (c < a.C) {
          const double A = coef[2 + 2 * c], D = coef[3 + 2 * c];
          // d score_c / d p_c = ((1+b2) t D - A) / D^2   (D = b2 T + S + s)
          gp[c] = (float)(-((1.0 + b2) * tt[c] * D - A) / (D * D) / a.C);
          dot += gp[c] * pr[c];
        }
      }
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) d[c] += pr[c] * (gp[c] - dot);
    }
    const long b = i / a.P, p = i - b * a.P;
    float* o = dout + b * a.C * a.P + p;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < a.C) o[(long)c * a.P] = g * d[c];
  }
}

// ------------------------------------------------------------------------------------------
// Multiclass confusion histogram: hist[t][pred] (+)= 1 with pred = argmax_c (first maximum, as
// torch.max) and row t clamped to C for targets outside [0, C) (ignore / void pixels still count in
// pixel_accuracy's total and in the predicted-class union of mean_iou).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mc_confusion_kernel(const float* out, const int64_t* tgt, int B, int C, long P,
                                                           unsigned long long* hist) {
  __shared__ unsigned int h[(kMaxC + 1) * kMaxC];
  const int nb = (C + 1) * C;
  for (int j = threadIdx.x; j < nb; j += blockDim.x) h[j] = 0;
  __syncthreads();
  const long total = (long)B * P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / P, p = i - b * P;
    const float* base = out + b * C * P + p;
    float m = base[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
      const float v = base[(long)c * P];
      if (v > m) {
        m = v;
        am = c;
      }
    }
    const long t = tgt[i];
    const int row = (t >= 0 && t < C) ? (int)t : C;
    atomicAdd(&h[row * C + am], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < nb; j += blockDim.x)
    if (h[j]) atomicAdd(&hist[j], (unsigned long long)h[j]);
}

inline int grid_of(long n, int per = 256, int cap = 65535 * 4) {
  long g = (n + per - 1) / per;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

static McArgs mc_args(const float* out, const int64_t* tgt, int B, int C, long P, const float* cls_w, long ignore,
                      int focal, float alpha, float gamma, const float* dice_t, int ct, float beta, float smooth) {
  McArgs a{};
  a.out = out; a.tgt = tgt; a.cls_w = cls_w; a.dice_t = dice_t; a.B = B; a.C = C; a.ct = ct; a.P = P;
  a.ignore = ignore; a.focal = focal; a.alpha = alpha; a.gamma = gamma; a.beta = beta; a.smooth = smooth;
  return a;
}

static int mc_blocks(int B, long P) { return grid_of((long)B * P, 256, 1024); }

// workspace: per-block partials + fp64 coefficients
UNETSEG_API size_t unetseg_mc_loss_workspace(int B, int C, long P) {
  return (size_t)mc_blocks(B, P) * (3 + 3 * C) * sizeof(float) + (2 + 2 * kMaxC) * sizeof(double) + 64;
}

// loss fp32[3] = (total, main, Dice); focal selects the main term: 0 CE, 1 Focal, 2 none (Dice only,
// tgt may be NULL).  Fills the workspace's coefficients for the backward.
// cls_w [C] may be NULL; dice_t float [B][P][ct] (one-hot, ct >= C) may be NULL (no Dice term);
// alpha < 0 means Focal's alpha=None.
UNETSEG_API int unetseg_mc_loss_fwd(const float* out, const int64_t* tgt, int B, int C, long P, const float* cls_w,
                                    long ignore_index, int focal, float alpha, float gamma, const float* dice_t, int ct,
                                    float beta, float smooth, void* ws, size_t ws_bytes, float* loss, void* stream) {
  US_CHECK_ARG(out && (tgt || focal == 2) && ws && loss && B > 0 && P > 0 && C >= 1 && C <= kMaxC && focal >= 0 &&
                   focal <= 2, "mc_loss_fwd: bad args (C=%d, kind %d)", C, focal);
  US_CHECK_ARG(!dice_t || ct >= C, "mc_loss_fwd: dice target has %d < %d channels", ct, C);
  US_CHECK_ARG(ws_bytes >= unetseg_mc_loss_workspace(B, C, P), "mc_loss_fwd: workspace too small");
  const int G = mc_blocks(B, P);
  float* part = (float*)ws;
  double* coef = (double*)(((uintptr_t)(part + (size_t)G * (3 + 3 * C)) + 15) & ~(uintptr_t)15);
  McArgs a = mc_args(out, tgt, B, C, P, cls_w, ignore_index, focal, alpha, gamma, dice_t, ct, beta, smooth);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_loss_partial_kernel, dim3(G), dim3(256), 0, st, a, part, G);
  hipLaunchKernelGGL(mc_loss_finalize_kernel, dim3(1), dim3(128), 0, st, a, part, G, loss, coef);
  US_LAUNCH_CHECK("mc_loss_fwd");
  return 0;
}

// dout fp32 [B][C][P] = gscale[0] (device scalar, NULL = 1) * d total / d out, from the workspace
// filled by the matching unetseg_mc_loss_fwd
UNETSEG_API int unetseg_mc_loss_bwd(const float* out, const int64_t* tgt, int B, int C, long P, const float* cls_w,
                                    long ignore_index, int focal, float alpha, float gamma, const float* dice_t, int ct,
                                    float beta, float smooth, const void* ws, const float* gscale, float* dout,
                                    void* stream) {
  US_CHECK_ARG(out && (tgt || focal == 2) && ws && dout && C >= 1 && C <= kMaxC, "mc_loss_bwd: bad args");
  const int G = mc_blocks(B, P);
  const float* part = (const float*)ws;
  const double* coef = (const double*)(((uintptr_t)(part + (size_t)G * (3 + 3 * C)) + 15) & ~(uintptr_t)15);
  McArgs a = mc_args(out, tgt, B, C, P, cls_w, ignore_index, focal, alpha, gamma, dice_t, ct, beta, smooth);
  hipLaunchKernelGGL(mc_loss_bwd_kernel, dim3(grid_of((long)B * P)), dim3(256), 0, (hipStream_t)stream, a, coef,
                     gscale, dout);
  US_LAUNCH_CHECK("mc_loss_bwd");
  return 0;
}

// hist u64 [(C+1)][C] += confusion of argmax(out) vs tgt (rows: target class, row C = any other value)
UNETSEG_API int unetseg_mc_confusion(const float* out, const int64_t* tgt, int B, int C, long P,
                                     unsigned long long* hist, void* stream) {
  US_CHECK_ARG(out && tgt && hist && C >= 1 && C <= kMaxC, "mc_confusion: bad args (C=%d)", C);
  hipLaunchKernelGGL(mc_confusion_kernel, dim3(grid_of((long)B * P, 256, 2048)), dim3(256), 0, (hipStream_t)stream, out,
                     tgt, B, C, P, hist);
  US_LAUNCH_CHECK("mc_confusion");
  return 0;
}
