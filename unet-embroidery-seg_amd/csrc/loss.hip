// Binary-segmentation loss and metric kernels of the U-Net hot path (Adam: optim.hip; the
// classification head and its cross entropy: cls_head.hip).
//
//   Lovasz hinge   model/unet_training.py:219-280  (per-image sort desc, Jaccard grad, dot)
//   BCE w/ logits  model/unet_training.py:205-216, utils/train_and_eval.py:155-182
//   2-class->1     utils/train_and_eval.py:106-113 (z = o1 - o0, fused into the loss kernels)
//   confusion      utils/train_and_eval.py:116-152, train.py:330-340
//
// The Lovasz sort is a segmented, stable LSD radix sort (4 x 8-bit passes) on 32-bit keys that
// order the hinge errors descending; ties keep ascending pixel order (the reference's
// torch.sort is not stable, so only the loss VALUE is tie-order independent).  The sort kernels live
// in radix_sort.h, shared with the Lovasz-softmax (lovasz_softmax.hip).
#include "elem_util.h"
#include "radix_sort.h"

namespace {

// logits source: planar fp32 [B][nch][P]; nch==2 -> z = o1 - o0, nch==1 -> z = o0
__device__ __forceinline__ float load_z(const float* out, int nch, int b, long P, long i) {
  const float* base = out + (long)b * nch * P;
  // both loads unconditional (a load under the nch branch was waited on inside it)
  const float o0 = base[i], o1 = base[nch == 2 ? P + i : i];
  return nch == 2 ? o1 - o0 : o0;
}

// has_ignore: pixels whose target is `ignore` get error -inf and label 0, so they sort after every
// valid pixel and contribute to neither the loss, the gradient nor the Jaccard counts of the valid
// prefix: the per-image Lovasz over the valid pixels (model/unet_training.py:268-274)
__global__ void lovasz_keygen_kernel(const float* out, int nch, const int64_t* tgt, int B, long P, uint32_t* keys,
                                     uint32_t* vals, int has_ignore, long ignore) {
  const long total = (long)B * P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / P);
    const long px = i - (long)b * P;
    const float z = load_z(out, nch, b, P, px);
    const int64_t tv = tgt[i];
    const bool ign = has_ignore && tv == ignore;
    const uint32_t y = (!ign && tv == 1) ? 1u : 0u;
    const float e = ign ? -INFINITY : 1.0f - z * (2.0f * (float)y - 1.0f);
    keys[i] = desc_key(e);
    vals[i] = (uint32_t)px | (y << 31);
  }
}

// per chunk: Jaccard gradient over the sorted labels, loss partial = sum relu(e)*g,
// dz[pixel] = g*[e>0]*(-(2y-1))/B.  256 threads x 16 consecutive sorted keys.
__global__ void lovasz_chunk_kernel(const uint32_t* keys, const uint32_t* vals, long P, int T, const uint32_t* cnt,
                                    float inv_b, float* gz, float* part) {
  __shared__ uint32_t wsum[4];
  __shared__ double sred[16];
  const int t = blockIdx.x, b = blockIdx.y;
  const uint32_t* cb = cnt + (long)b * T;
  uint32_t G = 0, before = 0;
  for (int j = 0; j < T; ++j) {
    const uint32_t c = cb[j];
    G += c;
    if (j < t) before += c;
  }
  const long lo = (long)t * kTile + threadIdx.x * 16;
  const long hi = min(P, lo + 16);
  const uint32_t* k = keys + (long)b * P;
  const uint32_t* v = vals + (long)b * P;
  uint32_t vv[16], kk[16];
  uint32_t mine = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long i = lo + e;
    vv[e] = i < hi ? v[i] : 0u;
    kk[e] = i < hi ? k[i] : 0u;
    mine += vv[e] >> 31;
  }
  // exclusive scan of `mine` over the block
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  uint32_t woff = 0;
  for (int w = 0; w < wid; ++w) woff += wsum[w];
  uint32_t cp = before + woff + incl - mine;  // positives strictly before lo
  const float Gf = (float)G;
  float jprev;
  if (lo == 0) {
    jprev = 0.f;
  } else {
    const float cn = (float)(lo - cp);
    jprev = 1.0f - (Gf - (float)cp) / (Gf + cn);
  }
  double loss = 0.0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long i = lo + e;
    if (i < hi) {
      const uint32_t y = vv[e] >> 31;
      cp += y;
      const float cn = (float)(i + 1 - cp);
      const float j = 1.0f - (Gf - (float)cp) / (Gf + cn);
      const float g = j - jprev;
      jprev = j;
      const float err = key_to_float(kk[e]);
      if (err > 0.f) loss += (double)err * (double)g;
      gz[(long)b * P + (vv[e] & 0x7fffffffu)] = err > 0.f ? g * (y ? -inv_b : inv_b) : 0.f;
    }
  }
  loss = block_sum(loss, sred);
  if (threadIdx.x == 0) part[(long)b * T + t] = (float)loss;
}

// loss = mean_b sum_t part[b][t]  (fixed order)
__global__ void lovasz_final_kernel(const float* part, int B, int T, float* loss) {
  __shared__ double sred[16];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    double sb = 0.0;
    for (int t = 0; t < T; ++t) sb += part[(long)b * T + t];
    s += sb;
  }
  s = block_sum(s, sred);
  if (threadIdx.x == 0) loss[0] = B > 0 ? (float)(s / B) : 0.f;
}

__global__ void mean_kernel(const float* x, int n, float* out) {
  __shared__ double sred[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
  s = block_sum(s, sred);
  if (threadIdx.x == 0) out[0] = n > 0 ? (float)(s / n) : 0.f;
}

// d_out for a per-pixel dz: nch==2 -> d o1 = +g, d o0 = -g ; scale = upstream[0] * factor
__global__ void dz_to_dout_kernel(const float* gz, int B, long P, int nch, const float* upstream, float factor,
                                  float* dout) {
  const float sc = (upstream ? upstream[0] : 1.f) * factor;
  const long total = (long)B * P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / P);
    const long px = i - (long)b * P;
    const float g = gz[i] * sc;
    if (nch == 2) {
      dout[((long)b * 2 + 1) * P + px] = g;
      dout[((long)b * 2) * P + px] = -g;
    } else {
      dout[(long)b * P + px] = g;
    }
  }
}

// BCE with logits (PyTorch formulation), per-block partial sums; grad dz stored unscaled (1/count applied)
__global__ void bce_kernel(const float* out, int nch, const int64_t* tgt, int B, long P, const float* pos_weight,
                           float* gz, float* part) {
  __shared__ double sred[16];
  const long total = (long)B * P;
  const float pw = pos_weight ? pos_weight[0] : 1.0f;
  double s = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / P);
    const long px = i - (long)b * P;
    const float z = load_z(out, nch, b, P, px);
    const float y = tgt[i] == 1 ? 1.f : 0.f;
    const float lw = (pw - 1.f) * y + 1.f;
    const float sp = log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
    s += (double)((1.f - y) * z + lw * sp);
    const float sig_neg = 1.f / (1.f + expf(z));  // sigmoid(-z)
    if (gz) gz[i] = ((1.f - y) - lw * sig_neg) / (float)total;
  }
  s = block_sum(s, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = (float)(s / (double)total);
}

__global__ void sum_kernel(const float* x, int n, float* out) {
  __shared__ double sred[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
  s = block_sum(s, sred);
  if (threadIdx.x == 0) out[0] = (float)s;
}

// Binary loss over the pixels whose target is not ignore_index (utils/train_and_eval.py:169-176):
// kind 0 = BCE-with-logits (pos_weight); kind 1 = the reference's Lovasz on the FLATTENED valid
// pixels: lovasz_hinge_loss then iterates over single pixels (model/unet_training.py:267-276), so its
// value is the mean hinge relu(1 - z(2y-1)) with gradient -(2y-1)[e > 0].  gz gets the per-pixel
// gradient numerator (0 on ignored pixels); part [2][G] = (loss sum, valid count) per block.
__global__ void masked_loss_kernel(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore, int kind,
                                   const float* pos_weight, float* gz, float* part) {
  __shared__ double sred[16];
  const long total = (long)B * P;
  const float pw = pos_weight ? pos_weight[0] : 1.0f;
  double s = 0.0, n = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / P);
    const long px = i - (long)b * P;
    const int64_t t = tgt[i];
    float g = 0.f;
    if (t != ignore) {
      const float z = load_z(out, nch, b, P, px);
      const float y = t == 1 ? 1.f : 0.f;
      if (kind == 0) {
        const float lw = (pw - 1.f) * y + 1.f;
        const float sp = log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
        s += (double)((1.f - y) * z + lw * sp);
        g = (1.f - y) - lw / (1.f + expf(z));
      } else {
        const float sg = 2.f * y - 1.f, e = 1.f - z * sg;
        s += (double)fmaxf(e, 0.f);
        g = e > 0.f ? -sg : 0.f;
      }
      n += 1.0;
    }
    gz[i] = g;
  }
  s = block_sum(s, sred);
  n = block_sum(n, sred);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = (float)s;
    part[gridDim.x + blockIdx.x] = (float)n;
  }
}

// loss = sum / count (count 0: NaN for BCE, as a mean over nothing; 0 for the Lovasz branch, whose
// empty loss list returns logits.sum() * 0); inv = 1 / count (0 if none)
__global__ void masked_finalize_kernel(const float* part, int G, int kind, float* loss, float* inv) {
  __shared__ double sred[16];
  double s = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < G; i += blockDim.x) {
    s += part[i];
    n += part[G + i];
  }
  s = block_sum(s, sred);
  n = block_sum(n, sred);
  if (threadIdx.x == 0) {
    loss[0] = n > 0.0 ? (float)(s / n) : (kind == 0 ? __builtin_nanf("") : 0.f);
    inv[0] = n > 0.0 ? (float)(1.0 / n) : 0.f;
  }
}

__global__ void scale_by_kernel(float* x, long n, const float* s) {
  const float f = s[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) x[i] *= f;
}

// confusion counts: mode 2 -> pred = o1 > o0 (argmax, tie -> 0); mode 1 -> pred = sigmoid(o0) > 0.5;
// pixels whose target equals `ignore` are skipped when has_ignore (utils/train_and_eval.py:125-126)
__global__ void confusion_kernel(const float* out, int nch, const int64_t* tgt, int B, long P,
                                 unsigned long long* conf, int has_ignore, long ignore) {
  __shared__ unsigned long long sc[4][16];
  const long total = (long)B * P;
  unsigned long long c[4] = {0, 0, 0, 0};
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    if (has_ignore && tgt[i] == ignore) continue;
    const int b = (int)(i / P);
    const long px = i - (long)b * P;
    bool pred;
    if (nch == 2) {
      const float* base = out + (long)b * 2 * P;
      pred = base[P + px] > base[px];
    } else {
      const float z = out[(long)b * P + px];
      pred = 1.0f / (1.0f + expf(-z)) > 0.5f;
    }
    const bool t = tgt[i] == 1;
    c[pred && t ? 0 : (pred ? 1 : (t ? 2 : 3))] += 1;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned long long v = c[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sc[k][wid] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) v += sc[threadIdx.x][w];
    atomicAdd(&conf[threadIdx.x], v);
  }
}

// multiply a per-element gradient buffer by a device scalar: out = g * (s1[0]*a1 + s2[0]*a2)
__global__ void scale_grad_kernel(const float* g, long n, const float* s1, float a1, const float* s2, float a2,
                                  float* out) {
  const float sc = (s1 ? s1[0] * a1 : 0.f) + (s2 ? s2[0] * a2 : 0.f);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = g[i] * sc;
}

constexpr int kLossGrid = 8192;  // block cap of the loss kernels (their partial buffers are sized by it)

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

UNETSEG_API size_t unetseg_lovasz_workspace(int B, long P) {
  const long T = (P + kTile - 1) / kTile;
  return (size_t)B * P * 4 * sizeof(uint32_t) + (size_t)B * 256 * T * sizeof(uint32_t) +
         (size_t)B * T * (sizeof(uint32_t) + sizeof(float)) + 256;
}

// Lovasz hinge (per-image mean).  out: planar fp32 [B][nch][P] logits (nch 2 -> z = o1-o0);
// tgt int64 [B][P] (==1 is foreground).  Writes loss[0] and gz [B][P] = dloss/dz (already /B).
static int lovasz_impl(const float* out, int nch, const int64_t* tgt, int B, long P, int has_ignore, long ignore,
                       void* ws, size_t ws_bytes, float* gz, float* loss, void* stream);

UNETSEG_API int unetseg_lovasz_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, void* ws,
                                   size_t ws_bytes, float* gz, float* loss, void* stream) {
  return lovasz_impl(out, nch, tgt, B, P, 0, 0L, ws, ws_bytes, gz, loss, stream);
}

// per-image Lovasz over the pixels whose target is not ignore_index (lovasz_hinge_loss(..., ignore_index))
UNETSEG_API int unetseg_lovasz_fwd_masked(const float* out, int nch, const int64_t* tgt, int B, long P,
                                          long ignore_index, void* ws, size_t ws_bytes, float* gz, float* loss,
                                          void* stream) {
  return lovasz_impl(out, nch, tgt, B, P, 1, ignore_index, ws, ws_bytes, gz, loss, stream);
}

static int lovasz_impl(const float* out, int nch, const int64_t* tgt, int B, long P, int has_ignore, long ignore,
                       void* ws, size_t ws_bytes, float* gz, float* loss, void* stream) {
  US_CHECK_ARG(out && tgt && ws && gz && loss, "lovasz_fwd: null pointer");
  US_CHECK_ARG(nch == 1 || nch == 2, "lovasz_fwd: nch must be 1 or 2");
  US_CHECK_ARG(P < 0x80000000L, "lovasz_fwd: too many pixels per image");
  US_CHECK_ARG(ws_bytes >= unetseg_lovasz_workspace(B, P), "lovasz_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || P == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), st);
    return 0;
  }
  const int T = (int)((P + kTile - 1) / kTile);
  uint32_t* k0 = (uint32_t*)ws;
  uint32_t* v0 = k0 + (long)B * P;
  uint32_t* k1 = v0 + (long)B * P;
  uint32_t* v1 = k1 + (long)B * P;
  uint32_t* hist = v1 + (long)B * P;
  uint32_t* cnt = hist + (long)B * 256 * T;
  float* part = (float*)(cnt + (long)B * T);
  hipLaunchKernelGGL(lovasz_keygen_kernel, dim3(grid_for((long)B * P, kLossGrid)), dim3(256), 0, st, out, nch, tgt, B,
                     P, k0, v0, has_ignore, ignore);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = pass * 8;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(T, B), dim3(256), 0, st, k0, P, T, shift, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(B), dim3(1024), 0, st, hist, T);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(T, B), dim3(256), 0, st, k0, v0, k1, v1, P, T, shift, hist);
    uint32_t* t;
    t = k0; k0 = k1; k1 = t;
    t = v0; v0 = v1; v1 = t;
  }
  hipLaunchKernelGGL(lovasz_count_kernel, dim3(T, B), dim3(256), 0, st, v0, P, T, cnt);
  hipLaunchKernelGGL(lovasz_chunk_kernel, dim3(T, B), dim3(256), 0, st, k0, v0, P, T, cnt, 1.0f / (float)B, gz, part);
  hipLaunchKernelGGL(lovasz_final_kernel, dim3(1), dim3(64), 0, st, part, B, T, loss);
  US_LAUNCH_CHECK("lovasz_fwd");
  return 0;
}

UNETSEG_API size_t unetseg_bce_workspace(int B, long P) {
  return (size_t)grid_for((long)B * P, kLossGrid) * sizeof(float) + 256;
}

// BCE-with-logits mean loss; gz (may be NULL) = dloss/dz (already /count); pos_weight fp32 scalar or NULL
UNETSEG_API int unetseg_bce_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, const float* pos_weight,
                                void* ws, size_t ws_bytes, float* gz, float* loss, void* stream) {
  US_CHECK_ARG(out && tgt && ws && loss, "bce_fwd: null pointer");  // gz may be NULL (no gradient)
  US_CHECK_ARG(nch == 1 || nch == 2, "bce_fwd: nch %d must be 1 or 2", nch);
  US_CHECK_ARG(B > 0 && P > 0, "bce_fwd: empty batch");
  US_CHECK_ARG(ws_bytes >= unetseg_bce_workspace(B, P), "bce_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int G = grid_for((long)B * P, kLossGrid);
  hipLaunchKernelGGL(bce_kernel, dim3(G), dim3(256), 0, st, out, nch, tgt, B, P, pos_weight, gz, (float*)ws);
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, G, loss);
  US_LAUNCH_CHECK("bce_fwd");
  return 0;
}

// dout = gz * (s1[0]*a1 + s2[0]*a2) scattered to the planar logits (nch 2: +/-)
UNETSEG_API int unetseg_dz_to_dout(const float* gz, int B, long P, int nch, const float* s1, float a1, const float* s2,
                                   float a2, float* scratch, float* dout, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)B * P;
  hipLaunchKernelGGL(scale_grad_kernel, dim3(grid_for(n, kLossGrid)), dim3(256), 0, st, gz, n, s1, a1, s2, a2, scratch);
  hipLaunchKernelGGL(dz_to_dout_kernel, dim3(grid_for(n, kLossGrid)), dim3(256), 0, st, scratch, B, P, nch,
                     (const float*)nullptr, 1.f, dout);
  US_LAUNCH_CHECK("dz_to_dout");
  return 0;
}

// conf (uint64[4]) += (tp, fp, fn, tn)
UNETSEG_API int unetseg_confusion(const float* out, int nch, const int64_t* tgt, int B, long P, unsigned long long* conf,
                                  void* stream) {
  hipLaunchKernelGGL(confusion_kernel, dim3(grid_for((long)B * P, 2048)), dim3(256), 0, (hipStream_t)stream, out, nch,
                     tgt, B, P, conf, 0, 0L);
  US_LAUNCH_CHECK("confusion");
  return 0;
}

// out = g * (s1[0]*a1 + s2[0]*a2)
UNETSEG_API int unetseg_scale_grad(const float* g, long n, const float* s1, float a1, const float* s2, float a2,
                                   float* out, void* stream) {
  hipLaunchKernelGGL(scale_grad_kernel, dim3(grid_for(n, kLossGrid)), dim3(256), 0, (hipStream_t)stream, g, n, s1, a1,
                     s2, a2, out);
  US_LAUNCH_CHECK("scale_grad");
  return 0;
}

// confusion counts over the pixels whose target is not ignore_index
UNETSEG_API int unetseg_confusion_masked(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index,
                                         unsigned long long* conf, void* stream) {
  US_CHECK_ARG(out && tgt && conf && (nch == 1 || nch == 2), "confusion_masked: bad args");
  hipLaunchKernelGGL(confusion_kernel, dim3(grid_for((long)B * P, 2048)), dim3(256), 0, (hipStream_t)stream, out, nch,
                     tgt, B, P, conf, 1, ignore_index);
  US_LAUNCH_CHECK("confusion_masked");
  return 0;
}

UNETSEG_API size_t unetseg_masked_loss_workspace(int B, long P) {
  return (size_t)2 * grid_for((long)B * P, kLossGrid) * sizeof(float) + 256;
}

// binary loss over the non-ignored pixels; kind 0 BCE (pos_weight may be NULL), 1 Lovasz (flattened,
// see masked_loss_kernel).  gz [B][P] = dloss/dz (already / count); loss fp32 scalar
UNETSEG_API int unetseg_masked_loss_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index,
                                        int kind, const float* pos_weight, void* ws, size_t ws_bytes, float* gz,
                                        float* loss, void* stream) {
  US_CHECK_ARG(out && tgt && gz && loss && ws && (kind == 0 || kind == 1), "masked_loss_fwd: bad args");
  US_CHECK_ARG(ws_bytes >= unetseg_masked_loss_workspace(B, P), "masked_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int G = grid_for((long)B * P, kLossGrid);
  float* part = (float*)ws;
  float* inv = part + 2 * G;
  hipLaunchKernelGGL(masked_loss_kernel, dim3(G), dim3(256), 0, st, out, nch, tgt, B, P, ignore_index, kind, pos_weight,
                     gz, part);
  hipLaunchKernelGGL(masked_finalize_kernel, dim3(1), dim3(256), 0, st, part, G, kind, loss, inv);
  hipLaunchKernelGGL(scale_by_kernel, dim3(G), dim3(256), 0, st, gz, (long)B * P, inv);
  US_LAUNCH_CHECK("masked_loss_fwd");
  return 0;
}
