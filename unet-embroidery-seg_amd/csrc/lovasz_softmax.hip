// Lovasz-softmax loss of the multiclass task (Berman, Rannen Triki, Blaschko, CVPR 2018, Alg. 1 with
// the class-averaged softmax errors): the multiclass form of the Lovasz hinge in loss.hip, on the same
// segmented stable radix sort (radix_sort.h).
//
// Logits fp32 planar [B][C][P], labels int64 [B][P]; a pixel whose label is ignore_index or lies
// outside [0, C) is invalid.  With p = softmax(logits), for every class c present among a segment's
// valid labels: fg = [label == c], e = |fg - p_c| over the valid pixels, sorted descending,
// J_k = 1 - (G - cumsum(fg)_k) / (G + cumsum(1 - fg)_k), g_k = J_k - J_{k-1} (J_0 = 0),
// loss_c = sum_k e_(k) g_k; the segment's loss is the mean over its present classes (0 if it has no
// valid pixel).  per_image: one segment per image and the mean over the B images (an image without a
// valid pixel counts as 0); else one segment of all B*P pixels.
//
// Sort segments: (image b, class c) -> segment b*C + c of P keys, which is the [B][C][P] layout of the
// logits themselves; in batch mode class c -> segment c of B*P keys (index b*P + px).  Equal errors
// keep ascending index order.  Invalid pixels get a key that sorts after every valid one and the
// chunk kernel gates on that key: without the gate the sorted-last invalid positions would receive a
// non-zero g (the count of negatives keeps growing).
//
// Workspace (one caller buffer), with N = B*C*P, S segments of L keys and T = ceil(L / 4096) tiles
// (per image S = B*C, L = P; batch S = C, L = B*P):
//   16 N (keys and values, double-buffered) + 4 S T (256 + 2) (digit histograms, chunk counts, chunk
//   partials) + 8 S (per-segment positives and weight) + 256 bytes.
// dL/dp is written into the caller's dlogits buffer and turned into dL/dlogits in place.
// No float atomics: every reduction has a fixed order, two runs give the same bits.
#include "elem_util.h"
#include "radix_sort.h"

namespace {

constexpr uint32_t kInvalidKey = 0xffffffffu;   // after desc_key(e) <= 0x7fffffff of every e >= 0

// one pass over the logits: softmax (max-subtracted; exp and the normalisation in fp64, so the error
// that is rounded into the 32-bit key is the correctly rounded one and near-equal errors rank as they
// do in exact arithmetic), then per class the key desc_key(|fg - p_c|) and the value word
// index | fg << 31 into the class's segment
__global__ __launch_bounds__(256) void lsm_keygen_kernel(const float* out, const int64_t* tgt, int B, int C, long P,
                                                         long ignore, int per_image, uint32_t* keys, uint32_t* vals) {
  const long total = (long)B * P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / P, px = i - b * P;
    const float* base = out + b * C * P + px;
    float x[kMaxC];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        x[c] = base[(long)c * P];
        m = fmaxf(m, x[c]);
      }
    double ex[kMaxC];
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        ex[c] = exp((double)x[c] - (double)m);
        s += ex[c];
      }
    const double inv = 1.0 / s;
    const long t = tgt[i];
    const bool valid = t != ignore && t >= 0 && t < C;
    const uint32_t idx = (uint32_t)(per_image ? px : i);
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        const bool fg = valid && c == t;
        const double p = ex[c] * inv;
        const float e = (float)fabs(fg ? 1.0 - p : p);
        const long a = per_image ? (b * C + c) * P + px : (long)c * total + i;
        keys[a] = valid ? desc_key(e) : kInvalidKey;
        vals[a] = idx | ((fg ? 1u : 0u) << 31);
      }
  }
}

// per group (image, or the whole batch): positives G of each class segment, the number of present
// classes and the segment's weight w = 1 / (n_present * n_groups), 0 for an absent class
__global__ __launch_bounds__(256) void lsm_segstat_kernel(const uint32_t* cnt, int C, int T, int n_groups,
                                                          uint32_t* gseg, float* wseg) {
  __shared__ uint32_t sred[16];
  __shared__ uint32_t G[kMaxC];
  const int grp = blockIdx.x;
  for (int c = 0; c < C; ++c) {
    const uint32_t* cb = cnt + ((long)grp * C + c) * T;
    uint32_t s = 0;
    for (int j = threadIdx.x; j < T; j += 256) s += cb[j];
    s = block_sum(s, sred);
    if (threadIdx.x == 0) G[c] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    int np = 0;
    for (int c = 0; c < C; ++c) np += G[c] > 0 ? 1 : 0;
    const uint32_t g = G[threadIdx.x];
    gseg[(long)grp * C + threadIdx.x] = g;
    wseg[(long)grp * C + threadIdx.x] = g > 0 ? 1.0f / ((float)np * (float)n_groups) : 0.f;
  }
}

// per chunk of 4096 sorted keys (256 threads x 16 consecutive): Jaccard gradient over the sorted
// labels, loss partial = sum e * g over the valid positions (fp64), dp[pixel] = w g (fg ? -1 : +1),
// exactly 0 at invalid positions and for an absent class.  With I = G - (positives before k) and
// U = G + (negatives before k), g_k = J_k - J_{k-1} is 1 / U at a positive and I / (U (U + 1)) at a
// negative: the same number without the cancellation of two Jaccard values that differ by ~1 / L.
__global__ __launch_bounds__(256) void lsm_chunk_kernel(const uint32_t* keys, const uint32_t* vals, long L, int T,
                                                        int C, long P, int per_image, const uint32_t* cnt,
                                                        const uint32_t* gseg, const float* wseg, float* dp,
                                                        float* part) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t ured[16];
  __shared__ double sred[16];
  const int t = blockIdx.x, sg = blockIdx.y;
  const uint32_t* cb = cnt + (long)sg * T;
  uint32_t bsum = 0;
  for (int j = threadIdx.x; j < t; j += 256) bsum += cb[j];
  const uint32_t before = block_sum(bsum, ured);
  const uint32_t G = gseg[sg];
  const float w = wseg[sg];
  const long lo = (long)t * kTile + threadIdx.x * 16;
  const long hi = min(L, lo + 16);
  const uint32_t* k = keys + (long)sg * L;
  const uint32_t* v = vals + (long)sg * L;
  uint32_t vv[16], kk[16];
  uint32_t mine = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long i = lo + e;
    vv[e] = i < hi ? v[i] : 0u;
    kk[e] = i < hi ? k[i] : kInvalidKey;
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
  for (int q = 0; q < wid; ++q) woff += wsum[q];
  uint32_t cp = before + woff + incl - mine;  // positives strictly before lo
  // dp is [B][C][P]: a per-image segment b*C + c is its own plane; in batch mode the index is b*P + px
  const int c = per_image ? 0 : sg;
  double loss = 0.0;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const long i = lo + e;
    if (i < hi) {
      const uint32_t y = vv[e] >> 31;
      const bool on = G > 0 && !(kk[e] >> 31);  // present class, valid position
      float d = 0.f;
      if (on) {
        const double U = (double)G + (double)(i - cp), I = (double)(G - cp);
        const double g = y ? 1.0 / U : I / (U * (U + 1.0));
        loss += (double)key_to_float(kk[e]) * g;
        d = (float)((double)w * g);
        if (y) d = -d;
      }
      cp += y;
      if (dp) {
        const uint32_t idx = vv[e] & 0x7fffffffu;
        long a;
        if (per_image) {
          a = (long)sg * P + idx;
        } else {
          const long b = idx / P;
          a = (b * C + c) * P + (idx - b * P);
        }
        dp[a] = d;
      }
    }
  }
  loss = block_sum(loss, sred);
  if (threadIdx.x == 0) part[(long)sg * T + t] = (float)loss;
}

// loss = sum_s w_s sum_t part[s][t] (fixed order: one wave per segment, lanes stride the chunks)
__global__ __launch_bounds__(256) void lsm_final_kernel(const float* part, const float* wseg, int S, int T,
                                                        float* loss) {
  __shared__ double sred[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double s = 0.0;
  for (int sg = wid; sg < S; sg += nw) {
    double sb = 0.0;
    for (int t = lane; t < T; t += 64) sb += (double)part[(long)sg * T + t];
    s += (double)wseg[sg] * wave_sum_d(sb);
  }
  s = block_sum(lane == 0 ? s : 0.0, sred);
  if (threadIdx.x == 0) loss[0] = (float)s;
}

// dl holds dL/dp [B][C][P]; in place dL/dlogit_k = p_k (dL/dp_k - sum_c dL/dp_c p_c) with p recomputed
// from the logits.  The normalisation and the dot product run in fp64 and each output is rounded
// once, so a pixel's C gradients sum to 0 within C roundings of its largest one; a pixel whose dL/dp
// are all 0 (invalid) gets exactly 0.
__global__ __launch_bounds__(256) void lsm_jacobian_kernel(const float* out, int B, int C, long P, float* dl) {
  const long total = (long)B * P;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / P, px = i - b * P;
    const float* base = out + b * C * P + px;
    float* o = dl + b * C * P + px;
    float x[kMaxC], d[kMaxC];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        x[c] = base[(long)c * P];
        d[c] = o[(long)c * P];
        m = fmaxf(m, x[c]);
      }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) {
        x[c] = expf(x[c] - m);
        s += (double)x[c];
      }
    const double inv = 1.0 / s;
    double dot = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) dot += (double)d[c] * ((double)x[c] * inv);
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) o[(long)c * P] = (float)(((double)x[c] * inv) * ((double)d[c] - dot));
  }
}

struct LsmShape {
  long S, L, T;  // segments, keys per segment, tiles per segment
};

LsmShape lsm_shape(int B, int C, long P, int per_image) {
  LsmShape s;
  s.S = per_image ? (long)B * C : C;
  s.L = per_image ? P : (long)B * P;
  s.T = (s.L + kTile - 1) / kTile;
  return s;
}

}  // namespace

UNETSEG_API size_t unetseg_lovasz_softmax_workspace(int B, int C, long P, int per_image) {
  if (B < 0 || C < 0 || P < 0) return 0;
  const LsmShape s = lsm_shape(B, C, P, per_image);
  return (size_t)B * C * P * 4 * sizeof(uint32_t) + (size_t)s.S * s.T * (256 + 2) * sizeof(uint32_t) +
         (size_t)s.S * (sizeof(uint32_t) + sizeof(float)) + 256;
}

// loss[0] = Lovasz-softmax of the fp32 planar logits out [B][C][P] against tgt int64 [B][P];
// dlogits (NULL: value only) fp32 [B][C][P] = d loss / d out for a unit upstream gradient
UNETSEG_API int unetseg_lovasz_softmax_fwd(const float* out, const int64_t* tgt, int B, int C, long P,
                                           long ignore_index, int per_image, void* ws, size_t ws_bytes,
                                           float* dlogits, float* loss, void* stream) {
  US_CHECK_ARG(C >= 2 && C <= kMaxC, "lovasz_softmax_fwd: C=%d must be in 2..%d", C, kMaxC);
  US_CHECK_ARG(out && tgt && loss, "lovasz_softmax_fwd: null pointer (out, tgt or loss)");
  US_CHECK_ARG(B >= 0 && P >= 0, "lovasz_softmax_fwd: negative size B=%d P=%ld", B, P);
  US_CHECK_ARG(P < 0x80000000L && (long)B * P < 0x80000000L,
               "lovasz_softmax_fwd: B*P = %d*%ld pixels do not fit the 31-bit index", B, P);
  US_CHECK_ARG((long)B * C <= 65535, "lovasz_softmax_fwd: B*C = %d*%d segments exceed the grid", B, C);
  US_CHECK_ARG(ws && ws_bytes >= unetseg_lovasz_softmax_workspace(B, C, P, per_image),
               "lovasz_softmax_fwd: workspace too small (%zu < %zu bytes)", ws_bytes,
               unetseg_lovasz_softmax_workspace(B, C, P, per_image));
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || P == 0) {
    (void)hipMemsetAsync(loss, 0, sizeof(float), st);
    return 0;
  }
  per_image = per_image ? 1 : 0;
  const LsmShape sh = lsm_shape(B, C, P, per_image);
  const int S = (int)sh.S, T = (int)sh.T;
  const long L = sh.L, N = (long)B * C * P;
  uint32_t* k0 = (uint32_t*)ws;
  uint32_t* v0 = k0 + N;
  uint32_t* k1 = v0 + N;
  uint32_t* v1 = k1 + N;
  uint32_t* hist = v1 + N;
  uint32_t* cnt = hist + (long)S * 256 * T;
  float* part = (float*)(cnt + (long)S * T);
  uint32_t* gseg = (uint32_t*)(part + (long)S * T);
  float* wseg = (float*)(gseg + S);
  hipLaunchKernelGGL(lsm_keygen_kernel, dim3(grid_for((long)B * P, 8192)), dim3(256), 0, st, out, tgt, B, C, P,
                     ignore_index, per_image, k0, v0);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = pass * 8;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(T, S), dim3(256), 0, st, k0, L, T, shift, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(S), dim3(1024), 0, st, hist, T);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(T, S), dim3(256), 0, st, k0, v0, k1, v1, L, T, shift, hist);
    uint32_t* t;
    t = k0; k0 = k1; k1 = t;
    t = v0; v0 = v1; v1 = t;
  }
  hipLaunchKernelGGL(lovasz_count_kernel, dim3(T, S), dim3(256), 0, st, v0, L, T, cnt);
  const int n_groups = per_image ? B : 1;
  hipLaunchKernelGGL(lsm_segstat_kernel, dim3(n_groups), dim3(256), 0, st, cnt, C, T, n_groups, gseg, wseg);
  hipLaunchKernelGGL(lsm_chunk_kernel, dim3(T, S), dim3(256), 0, st, k0, v0, L, T, C, P, per_image, cnt, gseg, wseg,
                     dlogits, part);
  hipLaunchKernelGGL(lsm_final_kernel, dim3(1), dim3(256), 0, st, part, wseg, S, T, loss);
  if (dlogits)
    hipLaunchKernelGGL(lsm_jacobian_kernel, dim3(grid_for((long)B * P, 8192)), dim3(256), 0, st, out, B, C, P, dlogits);
  US_LAUNCH_CHECK("lovasz_softmax_fwd");
  return 0;
}
