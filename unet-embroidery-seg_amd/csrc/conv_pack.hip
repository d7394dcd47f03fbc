// Conv weight packers: PyTorch's fp32 [K][C][R][S] into the images the conv kernels read -- one conv,
// all of a model's convs in one launch, and the ResNet stem's width-packed image -- with their C-ABI
// entry points.
#include "common.h"

namespace {

// fp32 [K][C][R][S] -> T [K][R][S][Cpad] (zero-padded channels) and optionally T [C][R][S][K]
template <typename T>
__global__ void pack_weights_kernel(const float* w, int K, int C, int R, int S, int Cpad, T* wk, T* wt) {
  const long total = (long)K * R * S * Cpad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const int c = (int)(t % Cpad); t /= Cpad;
    const int s = (int)(t % S); t /= S;
    const int r = (int)(t % R); t /= R;
    const int k = (int)t;
    float v = c < C ? w[(((long)k * C + c) * R + r) * S + s] : 0.f;
    wk[i] = (T)v;
    if (wt && c < C) wt[(((long)c * R + r) * S + s) * K + k] = (T)v;
  }
}

// Batched pack of many conv weights: one block per (16 output channels x CT input channels) tile of
// one conv (desc[i].start = its first tile; unetseg_pack_tiles gives a conv's tile count).  The fp32
// source of a tile is 16 contiguous runs of CT*taps floats ([K][C][R][S] keeps c and the taps of
// one k together), read with unit-stride coalesced loads into LDS; the wk image ([K][R][S][Cpad])
// and the transposed wt image ([C][R][S][K]) are then written from LDS, channel-contiguous and
// k-contiguous respectively.  CT = pow2 in [8, 256] with CT * taps <= 512, so the tile fits the
// static LDS array; the odd row pitch (513) keeps both LDS read patterns conflict-free.
constexpr int kPackK = 16;

__host__ __device__ inline int pack_ct(int taps) {
  int ct = 256;
  while (ct > 8 && ct * taps > 512) ct >>= 1;
  return ct;
}

template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const UnetsegPackDesc* desc, int n) {
  __shared__ float tile[kPackK][513];
  const long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {  // last desc with start <= b
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].start <= b) lo = mid; else hi = mid - 1;
  }
  const UnetsegPackDesc d = desc[lo];
  const int taps = d.R * d.S;
  const int CT = pack_ct(taps);
  const int lt = (int)(b - d.start);
  const int ctiles = (d.Cpad + CT - 1) / CT;
  const int kt = lt / ctiles, ct = lt - kt * ctiles;
  const int k0 = kt * kPackK, c0 = ct * CT;
  const int run = CT * taps;                           // floats per k row of the tile
  const int vrun = max(0, min(CT, d.C - c0)) * taps;   // of which exist in the source
  const int t = threadIdx.x;
  if ((d.C * taps) % 4 == 0 && vrun % 4 == 0) {  // 16-B loads (rows start 16-B aligned)
    // every load of the tile issued before the first LDS store: unconditional (absent rows / columns
    // read the source's first float4 and are zeroed after); a load under the lane condition was
    // waited on by itself, one round trip per loop iteration
    const int run4 = run >> 2;
    constexpr int NIT = kPackK * 512 / 4 / 256;  // run <= 512
    float4 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = t + it * 256;
      const int kl = i / run4, j = (i - kl * run4) * 4;
      const int k = k0 + kl;
      const bool ok = i < kPackK * run4 && k < d.K && j < vrun;
      const float4 x = *reinterpret_cast<const float4*>(ok ? d.w + ((long)k * d.C + c0) * taps + j : d.w);
      v[it] = ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = t + it * 256;
      if (i >= kPackK * run4) break;
      const int kl = i / run4, j = (i - kl * run4) * 4;
      tile[kl][j] = v[it].x;
      tile[kl][j + 1] = v[it].y;
      tile[kl][j + 2] = v[it].z;
      tile[kl][j + 3] = v[it].w;
    }
  } else {
    for (int i = t; i < kPackK * run; i += 256) {
      const int kl = i / run, j = i - kl * run;
      const int k = k0 + kl;
      tile[kl][j] = (k < d.K && j < vrun) ? d.w[((long)k * d.C + c0) * taps + j] : 0.f;
    }
  }
  __syncthreads();
  // wk[k][tap][c], c fastest, 4 channels per store (padding channels c in [C, Cpad) get the zeros
  // staged above)
  T* wk = reinterpret_cast<T*>(d.wk);
  if (d.Cpad % 4 == 0) {
    const int CT4 = CT >> 2;
    for (int i = t; i < kPackK * taps * CT4; i += 256) {
      const int c4 = i % CT4, rest = i / CT4;
      const int tap = rest % taps, kl = rest / taps;
      const int k = k0 + kl, c = c0 + c4 * 4;
      if (k >= d.K || c >= d.Cpad) continue;
      T o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)tile[kl][(c4 * 4 + e) * taps + tap];
      T* dst = wk + ((long)k * taps + tap) * d.Cpad + c;
      if (sizeof(T) == 2) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(o);
      else *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
    }
  } else {
    for (int i = t; i < kPackK * taps * CT; i += 256) {
      const int cl = i % CT, rest = i / CT;
      const int tap = rest % taps, kl = rest / taps;
      const int k = k0 + kl, c = c0 + cl;
      if (k < d.K && c < d.Cpad) wk[((long)k * taps + tap) * d.Cpad + c] = (T)tile[kl][cl * taps + tap];
    }
  }
  if (d.wt) {  // wt[c][tap][k], k fastest, 8 output channels per store; rows of Kld (>= K) elements
    T* wt = reinterpret_cast<T*>(d.wt);
    const int ldk = d.Kld > 0 ? d.Kld : d.K;
    if (d.K % 8 == 0 && ldk % 8 == 0) {
      constexpr int K8 = kPackK / 8;
      for (int i = t; i < K8 * taps * CT; i += 256) {
        const int k8 = i % K8, rest = i / K8;
        const int tap = rest % taps, cl = rest / taps;
        const int k = k0 + k8 * 8, c = c0 + cl;
        if (k >= d.K || c >= d.C) continue;
        T o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (T)tile[k8 * 8 + e][cl * taps + tap];
        T* dst = wt + ((long)c * taps + tap) * ldk + k;
        if (sizeof(T) == 2) {
          *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
        } else {
          reinterpret_cast<uint4*>(dst)[0] = reinterpret_cast<const uint4*>(o)[0];
          reinterpret_cast<uint4*>(dst)[1] = reinterpret_cast<const uint4*>(o)[1];
        }
      }
    } else {
      for (int i = t; i < kPackK * taps * CT; i += 256) {
        const int kl = i % kPackK, rest = i / kPackK;
        const int tap = rest % taps, cl = rest / taps;
        const int k = k0 + kl, c = c0 + cl;
        if (k < d.K && c < d.C) wt[((long)c * taps + tap) * ldk + k] = (T)tile[kl][cl * taps + tap];
      }
    }
  }
}

// The ResNet stem's weight on the width-packed input (conv.hip, "ResNet stem"):
// wk: bf16 [K][7][64] with wk[k][r][s*8+c] = w[k][c][r][s] (s < 7, c < C), else 0.
__global__ void stem_pack_weight_kernel(const float* w, int K, int C, bf16* wk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over K*7*64
  if (i >= K * 7 * 64) return;
  const int k = i / 448, rem = i - k * 448, r = rem / 64, j = rem - r * 64;
  const int s = j >> 3, c = j & 7;
  wk[i] = (bf16)((s < 7 && c < C) ? w[((k * C + c) * 7 + r) * 7 + s] : 0.f);
}

}  // namespace

// All of a model's conv weights in one launch.  desc: DEVICE array of n UnetsegPackDesc with
// ascending `start` = first tile (desc[0].start == 0; a conv has ceil(K/32)*ceil(Cpad/64) tiles);
// total = number of tiles.
// blocks of unetseg_pack_conv_weights for one conv (its desc.start advances by this much)
UNETSEG_API int unetseg_pack_tiles(int K, int Cpad, int taps) {
  const int ct = pack_ct(taps);
  return ceil_div(K, kPackK) * ceil_div(Cpad, ct);
}

UNETSEG_API int unetseg_pack_conv_weights(int dtype, const void* desc, int n, long total, void* stream) {
  US_CHECK_ARG(desc && n > 0 && total > 0 && total < (1L << 31), "pack_conv_weights: bad args");
  hipStream_t st = (hipStream_t)stream;
  const UnetsegPackDesc* d = (const UnetsegPackDesc*)desc;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(pack_weights_batched_kernel<bf16>, dim3(total), dim3(256), 0, st, d, n);
  else
    hipLaunchKernelGGL(pack_weights_batched_kernel<float>, dim3(total), dim3(256), 0, st, d, n);
  US_LAUNCH_CHECK("pack_weights_batched");
  return 0;
}

// fp32 [K][C][R][S] -> dtype [K][R][S][Cpad] (+ optional dtype [C][R][S][K] for dgrad)
UNETSEG_API int unetseg_pack_conv_weight(int dtype, const float* w, int K, int C, int R, int S, int Cpad, void* wk,
                                         void* wt, void* stream) {
  US_CHECK_ARG(w && wk && Cpad >= C, "pack_conv_weight: bad args");
  const long total = (long)K * R * S * Cpad;
  int blocks = ceil_div(total, 256);
  if (blocks > 8192) blocks = 8192;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(pack_weights_kernel<bf16>, dim3(blocks), dim3(256), 0, st, w, K, C, R, S, Cpad, (bf16*)wk, (bf16*)wt);
  else
    hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(blocks), dim3(256), 0, st, w, K, C, R, S, Cpad, (float*)wk, (float*)wt);
  US_LAUNCH_CHECK("pack_weights");
  return 0;
}

UNETSEG_API int unetseg_stem_pack_weight(const float* w, int K, int C, void* wk, void* stream) {
  US_CHECK_ARG(w && wk && C >= 1 && C <= 8 && K % 8 == 0, "stem_pack_weight: bad args");
  hipLaunchKernelGGL(stem_pack_weight_kernel, dim3(ceil_div((long)K * 448, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     K, C, (bf16*)wk);
  US_LAUNCH_CHECK("stem_pack_weight");
  return 0;
}
