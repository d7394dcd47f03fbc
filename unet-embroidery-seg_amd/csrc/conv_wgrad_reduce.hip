// The deterministic split-K reduce of the weight gradients: every family (generic, fast, ring, halo)
// writes slabs ws[split][cout][r*s*cin] that these kernels sum into dW in a fixed order -- slab order
// within a lane, then lane order -- so each result bit depends on that order alone.  Also the stem's
// permutation of its reduced virtual gradient.
#include "common.h"
#include "conv_generic.h"

namespace {

__device__ __forceinline__ void add4(float4& v, const float4& a) {
  v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
}

// dW[k][c][tap] (+)= sum_z ws[z][k][tap*cin + c] for c < dw_c.  Block = (output channel k, a run of
// cw input channels) x SL split lanes: item i = (tap, 4 channels) is one 16-B load per slab; lane l
// sums slabs l, l+SL, ... in ascending order, the SL partials are combined in LDS in a fixed order
// (deterministic), and the block's dW run -- cw x taps consecutive floats of PyTorch's [K][C][R][S]
// -- is written through an LDS transpose, so both the slab reads and the dW writes are contiguous.
template <int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, int splits, int Cout, int cin, int taps,
                                                           float* dw, int dw_c, int accumulate, int cw, int rows_out) {
  constexpr int IT = 256 / SL;
  __shared__ float4 red[SL][IT];
  __shared__ float tile[1024];
  const long Ng = (long)taps * cin, slab = (long)Cout * Ng;
  const int nchunk = (dw_c + cw - 1) / cw;
  const int k = blockIdx.x / nchunk, cc0 = (blockIdx.x - k * nchunk) * cw;
  if (k >= rows_out) return;  // whole block: a padded output channel, not written
  const int q4 = cw >> 2, items = taps * q4;
  const int it = threadIdx.x % IT, sl = threadIdx.x / IT;
  const int tap = it / q4, cl = (it - tap * q4) * 4;
  const bool live = it < items && cc0 + cl < dw_c;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4* p = reinterpret_cast<const float4*>(ws + (long)k * Ng + (long)tap * cin + cc0 + cl);
    const long s4 = slab >> 2;
    int z = sl;
    for (; z + 3 * SL < splits; z += 4 * SL) {
      const float4 a = p[z * s4], b = p[(z + SL) * s4], c = p[(z + 2 * SL) * s4], d = p[(z + 3 * SL) * s4];
      add4(v, a);
      add4(v, b);
      add4(v, c);
      add4(v, d);
    }
    for (; z < splits; z += SL) {
      const float4 a = p[z * s4];
      add4(v, a);
    }
  }
  if constexpr (SL > 1) {
    red[sl][it] = v;
    __syncthreads();
    if (sl == 0)
      for (int j = 1; j < SL; ++j) {
        const float4 a = red[j][it];
        add4(v, a);
      }
  }
  if (sl == 0 && it < items) {  // [c][tap] order of the block's dW run
    tile[(cl + 0) * taps + tap] = v.x;
    tile[(cl + 1) * taps + tap] = v.y;
    tile[(cl + 2) * taps + tap] = v.z;
    tile[(cl + 3) * taps + tap] = v.w;
  }
  __syncthreads();
  const int run = min(cw, dw_c - cc0) * taps;
  float* out = dw + ((long)k * dw_c + cc0) * taps;
  for (int i = threadIdx.x; i < run; i += 256) out[i] = accumulate ? out[i] + tile[i] : tile[i];
}

// The same sum when there are many slabs (or a 1x1 filter): block = IT consecutive float4 items of a
// slab x SL split lanes; lane l sums the contiguous slab range [l*R, (l+1)*R), R = ceil(splits/SL),
// four loads in flight, and the SL partials are added in LDS in lane order (deterministic).  Enough
// (item, lane) pairs to keep every CU streaming; the dW writes are permuted 4-B stores (float4 for
// 1x1), a 1/splits share of the traffic.
template <int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_split_kernel(const float* ws, int splits, int Cout, int cin,
                                                                 int taps, float* dw, int dw_c, int accumulate,
                                                                 int rows_out) {
  constexpr int IT = 256 / SL;
  __shared__ float4 red[SL][IT];
  const long Ng = (long)taps * cin, s4 = (long)Cout * Ng / 4;
  const int it = threadIdx.x % IT, sl = threadIdx.x / IT;
  const long q = (long)blockIdx.x * IT + it;
  const int R = (splits + SL - 1) / SL;
  const int z1 = min(splits, (sl + 1) * R);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < s4) {
    const float4* p = reinterpret_cast<const float4*>(ws) + q;
    int z = sl * R;
    for (; z + 7 < z1; z += 8) {  // eight slabs in flight, added in slab order
      float4 a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = p[(z + u) * s4];
#pragma unroll
      for (int u = 0; u < 8; ++u) add4(v, a[u]);
    }
    for (; z + 3 < z1; z += 4) {
      const float4 a = p[z * s4], b = p[(z + 1) * s4], c = p[(z + 2) * s4], d = p[(z + 3) * s4];
      add4(v, a);
      add4(v, b);
      add4(v, c);
      add4(v, d);
    }
    for (; z < z1; ++z) {
      const float4 a = p[z * s4];
      add4(v, a);
    }
  }
  if constexpr (SL > 1) {
    red[sl][it] = v;
    __syncthreads();
    if (sl != 0) return;
    v = red[0][it];
    for (int j = 1; j < SL; ++j) {
      const float4 a = red[j][it];
      add4(v, a);
    }
  }
  if (q >= s4) return;
  const long k = q * 4 / Ng;
  if (k >= rows_out) return;  // a padded output channel (after the block's last barrier)
  const int col = (int)(q * 4 - k * Ng);
  const int tap = col / cin, c0 = col - tap * cin;
  if (taps == 1 && c0 + 4 <= dw_c && dw_c % 4 == 0) {
    float4* o = reinterpret_cast<float4*>(dw + k * dw_c + c0);
    if (accumulate) {
      const float4 w = *o;
      add4(v, w);
    }
    *o = v;
    return;
  }
  const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (c0 + e >= dw_c) break;
    const long dst = (k * dw_c + c0 + e) * taps + tap;
    dw[dst] = accumulate ? dw[dst] + e4[e] : e4[e];
  }
}

// dw[k][c][r][s] (+)= v[k][s*8 + c][r]   (c < C, s < 7): the split-reduced virtual gradient
// (wgrad_reduce_kernel, layout [K][64][7]) permuted into PyTorch's [K][C][7][7]
__global__ void stem_wgrad_remap_kernel(const float* v, int K, int C, float* dw, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over K*C*49
  if (i >= K * C * 49) return;
  const int k = i / (C * 49), rem = i - k * C * 49, c = rem / 49, rs = rem - c * 49;
  const int r = rs / 7, s = rs - r * 7;
  const float g = v[((long)k * 64 + s * 8 + c) * 7 + r];
  dw[i] = accumulate ? dw[i] + g : g;
}

}  // namespace

// Few slabs of a multi-tap filter: the transposing kernel (coalesced dW runs, one lane group per
// block); otherwise the split-parallel kernel with ~4 (up to splits / 16) slabs per lane.
void launch_wgrad_reduce(const float* ws, int splits, int cout, int cin, int taps, float* dw, int dw_c,
                         int accumulate, hipStream_t st, int rows_out) {
  if (rows_out < 0 || rows_out > cout) rows_out = cout;
  if (taps > 1 && splits <= 8 && taps <= 256) {
    int cw = 4 * (256 / taps);
    if (cw > 1024 / taps / 4 * 4) cw = 1024 / taps / 4 * 4;  // LDS transpose tile
    if (cw > 64) cw = 64;
    if (cw > ceil_div(dw_c, 4) * 4) cw = ceil_div(dw_c, 4) * 4;
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(cout * ceil_div(dw_c, cw)), dim3(256), 0, st, ws, splits, cout,
                       cin, taps, dw, dw_c, accumulate, cw, rows_out);
    return;
  }
  int sl = 1;  // at most 16 lanes: 16-item (256-B) runs per slab read, a short LDS combine
  while (sl < 16 && sl * 4 < splits) sl *= 4;
  const long s4 = (long)cout * taps * cin / 4;
  const unsigned blocks = (unsigned)((s4 + 256 / sl - 1) / (256 / sl));
  switch (sl) {
    case 16: hipLaunchKernelGGL(wgrad_reduce_split_kernel<16>, dim3(blocks), dim3(256), 0, st, ws, splits, cout, cin, taps, dw, dw_c, accumulate, rows_out); break;
    case 4: hipLaunchKernelGGL(wgrad_reduce_split_kernel<4>, dim3(blocks), dim3(256), 0, st, ws, splits, cout, cin, taps, dw, dw_c, accumulate, rows_out); break;
    default: hipLaunchKernelGGL(wgrad_reduce_split_kernel<1>, dim3(blocks), dim3(256), 0, st, ws, splits, cout, cin, taps, dw, dw_c, accumulate, rows_out); break;
  }
}

void launch_stem_wgrad_remap(const float* v, int K, int C, float* dw, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(stem_wgrad_remap_kernel, dim3(ceil_div((long)K * C * 49, 256)), dim3(256), 0, st, v, K, C, dw,
                     accumulate);
}
