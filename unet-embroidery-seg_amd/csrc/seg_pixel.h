// Shared by the per-pixel passes over the binary head and over class maps (boundary_loss, cldice, skeleton):
// four-pixel group loads and stores, the logit group load, the sigmoid pieces, the fixed-order sum of block
// partials, and the host's workspace rounding, tile grid and shape check.
//
// The device helpers only load, store, subtract and divide.  A product that feeds a sum stays in the kernel
// that owns it, under that kernel's `#pragma clang fp contract(off)`: the pragma scopes lexically and would
// not reach a helper.
#pragma once
#include "elem_util.h"

namespace {

typedef long i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// v = p[0 .. 3]: 16-byte loads when p is 16-byte aligned (the same for every group of an array whose
// base is, as groups start at multiples of 4 elements), else element loads
__device__ __forceinline__ void ld4(const int64_t* p, long (&v)[4]) {
  if (aligned16(p)) {
    const i64x2 a = *reinterpret_cast<const i64x2*>(p), b = *reinterpret_cast<const i64x2*>(p + 2);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[k];
  }
}
template <typename T>  // a 4-byte T
__device__ __forceinline__ void ld4(const T* p, T (&v)[4]) {
  if (aligned16(p)) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = e[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = p[k];
  }
}
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  if (aligned16(p)) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = v[k];
  }
}

// a group of the flat batch: four pixels, or the m < 4 that are left at its end.  v[m ..] is not touched
template <typename P, typename V>
__device__ __forceinline__ void ld_group(const P* p, int m, V (&v)[4]) {
  if (m == 4) {
    ld4(p, v);
  } else {
    for (int k = 0; k < m; ++k) v[k] = p[k];
  }
}
__device__ __forceinline__ void st_group(float* p, int m, const float (&v)[4]) {
  if (m == 4) {
    st4(p, v);
  } else {
    for (int k = 0; k < m; ++k) p[k] = v[k];
  }
}

// z[0 .. m) of the group at flat pixel i0 of planar fp32 logits [B][nch][P]: o1 - o0 (nch 2) or o0 (nch 1)
__device__ __forceinline__ void ld_logit_group(const float* out, int nch, long P, long i0, int m, float (&z)[4]) {
  const long b0 = i0 / P, px0 = i0 - b0 * P;
  if (m == 4 && px0 + 4 <= P) {  // the group lies in one image: its logit planes are contiguous
    const float* base = out + b0 * nch * P + px0;
    float o0[4], o1[4];
    ld4(base, o0);
    ld4(base + (nch == 2 ? P : 0), o1);
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = nch == 2 ? o1[k] - o0[k] : o0[k];
  } else {
    for (int k = 0; k < m; ++k) {
      const long i = i0 + k, b = i / P;
      const float* base = out + b * nch * P + (i - b * P);
      z[k] = nch == 2 ? base[P] - base[0] : base[0];
    }
  }
}

// hi = sigmoid(|z|), lo = sigmoid(-|z|), p = sigmoid(z); p (1 - p) = hi * lo, which keeps its relative
// accuracy where 1 - p would cancel
struct Sigmoid {
  float hi, lo, p;
};
__device__ __forceinline__ Sigmoid sigmoid_parts(float z) {
  const float e = expf(-fabsf(z));
  const float d = 1.f + e, hi = 1.f / d, lo = e / d;
  return {hi, lo, z >= 0.f ? hi : lo};
}

// one block of 256 threads: the sum of part[0 .. G) in a fixed order, in every thread
template <typename A, typename T>
__device__ __forceinline__ A sum_parts(const T* part, int G, A* sred /* >= 16 entries */) {
  A s = 0;
  for (int i = threadIdx.x; i < G; i += 256) s += part[i];
  return block_sum(s, sred);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// N images [H][W] cut into tiles of TW x TH pixels, one block per tile
template <int TW, int TH = TW>
struct TileGrid {
  int tx, ty;
  long blocks;
  TileGrid(int N, int H, int W) : tx((W + TW - 1) / TW), ty((H + TH - 1) / TH) { blocks = (long)tx * ty * N; }

  // what the kernels take: at most 2^40 pixels, and the block count fits an int
  static bool shape_ok(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return false;
    const TileGrid t(N, H, W);
    return t.blocks <= 0x7fffffffL && (size_t)N * H * W <= ((size_t)1 << 40);
  }

  // block -> (image, tile of the image, tile origin)
  struct Pos {
    long img;
    int tile, y0, x0;
  };
  static __device__ __forceinline__ Pos pos(int tiles_x, int tiles_y) {
    const long b = blockIdx.x;
    const long per = (long)tiles_x * tiles_y;
    Pos t;
    t.img = b / per;
    t.tile = (int)(b - t.img * per);
    t.y0 = (t.tile / tiles_x) * TH;
    t.x0 = (t.tile % tiles_x) * TW;
    return t;
  }
};

}  // namespace
