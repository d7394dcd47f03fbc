// Shared by the memory-bound translation units (elem, pool, upsample, pointwise, resize, tiles, tta, augment, loss,
// lovasz_softmax, multiclass, optim, cls_head, ccl, boundary): the 16-B vector width, the dtype dispatch and the
// small host helpers of their C-ABI sections.  boundary_loss, cldice and skeleton take it through seg_pixel.h,
// which adds what their per-pixel passes share (four-pixel group loads and stores, the logit group load, the
// sigmoid pieces, the sum of block partials, the workspace rounding, the tile grid and its shape check).
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace {

// elements of T in a 16-B vector
template <typename T>
constexpr int VE = 16 / sizeof(T);

// the same on the host, from the C ABI's dtype code
inline int vec_elems(int dtype) { return dtype == DT_BF16 ? 8 : 4; }

constexpr int kMaxC = 32;  // classes the multiclass kernels hold in registers

template <typename T>
__device__ __forceinline__ void cvt16(const uint4& raw, float (&out)[16 / sizeof(T)]) {
  const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
  for (int i = 0; i < 16 / (int)sizeof(T); ++i) out[i] = (float)e[i];
}

// blocks of 256 threads for `work` items, at least 1 and at most `cap` (the kernels stride over the rest)
inline int grid_for(long work, int cap = 16384) {
  long b = (work + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

inline int pow2_le(int v, int cap) {
  int t = 1;
  while (t * 2 <= v && t * 2 <= cap && v % (t * 2) == 0) t *= 2;
  return t;
}

// f(std::integral_constant<int, V>{}) for the V among Vs that equals the runtime value v; false (and
// no call) when none does: a launcher checks that.  Turns a runtime choice into a template argument
// without a macro ladder.
template <int... Vs, typename F>
inline bool with_const(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

}  // namespace

// runs the statement with T = bf16 or float
#define DISPATCH_T(dtype, ...)            \
  do {                                    \
    if ((dtype) == DT_BF16) {             \
      typedef bf16 T;                     \
      __VA_ARGS__;                        \
    } else {                              \
      typedef float T;                    \
      __VA_ARGS__;                        \
    }                                     \
  } while (0)

#define CHECK_VEC(dtype, C, name)                                                                               \
  do {                                                                                                          \
    US_CHECK_DTYPE(dtype, name);                                                                                \
    US_CHECK_ARG((C) > 0 && (C) % vec_elems(dtype) == 0,                                                        \
                 "%s: channels (%d) must be a positive multiple of the 16-B vector", name, (int)(C));           \
  } while (0)
