// Flip / rotation test-time augmentation (unetseg_hip/tta.py; no reference counterpart: the reference's
// predict.py has none): the K views of a batch in one launch, and the K per-view logit slabs merged
// back into one map of log mean probabilities.
//
// Views.  k in 0..7, f = k & 1, r = k >> 1: view k of x[.., H, W] is the W-flip (if f) followed by r
// counter-clockwise quarter turns, torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1)).  A set of
// views is the 8-bit mask `views` (bit k = view k), its slabs ordered by ascending k, K = popcount.
// A quarter turn (odd r: bits 2, 3, 6, 7) needs H == W.  view_map below is the one statement of where
// view k puts a pixel; both kernels go through it.
//
// Both kernels work on 32 x 32 tiles of the identity frame.  A view with even r keeps rows as rows, so
// a lane that walks x in the identity frame also walks x (up or down) in the view.  A quarter turn
// maps identity columns to view rows: there the lanes walk the identity tile's y instead, which is the
// view's x, and the values cross a 32 x 33 LDS tile between the two walks (row stride 33 dwords: the
// row-wise and the column-wise access both touch 32 different banks per 32 lanes).  So every global
// load and store of every view is two contiguous 128-B runs per wave.  Offsets are 64-bit.
//
// Merge.  out[b,c,y,x] = log(max(sum_k p_k[c] / K, FLT_MIN)), p_k = the max-subtracted softmax over C
// of view k's logits at the pixel view k maps (y, x) to.  The sum starts from 0 and adds the views in
// ascending k with plain fp32 adds, by the one lane that owns the output pixel: no atomics, and the bits
// do not depend on the launch geometry.  C == 1 (a sigmoid head) is the two-class softmax of (z, 0),
// i.e. (sigmoid(z), sigmoid(-z)) each formed on its own from expf(-|z|), and returns
// log(max(mean p, FLT_MIN)) - log(max(mean q, FLT_MIN)): a logit again, z itself for K = 1 up to rounding.
#include <cfloat>

#include "elem_util.h"

// the merge's sums and quotients are the rounded operations written below, never contracted
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 32;        // identity-frame tile edge
constexpr int kPad = kTile + 1;  // LDS row stride in dwords
constexpr int kChunk = 8;        // class planes that cross the LDS tile per barrier pair of the merge

// where view k puts pixel (y, x) of an H x W plane (H == W when k >> 1 is odd)
__device__ __forceinline__ void view_map(int k, int y, int x, int H, int W, int& vy, int& vx) {
  const int f = k & 1;
  switch (k >> 1) {
    case 0:
      vy = y;
      vx = f ? W - 1 - x : x;
      break;
    case 1:
      vy = f ? x : W - 1 - x;
      vx = y;
      break;
    case 2:
      vy = H - 1 - y;
      vx = f ? x : W - 1 - x;
      break;
    default:
      vy = f ? W - 1 - x : x;
      vx = H - 1 - y;
      break;
  }
}

// block = one 32 x 32 tile of one plane; thread (ty, tx) holds rows ty, ty + 8, ty + 16, ty + 24 at column tx
__global__ __launch_bounds__(256) void tta_views_kernel(const float* x, long planes, int H, int W, int views,
                                                        int tiles_x, int tiles_y, float* out) {
  __shared__ float s[kTile][kPad];
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x >> 5;
  const long tile = blockIdx.x;
  const long plane = tile / ((long)tiles_x * tiles_y);
  const int t = (int)(tile - plane * tiles_x * tiles_y);
  const int y0 = (t / tiles_x) * kTile, x0 = (t % tiles_x) * kTile;
  const long HW = (long)H * W;
  const float* src = x + plane * HW;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + ty + 8 * i, xx = x0 + tx;
    v[i] = (y < H && xx < W) ? src[(long)y * W + xx] : 0.f;
  }
  if (views & 0xCC) {  // a quarter turn is asked for: the tile crosses the LDS
#pragma unroll
    for (int i = 0; i < 4; ++i) s[ty + 8 * i][tx] = v[i];
    __syncthreads();
  }
  int slab = 0;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    if (!(views >> k & 1)) continue;
    float* dst = out + ((long)slab * planes + plane) * HW;
    ++slab;
    const bool turn = (k >> 1) & 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = ty + 8 * i;
      // lanes walk x of the identity tile, or its y under a quarter turn (the view's x either way)
      const int y = y0 + (turn ? tx : a), xx = x0 + (turn ? a : tx);
      if (y >= H || xx >= W) continue;
      int vy, vx;
      view_map(k, y, xx, H, W, vy, vx);
      dst[(long)vy * W + vx] = turn ? s[tx][a] : v[i];
    }
  }
}

// block = one 32 x 32 identity-frame tile of one image, all classes; thread (a, b) owns output pixel
// (y0 + a, x0 + b) and, for a quarter-turn view, carries the probabilities of pixel (y0 + b, x0 + a).
// NC = the register arrays' length (8 or kMaxC); n = the classes of the softmax (2 for C == 1).
template <int NC>
__global__ __launch_bounds__(1024) void tta_merge_kernel(const float* lg, int B, int C, int H, int W, int views,
                                                         int tiles_x, int tiles_y, float* out) {
  __shared__ float s[kChunk][kTile][kPad];
  const int b = threadIdx.x & (kTile - 1), a = threadIdx.x >> 5;
  const long tile = blockIdx.x;
  const long img = tile / ((long)tiles_x * tiles_y);
  const int t = (int)(tile - img * tiles_x * tiles_y);
  const int y0 = (t / tiles_x) * kTile, x0 = (t % tiles_x) * kTile;
  const long HW = (long)H * W;
  const int n = C == 1 ? 2 : C;
  const bool own = y0 + a < H && x0 + b < W;    // this lane's output pixel exists
  const bool carry = y0 + b < H && x0 + a < W;  // so does the transposed one
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  int slab = 0, K = 0;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    if (!(views >> k & 1)) continue;
    const float* base = lg + ((long)slab * B + img) * C * HW;
    ++slab;
    ++K;
    const bool turn = (k >> 1) & 1;
    const bool live = turn ? carry : own;
    float v[NC];
    if (live) {
      int vy, vx;
      view_map(k, y0 + (turn ? b : a), x0 + (turn ? a : b), H, W, vy, vx);
      const float* p = base + (long)vy * W + vx;
      float m = -INFINITY;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n) {
          v[c] = c < C ? p[c * HW] : 0.f;  // C == 1: the second logit is 0
          m = fmaxf(m, v[c]);
        }
      float den = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n) {
          v[c] = expf(v[c] - m);
          den += v[c];
        }
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < n) v[c] = v[c] / den;
    }
    if (!turn) {
      if (own) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < n) acc[c] += v[c];
      }
    } else {
      // carrier (a, b) holds pixel (b, a): store row a, column b; owner (a, b) reads row b, column a
#pragma unroll
      for (int c0 = 0; c0 < NC; c0 += kChunk) {
        if (c0 < n) {  // the same in every lane of the block
          if (carry) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j)
              if (c0 + j < n) s[j][a][b] = v[c0 + j];
          }
          __syncthreads();
          if (own) {
#pragma unroll
            for (int j = 0; j < kChunk; ++j)
              if (c0 + j < n) acc[c0 + j] += s[j][b][a];
          }
          __syncthreads();
        }
      }
    }
  }
  if (!own) return;
  const float kf = (float)K;
  float* o = out + img * C * HW + (long)(y0 + a) * W + (x0 + b);
  if (C == 1) {
    o[0] = logf(fmaxf(acc[0] / kf, FLT_MIN)) - logf(fmaxf(acc[1] / kf, FLT_MIN));
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < C) o[c * HW] = logf(fmaxf(acc[c] / kf, FLT_MIN));
  }
}

// the checked geometry shared by the two entry points; 0, or 1 with the message set
int tta_geometry(const char* name, int B, int C, int H, int W, int views, long& tiles) {
  US_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: bad shape B=%d C=%d H=%d W=%d", name, B, C, H, W);
  US_CHECK_ARG(views >= 1 && views <= 255, "%s: views mask %d outside [1, 255]", name, views);
  US_CHECK_ARG(!(views & 0xCC) || H == W, "%s: views mask 0x%02x has a quarter turn, which needs H == W (got %d x %d)",
               name, views, H, W);
  // K * B * C * H * W * 4 bytes within a signed 64-bit offset
  long e = 4L * __builtin_popcount(views);
  bool fits = true;
  for (long f : {(long)B, (long)C, (long)H, (long)W}) {
    if (e > INT64_MAX / f) {
      fits = false;
      break;
    }
    e *= f;
  }
  US_CHECK_ARG(fits, "%s: K * B * C * H * W * 4 = %d * %d * %d * %d * %d * 4 exceeds 64-bit offsets", name,
               __builtin_popcount(views), B, C, H, W);
  tiles = (long)((H + kTile - 1) / kTile) * ((W + kTile - 1) / kTile);
  return 0;
}

}  // namespace

// out fp32 [K][B][C][H][W] = the views of x fp32 [B][C][H][W] named by the mask, ascending k; a pure
// permutation
UNETSEG_API int unetseg_tta_views(const float* x, int B, int C, int H, int W, int views, float* out, void* stream) {
  US_CHECK_ARG(x && out, "tta_views: null pointer");
  long tiles;
  if (tta_geometry("tta_views", B, C, H, W, views, tiles)) return 1;
  const long planes = (long)B * C;
  US_CHECK_ARG(tiles <= INT32_MAX / planes, "tta_views: %ld planes of %ld tiles exceed the launch grid", planes,
               tiles);
  hipLaunchKernelGGL(tta_views_kernel, dim3((unsigned)(planes * tiles)), dim3(256), 0, (hipStream_t)stream, x, planes,
                     H, W, views, (W + kTile - 1) / kTile, (H + kTile - 1) / kTile, out);
  US_LAUNCH_CHECK("tta_views");
  return 0;
}

// out fp32 [B][C][H][W] (identity frame) = log mean_k softmax of logits fp32 [K][B][C][H][W], slab k in
// view k's frame; C == 1: the logit of the mean sigmoid
UNETSEG_API int unetseg_tta_merge(const float* logits, int B, int C, int H, int W, int views, float* out,
                                  void* stream) {
  US_CHECK_ARG(logits && out, "tta_merge: null pointer");
  long tiles;
  if (tta_geometry("tta_merge", B, C, H, W, views, tiles)) return 1;
  US_CHECK_ARG(C <= kMaxC, "tta_merge: C=%d outside [1, %d]", C, kMaxC);
  US_CHECK_ARG(tiles <= INT32_MAX / B, "tta_merge: %d images of %ld tiles exceed the launch grid", B, tiles);
  const bool ok = with_const<8, kMaxC>(C <= 8 ? 8 : kMaxC, [&](auto nc) {
    hipLaunchKernelGGL((tta_merge_kernel<decltype(nc)::value>), dim3((unsigned)(B * tiles)), dim3(1024), 0,
                       (hipStream_t)stream, logits, B, C, H, W, views, (W + kTile - 1) / kTile,
                       (H + kTile - 1) / kTile, out);
  });
  US_CHECK_ARG(ok, "tta_merge: no kernel for C=%d", C);
  US_LAUNCH_CHECK("tta_merge");
  return 0;
}
