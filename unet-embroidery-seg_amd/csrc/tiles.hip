// Tiled full-resolution inference (predict.predict_labels_tiled; no reference counterpart: the
// reference's predict.py only knows the 480x480 letterbox): cut a uint8 RGB image into overlapping
// network inputs on the device, blend the per-tile class probabilities back into one map, argmax.
//
// Grid (restated from utils/tiling.py, which the tests hold this file to): tile t, overlap o with
// 0 <= o <= t/2, stride s = t - o; n = max(1, ceil((L - o) / s)) tiles along an axis of L pixels, origins
// i * s, row-major tile index iy * nx + ix.  Tiles hang over the right / bottom edge and are never
// shifted back, so a pixel lies in at most 2 tiles per axis.  The 1-D window is
//   w(u) = min(1, (u + 1) / (o + 1), (t - u) / (o + 1))        (fp32)
// a pixel's weight in a tile is w(uy) * w(ux), and
//   prob = sum_i w_i softmax(logits_i) / sum_i w_i             over the covering tiles, ascending index.
// The accumulation is a gather with one writer per pixel per launch and no atomics: launches for
// successive tile ranges are ordered on the stream and every pixel adds its tiles in ascending index
// through the same chain of fmaf, so the accumulated bits do not depend on how the tiles were split
// into ranges.  All three kernels stream: one lane per pixel (four for the vector gather), x fastest,
// so a wave's loads and stores of every plane are contiguous; offsets are 64-bit.
#include <algorithm>

#include "elem_util.h"

// The letterbox path's label map (predict.predict_labels).  It stands ahead of the contraction pragma
// below, which is for the tile kernels only: this kernel keeps the compiler's default contraction.
namespace {

// ------------------------------------------------------------------------------------------
// predict.py:79-93 for one image: probabilities = softmax over C of logits [C][H][W], cropped to
// the letterbox window (y0, x0, ch, cw), resized bilinearly (half-pixel centres, edge clamp: cv2
// INTER_LINEAR = F.interpolate(align_corners=False) without antialias) to OH x OW, argmax (first).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_resize_argmax_kernel(const float* lg, int C, int H, int W, int y0,
                                                                    int x0, int ch, int cw, int OH, int OW,
                                                                    int32_t* labels) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)OH * OW) return;
  const int oy = (int)(i / OW), ox = (int)(i - (long)oy * OW);
  auto src = [](int d, int n_in, int n_out, int& i0, int& i1, float& l) {
    float s = ((float)d + 0.5f) * ((float)n_in / (float)n_out) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s;
    if (i0 > n_in - 1) i0 = n_in - 1;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l = s - (float)i0;
  };
  int ya, yb, xa, xb;
  float ly, lx;
  src(oy, ch, OH, ya, yb, ly);
  src(ox, cw, OW, xa, xb, lx);
  const long HW = (long)H * W;
  const long q[4] = {(long)(y0 + ya) * W + x0 + xa, (long)(y0 + ya) * W + x0 + xb, (long)(y0 + yb) * W + x0 + xa,
                     (long)(y0 + yb) * W + x0 + xb};
  const float wq[4] = {(1.f - ly) * (1.f - lx), (1.f - ly) * lx, ly * (1.f - lx), ly * lx};
  float mx[4], den[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, lg[c * HW + q[k]]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c * HW + q[k]] - m);
    mx[k] = m;
    den[k] = s;
  }
  float best = -1.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += wq[k] * (expf(lg[c * HW + q[k]] - mx[k]) / den[k]);
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  labels[i] = arg;
}

}  // namespace

// every fused multiply-add below is an explicit fmaf: the window weight is the ROUNDED product
// w(uy) * w(ux) in the accumulation and in the normalisation alike
#pragma clang fp contract(off)

namespace {

constexpr int kTileMaxC = kMaxC;

struct TileGrid {
  int t, o, s, nx, ny;
};

// the tiles of one axis that contain a pixel: n of them (1 or 2), ascending, with their window weights
struct Cover {
  int n, i0, i1;
  float w0, w1;
};

__device__ __forceinline__ float tile_window(int u, int t, float d) {
  return fminf(1.f, fminf((float)(u + 1) / d, (float)(t - u) / d));
}

// d = (float)(o + 1).  The last tile that starts at or before x always contains it (its far end is at
// least the axis' extent); the one before does when x lies in its overlap.
__device__ __forceinline__ Cover tile_cover(int x, int t, int s, int n, float d) {
  const int hi = min(x / s, n - 1);
  Cover c;
  const int u1 = x - hi * s;
  if (hi >= 1 && u1 + s < t) {
    c.n = 2;
    c.i0 = hi - 1;
    c.w0 = tile_window(u1 + s, t, d);
    c.i1 = hi;
    c.w1 = tile_window(u1, t, d);
  } else {
    c.n = 1;
    c.i0 = c.i1 = hi;
    c.w0 = c.w1 = tile_window(u1, t, d);
  }
  return c;
}

// out fp32 [nt][3][t][t]: lane = V consecutive x of one tile row, all three channels
template <int V>
__global__ __launch_bounds__(256) void tile_gather_kernel(const uint8_t* img, int H, int W, TileGrid g, int t0,
                                                          long total, float fillv, float* out) {
  const int tv = g.t / V;
  const long tt = (long)g.t * g.t;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int xg = (int)(i % tv);
    const long r = i / tv;
    const int y = (int)(r % g.t);
    const long j = r / g.t;
    const int idx = t0 + (int)j, iy = idx / g.nx, ix = idx - iy * g.nx;
    const long Y = (long)iy * g.s + y, X0 = (long)ix * g.s + (long)xg * V;
    float v[3][V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const long X = X0 + e;
      if (Y < H && X < W) {
        const uint8_t* p = img + (Y * W + X) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][e] = (float)p[c] / 255.0f;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][e] = fillv;
      }
    }
    float* o = out + j * 3 * tt + (long)y * g.t + (long)xg * V;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (V == 4) {
        const f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
        *reinterpret_cast<f32x4*>(o + c * tt) = q;
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) o[c * tt + e] = v[c][e];
      }
    }
  }
}

// acc fp32 [C][H][W] += w * softmax(logits) of the tiles t0 .. t0+nt-1 that cover the pixel.  The launch
// spans the rows (ry0 ..) and columns (rx0 .. rx0+rw-1) the range touches: blockIdx.x = row * bpr + column
// block.  A pixel none of the range's tiles covers is left alone.
__global__ __launch_bounds__(256) void tile_accum_kernel(const float* lg, int C, int H, int W, TileGrid g, int t0,
                                                         int nt, int ry0, int rx0, int rw, int bpr, float* acc) {
  const int row = blockIdx.x / bpr;
  const long xx = (long)(blockIdx.x - row * bpr) * 256 + threadIdx.x;
  if (xx >= rw) return;
  const int y = ry0 + row, x = rx0 + (int)xx;
  const float d = (float)(g.o + 1);
  const Cover cy = tile_cover(y, g.t, g.s, g.ny, d), cx = tile_cover(x, g.t, g.s, g.nx, d);
  const long HW = (long)H * W, tt = (long)g.t * g.t;
  float* a_out = acc + (long)y * W + x;
#pragma unroll 1
  for (int k = 0; k < cy.n * cx.n; ++k) {
    const int ky = k / cx.n, kx = k - ky * cx.n;
    const int iy = ky ? cy.i1 : cy.i0, ix = kx ? cx.i1 : cx.i0;
    const long j = (long)iy * g.nx + ix - t0;
    if (j < 0 || j >= nt) continue;
    const float w = (ky ? cy.w1 : cy.w0) * (kx ? cx.w1 : cx.w0);
    const float* p = lg + j * C * tt + (long)(y - iy * g.s) * g.t + (x - ix * g.s);
    float v[kTileMaxC];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kTileMaxC; ++c)
      if (c < C) {
        v[c] = p[c * tt];
        m = fmaxf(m, v[c]);
      }
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < kTileMaxC; ++c)
      if (c < C) {
        v[c] = expf(v[c] - m);
        den += v[c];
      }
    // the same lane re-reads what it stored for the previous tile of this pixel
#pragma unroll
    for (int c = 0; c < kTileMaxC; ++c)
      if (c < C) a_out[c * HW] = fmaf(w, v[c] / den, a_out[c * HW]);
  }
}

// probs (may be NULL) = acc / (the pixel's total window weight, recomputed from the grid with the
// accumulation's own rounded weights in its own order, so that a quotient never exceeds 1);
// labels = first argmax over the classes
__global__ __launch_bounds__(256) void tile_finish_kernel(const float* acc, int C, int H, int W, TileGrid g,
                                                          float* probs, int32_t* labels) {
  const long HW = (long)H * W;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= HW) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const float d = (float)(g.o + 1);
  const Cover cy = tile_cover(y, g.t, g.s, g.ny, d), cx = tile_cover(x, g.t, g.s, g.nx, d);
  float wsum = 0.f;
  for (int k = 0; k < cy.n * cx.n; ++k) {
    const int ky = k / cx.n, kx = k - ky * cx.n;
    const float w = (ky ? cy.w1 : cy.w0) * (kx ? cx.w1 : cx.w0);
    wsum += w;
  }
  float best = -1.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float p = acc[c * HW + i] / wsum;
    if (probs) probs[c * HW + i] = p;
    if (p > best) {
      best = p;
      arg = c;
    }
  }
  labels[i] = arg;
}

long axis_tiles(long L, int t, int o) {
  const long s = t - o, n = (L - o + s - 1) / s;
  return n < 1 ? 1 : n;
}

// the checked grid of an H x W image; 0, or 1 with the message set
int tile_grid(const char* name, int H, int W, int tile, int overlap, TileGrid& g) {
  US_CHECK_ARG(H > 0 && W > 0, "%s: bad image size H=%d W=%d", name, H, W);
  US_CHECK_ARG(tile > 0, "%s: tile must be positive, got %d", name, tile);
  US_CHECK_ARG(overlap >= 0 && overlap <= tile / 2, "%s: overlap %d outside [0, tile / 2 = %d]", name, overlap,
               tile / 2);
  const long nx = axis_tiles(W, tile, overlap), ny = axis_tiles(H, tile, overlap);
  US_CHECK_ARG(nx * ny <= INT32_MAX, "%s: %ld x %ld tiles do not fit the 32-bit tile index", name, nx, ny);
  g.t = tile;
  g.o = overlap;
  g.s = tile - overlap;
  g.nx = (int)nx;
  g.ny = (int)ny;
  return 0;
}

int tile_range(const char* name, const TileGrid& g, int t0, int nt) {
  US_CHECK_ARG(t0 >= 0 && nt > 0 && (long)t0 + nt <= (long)g.nx * g.ny,
               "%s: tile range t0=%d nt=%d outside the %d x %d grid", name, t0, nt, g.nx, g.ny);
  return 0;
}

// a * b * c * 4 bytes must fit a signed 64-bit offset (all factors positive)
bool fits_bytes(long a, long b, long c) {
  const long lim = INT64_MAX / 4;
  if (a > lim / b) return false;
  return a * b <= lim / c;
}

}  // namespace

// tiles per row (nx) and per column (ny) of the grid; host only, the rule of utils/tiling.py
UNETSEG_API int unetseg_tile_count(int H, int W, int tile, int overlap, int* nx, int* ny) {
  US_CHECK_ARG(nx && ny, "tile_count: null output");
  TileGrid g;
  if (tile_grid("tile_count", H, W, tile, overlap, g)) return 1;
  *nx = g.nx;
  *ny = g.ny;
  return 0;
}

// out fp32 [nt][3][tile][tile] = img (uint8 HWC RGB, device) / 255 for tiles t0 .. t0+nt-1, fill / 255
// outside the image
UNETSEG_API int unetseg_tile_gather(const uint8_t* img, int H, int W, int tile, int overlap, int t0, int nt, int fill,
                                    float* out, void* stream) {
  US_CHECK_ARG(img && out, "tile_gather: null pointer");
  TileGrid g;
  if (tile_grid("tile_gather", H, W, tile, overlap, g) || tile_range("tile_gather", g, t0, nt)) return 1;
  US_CHECK_ARG(fill >= 0 && fill <= 255, "tile_gather: fill %d is not a byte value", fill);
  US_CHECK_ARG(fits_bytes(H, W, 3), "tile_gather: image %d x %d exceeds 64-bit offsets", H, W);
  US_CHECK_ARG(fits_bytes((long)nt * 3, tile, tile), "tile_gather: %d tiles of %d exceed 64-bit offsets", nt, tile);
  const bool vec = tile % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const long total = (long)nt * tile * (tile / (vec ? 4 : 1));
  long blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride beyond 16 blocks per CU
  const float fillv = (float)fill / 255.0f;
  if (vec)
    hipLaunchKernelGGL(tile_gather_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, H, W, g,
                       t0, total, fillv, out);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, H, W, g,
                       t0, total, fillv, out);
  US_LAUNCH_CHECK("tile_gather");
  return 0;
}

// acc fp32 [C][H][W] (zeroed by the caller before the first range) += window * softmax over C of
// logits fp32 [nt][C][tile][tile], tiles t0 .. t0+nt-1
UNETSEG_API int unetseg_tile_accum(const float* logits, int C, int H, int W, int tile, int overlap, int t0, int nt,
                                   float* acc, void* stream) {
  US_CHECK_ARG(logits && acc, "tile_accum: null pointer");
  US_CHECK_ARG(C >= 2 && C <= kTileMaxC, "tile_accum: C=%d outside [2, %d]", C, kTileMaxC);
  TileGrid g;
  if (tile_grid("tile_accum", H, W, tile, overlap, g) || tile_range("tile_accum", g, t0, nt)) return 1;
  US_CHECK_ARG(fits_bytes(H, W, C), "tile_accum: H * W * C * 4 = %d * %d * %d * 4 exceeds 64-bit offsets", H, W, C);
  US_CHECK_ARG(fits_bytes((long)nt * C, tile, tile), "tile_accum: %d tiles of %d exceed 64-bit offsets", nt, tile);
  // rows and columns the range touches
  const int iy0 = t0 / g.nx, iy1 = (t0 + nt - 1) / g.nx;
  const long ry0 = (long)iy0 * g.s, ry1 = std::min<long>(H, (long)iy1 * g.s + g.t);
  long rx0 = 0, rx1 = W;
  if (iy0 == iy1) {
    rx0 = (long)(t0 - iy0 * g.nx) * g.s;
    rx1 = std::min<long>(W, (long)(t0 + nt - 1 - iy0 * g.nx) * g.s + g.t);
  }
  const long bpr = (rx1 - rx0 + 255) / 256, blocks = (ry1 - ry0) * bpr;
  US_CHECK_ARG(blocks <= INT32_MAX, "tile_accum: %ld blocks exceed the launch grid", blocks);
  hipLaunchKernelGGL(tile_accum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, logits, C, H, W, g,
                     t0, nt, (int)ry0, (int)rx0, (int)(rx1 - rx0), (int)bpr, acc);
  US_LAUNCH_CHECK("tile_accum");
  return 0;
}

// probs fp32 [C][H][W] (may be NULL) = acc / total window weight; labels int32 [H][W] = argmax, a tie to
// the lowest class
UNETSEG_API int unetseg_tile_finish(const float* acc, int C, int H, int W, int tile, int overlap, float* probs,
                                    int32_t* labels, void* stream) {
  US_CHECK_ARG(acc && labels, "tile_finish: null pointer");
  US_CHECK_ARG(C >= 2 && C <= kTileMaxC, "tile_finish: C=%d outside [2, %d]", C, kTileMaxC);
  TileGrid g;
  if (tile_grid("tile_finish", H, W, tile, overlap, g)) return 1;
  US_CHECK_ARG(fits_bytes(H, W, C), "tile_finish: H * W * C * 4 = %d * %d * %d * 4 exceeds 64-bit offsets", H, W, C);
  const long blocks = ((long)H * W + 255) / 256;
  US_CHECK_ARG(blocks <= INT32_MAX, "tile_finish: %ld blocks exceed the launch grid", blocks);
  hipLaunchKernelGGL(tile_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, C, H, W, g,
                     probs, labels);
  US_LAUNCH_CHECK("tile_finish");
  return 0;
}

// labels int32 [OH][OW] for one image's logits [C][H][W] (predict.py:79-93)
UNETSEG_API int unetseg_softmax_resize_argmax(const float* logits, int C, int H, int W, int y0, int x0, int ch, int cw,
                                              int OH, int OW, int32_t* labels, void* stream) {
  US_CHECK_ARG(logits && labels && C >= 1 && ch >= 1 && cw >= 1 && y0 >= 0 && x0 >= 0 && y0 + ch <= H &&
                   x0 + cw <= W && OH >= 1 && OW >= 1,
               "softmax_resize_argmax: bad window");
  hipLaunchKernelGGL(softmax_resize_argmax_kernel, dim3(ceil_div((long)OH * OW, 256)), dim3(256), 0,
                     (hipStream_t)stream, logits, C, H, W, y0, x0, ch, cw, OH, OW, labels);
  US_LAUNCH_CHECK("softmax_resize_argmax");
  return 0;
}
