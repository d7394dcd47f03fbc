// Soft skeleton and soft-clDice loss (Shit et al., CVPR 2021) for the binary and multitask heads
// (unetseg_hip/losses.py: soft_skeleton, cldice_loss, cldice_weight= of the region losses; no reference
// counterpart).
//
// Definition.  x fp32 [H][W] in [0, 1]; windows are clipped to the image.
//   E(x)(q) = min over q and its four edge neighbours      window order: up, left, centre, right, down
//   D(x)(q) = max over the 3 x 3 neighbourhood of q        window order: row-major
//   O(x)    = D(E(x))
//   x_0 = x,              d_0 = relu(x_0 - O(x_0)),  s_0 = d_0
//   x_j = E(x_{j-1}),     d_j = relu(x_j - O(x_j)),  s_j = s_{j-1} + relu(d_j - s_{j-1} d_j)     j = 1 .. k
//   S_k(x) = s_k
// Level 0 is level j with s_{-1} = 0 and no erosion in front, and runs as that: d_0 - 0 d_0 = d_0 bit for bit.
// Subgradients: relu'(a) = [a > 0]; a min or max window hands its whole gradient to the first element that attains
// the extreme in window order (strict comparisons while scanning in that order).
//
// Forward, one launch per level (k + 1 in all).  A block owns a 32 x 32 tile of one image and stages x_{j-1} with a
// 3-pixel halo in LDS: x_j on the tile + 2, E(x_j) on the tile + 1, O(x_j) on the tile.  x_j and O(x_j) are
// selections of input values, hence exact; d_j and s_j take four fp32 roundings a level (no contraction).
// 8 B read and 8 B written per pixel.
//
// Backward, one launch per level, j = k .. 0, in gather form: no atomics, every sum in a fixed order.
// With m = [d_j - s_{j-1} d_j > 0] and r = [x_j - O(x_j) > 0]:
//   gs_{j-1}(q) = gs_j(q) (1 - m d_j)                         the skeleton chain
//   gu(q)       = gs_j(q) m (1 - s_{j-1}(q)) r                into x_j(q) directly and, negated, into O(x_j)(q)
//   ge(r)       = Gx_{j+1}(r) - sum over q in the 3 x 3 of r whose max window selected r of gu(q)
//                 (e = E(x_j) is x_{j+1} as well as the input of D: both gradients take the same argmin hop)
//   Gx_j(t)     = gu(t) + sum over r in the cross of t whose min window selected t of ge(r)
// A block stages x_j with a 4-pixel halo and rebuilds e and its argmin on the tile + 3, gu and the argmax on the
// tile + 2, ge on the tile + 1.  16 B read and 8 B written per pixel.
//
// Loss.  p = sigmoid(z), y = [t == 1], ignored pixels p = y = 0.  Over the whole batch
//   tprec = (sum S(p) y + smooth) / (sum S(p) + smooth),  tsens = (sum S(y) p + smooth) / (sum S(y) + smooth),
//   L = 1 - 2 tprec tsens / (tprec + tsens).
// Launches of unetseg_cldice_fwd, all on the caller's stream, none waits on the host:
//   1. maps:    logits and target -> p, y and p (1 - p) (= hi * lo, see boundary_loss.hip)   16-byte vectors
//   2. forward of S(p), its levels kept for the backward; forward of S(y) between two pairs of scratch maps
//   3. sums:    four double partials per block; final: one block adds them in a fixed order and leaves L and
//               the three factors the backward needs (dL/dtprec / (sum S(p) + smooth), tprec,
//               dL/dtsens / (sum S(y) + smooth)) in device scalars
//   4. backward of S(p) from gs_k = cA (y - tprec), formed in the level-k kernel
//   5. gz:      gz (+)= weight * ((Gx_0 + cB S(y)) * p (1 - p))
#include "seg_pixel.h"

namespace {

constexpr int kT = 32;         // tile edge
constexpr int kCdGrid = 2048;  // block cap of the elementwise passes (their partial buffers are sized by it)
constexpr int kMaxIters = 64;

using Tiles = TileGrid<kT>;

// ---- stencil pieces on an LDS region ---------------------------------------------------------------------
// a[] has row pitch `pitch`; i is the centre's index.  Pixels outside the image hold +inf for a min window and
// -inf for a max window, so they never win a strict comparison against a value of the image.

// min over the cross in window order; sel = the winner's window position (0 up, 1 left, 2 centre, 3 right, 4 down)
__device__ __forceinline__ float cross_min(const float* a, int i, int pitch, int& sel) {
  float best = a[i - pitch];
  sel = 0;
  float v = a[i - 1];
  if (v < best) best = v, sel = 1;
  v = a[i];
  if (v < best) best = v, sel = 2;
  v = a[i + 1];
  if (v < best) best = v, sel = 3;
  v = a[i + pitch];
  if (v < best) best = v, sel = 4;
  return best;
}

// max over the 3 x 3 in row-major order; sel = the winner's window position 0 .. 8
__device__ __forceinline__ float box_max(const float* a, int i, int pitch, int& sel) {
  float best = a[i - pitch - 1];
  sel = 0;
#pragma unroll
  for (int w = 1; w < 9; ++w) {
    const float v = a[i + (w / 3 - 1) * pitch + (w % 3 - 1)];
    if (v > best) best = v, sel = w;
  }
  return best;
}

// region of edge kT + 2 * halo around the tile <- src (one image), `outside` where the image ends
template <int HALO>
__device__ __forceinline__ void stage(const float* src, int H, int W, int y0, int x0, float outside, float* dst) {
  constexpr int R = kT + 2 * HALO;
  for (int i = threadIdx.x; i < R * R; i += 256) {
    const int ry = i / R, rx = i - ry * R;
    const int y = y0 + ry - HALO, x = x0 + rx - HALO;
    dst[i] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(long)y * W + x] : outside;
  }
}

// ---- forward level ----------------------------------------------------------------------------------------
// FIRST: xin is x_0 and s_{-1} = 0 (sprev unused), nothing is eroded in front and xout is not written.
// Otherwise xin = x_{j-1}, xout = x_j = E(xin).  sout = s_j.  All maps [N][H][W].
template <bool FIRST>
__global__ __launch_bounds__(256) void skel_fwd_kernel(const float* xin, const float* sprev, int H, int W, int tiles_x,
                                                       int tiles_y, float* xout, float* sout) {
#pragma clang fp contract(off)
  constexpr int R3 = kT + 6, R2 = kT + 4, R1 = kT + 2;
  __shared__ float X0[FIRST ? 1 : R3 * R3];  // x_{j-1}, tile + 3, +inf outside
  __shared__ float X1[R2 * R2];              // x_j,     tile + 2, +inf outside
  __shared__ float E1[R1 * R1];              // E(x_j),  tile + 1, -inf outside
  const Tiles::Pos tp = Tiles::pos(tiles_x, tiles_y);
  const long base = tp.img * H * W;
  const float inf = __builtin_inff();
  if (FIRST) {
    stage<2>(xin + base, H, W, tp.y0, tp.x0, inf, X1);
  } else {
    stage<3>(xin + base, H, W, tp.y0, tp.x0, inf, X0);
    __syncthreads();
    for (int i = threadIdx.x; i < R2 * R2; i += 256) {
      const int ry = i / R2, rx = i - ry * R2;
      const int y = tp.y0 + ry - 2, x = tp.x0 + rx - 2;
      int sel;
      const float v = cross_min(X0, (ry + 1) * R3 + rx + 1, R3, sel);
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      X1[i] = in ? v : inf;
      if (in && ry >= 2 && ry < kT + 2 && rx >= 2 && rx < kT + 2) xout[base + (long)y * W + x] = v;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R1 * R1; i += 256) {
    const int ry = i / R1, rx = i - ry * R1;
    const int y = tp.y0 + ry - 1, x = tp.x0 + rx - 1;
    int sel;
    const float v = cross_min(X1, (ry + 1) * R2 + rx + 1, R2, sel);
    E1[i] = (y >= 0 && y < H && x >= 0 && x < W) ? v : -inf;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kT * kT; i += 256) {
    const int ry = i / kT, rx = i - ry * kT;
    const int y = tp.y0 + ry, x = tp.x0 + rx;
    if (y >= H || x >= W) continue;
    int sel;
    const float o = box_max(E1, (ry + 1) * R1 + rx + 1, R1, sel);
    const float d = fmaxf(X1[(ry + 2) * R2 + rx + 2] - o, 0.f);
    const long g = base + (long)y * W + x;
    const float s = FIRST ? 0.f : sprev[g];
    const float sd = s * d;
    sout[g] = s + fmaxf(d - sd, 0.f);
  }
}

// ---- backward level ---------------------------------------------------------------------------------------
// xj = x_j; sprev = s_{j-1} (NULL: 0, level 0); gs = gs_j, or with coef != NULL gs_j = coef[0] * (ymap - coef[1])
// (the clDice loss's top level); gxn = Gx_{j+1} (NULL: 0, level k); gsprev = gs_{j-1} (NULL at level 0); gx = Gx_j
__global__ __launch_bounds__(256) void skel_bwd_kernel(const float* xj, const float* sprev, const float* gs,
                                                       const float* coef, const float* ymap, const float* gxn, int H,
                                                       int W, int tiles_x, int tiles_y, float* gsprev, float* gx) {
#pragma clang fp contract(off)
  constexpr int R4 = kT + 8, R3 = kT + 6, R2 = kT + 4, R1 = kT + 2;
  __shared__ float X[R4 * R4];          // x_j,      tile + 4, +inf outside
  __shared__ float Ee[R3 * R3];         // E(x_j),   tile + 3, -inf outside
  __shared__ unsigned char Amin[R3 * R3];  // its winner's window position, 255 outside
  __shared__ float GU[R2 * R2];         // gu,       tile + 2, 0 outside
  __shared__ unsigned char Amax[R2 * R2];  // D's winner at that pixel, 255 outside
  __shared__ float GE[R1 * R1];         // ge,       tile + 1, 0 outside
  const Tiles::Pos tp = Tiles::pos(tiles_x, tiles_y);
  const long base = tp.img * H * W;
  const float inf = __builtin_inff();
  stage<4>(xj + base, H, W, tp.y0, tp.x0, inf, X);
  __syncthreads();
  for (int i = threadIdx.x; i < R3 * R3; i += 256) {
    const int ry = i / R3, rx = i - ry * R3;
    const int y = tp.y0 + ry - 3, x = tp.x0 + rx - 3;
    int sel;
    const float v = cross_min(X, (ry + 1) * R4 + rx + 1, R4, sel);
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    Ee[i] = in ? v : -inf;
    Amin[i] = in ? (unsigned char)sel : (unsigned char)255;
  }
  __syncthreads();
  const float cA = coef ? coef[0] : 0.f, cT = coef ? coef[1] : 0.f;
  for (int i = threadIdx.x; i < R2 * R2; i += 256) {
    const int ry = i / R2, rx = i - ry * R2;
    const int y = tp.y0 + ry - 2, x = tp.x0 + rx - 2;
    float gu = 0.f;
    unsigned char am = 255;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      int sel;
      const float o = box_max(Ee, (ry + 1) * R3 + rx + 1, R3, sel);
      am = (unsigned char)sel;
      const float u = X[(ry + 2) * R4 + rx + 2] - o;
      const float d = fmaxf(u, 0.f);
      const long g = base + (long)y * W + x;
      const float s = sprev ? sprev[g] : 0.f;
      const float gsj = coef ? cA * (ymap[g] - cT) : gs[g];
      const float sd = s * d;
      const bool m = d - sd > 0.f;
      gu = (m && u > 0.f) ? gsj * (1.f - s) : 0.f;
      if (gsprev && ry >= 2 && ry < kT + 2 && rx >= 2 && rx < kT + 2) gsprev[g] = m ? gsj * (1.f - d) : gsj;
    }
    GU[i] = gu;
    Amax[i] = am;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < R1 * R1; i += 256) {
    const int ry = i / R1, rx = i - ry * R1;
    const int y = tp.y0 + ry - 1, x = tp.x0 + rx - 1;
    float ge = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      if (gxn) ge = gxn[base + (long)y * W + x];
      const int c = (ry + 1) * R2 + rx + 1;
#pragma unroll
      for (int w = 0; w < 9; ++w) {  // q = r + offset(w) selected r iff its winner sits at the mirrored position
        const int q = c + (w / 3 - 1) * R2 + (w % 3 - 1);
        if (Amax[q] == 8 - w) ge -= GU[q];
      }
    }
    GE[i] = ge;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kT * kT; i += 256) {
    const int ry = i / kT, rx = i - ry * kT;
    const int y = tp.y0 + ry, x = tp.x0 + rx;
    if (y >= H || x >= W) continue;
    float g = GU[(ry + 2) * R2 + rx + 2];
    const int c1 = (ry + 1) * R1 + rx + 1, c3 = (ry + 3) * R3 + rx + 3;
    if (Amin[c3 - R3] == 4) g += GE[c1 - R1];  // up selected its `down`
    if (Amin[c3 - 1] == 3) g += GE[c1 - 1];    // left selected its `right`
    if (Amin[c3] == 2) g += GE[c1];
    if (Amin[c3 + 1] == 1) g += GE[c1 + 1];
    if (Amin[c3 + R3] == 0) g += GE[c1 + R1];
    gx[base + (long)y * W + x] = g;
  }
}

// ---- the loss's elementwise passes ------------------------------------------------------------------------
// thread = 4 consecutive pixels of the flat batch.  out planar fp32 [B][nch][P]; p, y, hl fp32 [total]
__global__ __launch_bounds__(256) void cd_maps_kernel(const float* out, int nch, long P, const int64_t* tgt, long total,
                                                      long ignore, float* p, float* y, float* hl) {
  const bool has_ign = ignore != -1;
  const long groups = (total + 3) / 4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;
    long t[4] = {0, 0, 0, 0};
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    ld_group(tgt + i0, m, t);
    ld_logit_group(out, nch, P, i0, m, z);
    float pv[4], yv[4], hv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = !(has_ign && t[k] == ignore);
      const Sigmoid sg = sigmoid_parts(z[k]);
      pv[k] = valid ? sg.p : 0.f;
      yv[k] = valid && t[k] == 1 ? 1.f : 0.f;
      hv[k] = valid ? sg.hi * sg.lo : 0.f;
    }
    st_group(p + i0, m, pv);
    st_group(y + i0, m, yv);
    st_group(hl + i0, m, hv);
  }
}

// part [4][kCdGrid]: the block's sums of S(p) y, S(p), S(y) p, S(y)
__global__ __launch_bounds__(256) void cd_sums_kernel(const float* sp, const float* sy, const float* p, const float* y,
                                                      long total, double* part) {
  __shared__ double sred[16];
  const long groups = (total + 3) / 4;
  double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;
    float vsp[4] = {0.f, 0.f, 0.f, 0.f}, vsy[4] = {0.f, 0.f, 0.f, 0.f}, vp[4] = {0.f, 0.f, 0.f, 0.f},
          vy[4] = {0.f, 0.f, 0.f, 0.f};
    ld_group(sp + i0, m, vsp), ld_group(sy + i0, m, vsy), ld_group(p + i0, m, vp), ld_group(y + i0, m, vy);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a1 += (double)vsp[k] * (double)vy[k];
      a2 += (double)vsp[k];
      b1 += (double)vsy[k] * (double)vp[k];
      b2 += (double)vsy[k];
    }
  }
  a1 = block_sum(a1, sred);
  a2 = block_sum(a2, sred);
  b1 = block_sum(b1, sred);
  b2 = block_sum(b2, sred);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = a1;
    part[kCdGrid + blockIdx.x] = a2;
    part[2 * kCdGrid + blockIdx.x] = b1;
    part[3 * kCdGrid + blockIdx.x] = b2;
  }
}

// loss[0] = L; coef = {dL/dtprec / (sum S(p) + smooth), tprec, dL/dtsens / (sum S(y) + smooth)}
__global__ __launch_bounds__(256) void cd_final_kernel(const double* part, int G, float smooth, float* coef,
                                                       float* loss) {
  __shared__ double sred[16];
  double s[4];
  for (int a = 0; a < 4; ++a) s[a] = sum_parts(part + a * kCdGrid, G, sred);
  if (threadIdx.x == 0) {
    const double sm = (double)smooth;
    const double tp = (s[0] + sm) / (s[1] + sm), ts = (s[2] + sm) / (s[3] + sm), den = tp + ts;
    loss[0] = (float)(1.0 - 2.0 * tp * ts / den);
    coef[0] = (float)(-2.0 * ts * ts / (den * den) / (s[1] + sm));
    coef[1] = (float)tp;
    coef[2] = (float)(-2.0 * tp * tp / (den * den) / (s[3] + sm));
  }
}

// gz (+)= weight * ((gx0 + coef[2] * sy) * hl): a product and a sum, never one fused multiply-add, so that
// accumulating onto a zeroed gz and writing gz give the same bits
__global__ __launch_bounds__(256) void cd_gz_kernel(const float* gx0, const float* sy, const float* hl,
                                                    const float* coef, long total, float weight, float* gz,
                                                    int accumulate) {
#pragma clang fp contract(off)
  const float cB = coef[2];
  const long groups = (total + 3) / 4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, h[4] = {0.f, 0.f, 0.f, 0.f},
          acc[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
    ld_group(gx0 + i0, m, a), ld_group(sy + i0, m, b), ld_group(hl + i0, m, h);
    if (accumulate) ld_group(gz + i0, m, acc);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float term = h[k] != 0.f ? (a[k] + cB * b[k]) * h[k] : 0.f;
      v[k] = acc[k] + weight * term;
    }
    st_group(gz + i0, m, v);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------
// the skeleton's workspace, in maps of `map` bytes: x_1 .. x_k | s_0 .. s_{k-1} | gs a, b | Gx a, b
struct SkelWorkspace {
  size_t map, bytes;
  int k;
  SkelWorkspace(size_t total, int iters) : k(iters) {
    map = up256(total * sizeof(float));
    bytes = map * (2 * (size_t)k + 4);
  }
  float* x(void* ws, int j) const { return (float*)((uint8_t*)ws + map * (size_t)(j - 1)); }      // j = 1 .. k
  float* s(void* ws, int j) const { return (float*)((uint8_t*)ws + map * (size_t)(k + j)); }      // j = 0 .. k-1
  float* scratch(void* ws, int i) const { return (float*)((uint8_t*)ws + map * (size_t)(2 * k + i)); }  // 0 .. 3
};

// S_k of x0 -> skel.  keep != NULL: x_1 .. x_k and s_0 .. s_{k-1} stay in its workspace for the backward;
// otherwise the levels alternate between the four maps of pp
void launch_skel_fwd(const float* x0, int N, int H, int W, int k, const SkelWorkspace* keep, void* ws, float* const* pp,
                     float* skel, hipStream_t st) {
  const Tiles t(N, H, W);
  const dim3 grid((unsigned)t.blocks), block(256);
  const float* xin = x0;
  const float* sprev = nullptr;
  for (int j = 0; j <= k; ++j) {
    float* sout = j == k ? skel : (keep ? keep->s(ws, j) : pp[2 + (j & 1)]);
    if (j == 0) {
      hipLaunchKernelGGL(skel_fwd_kernel<true>, grid, block, 0, st, xin, sprev, H, W, t.tx, t.ty, (float*)nullptr, sout);
    } else {
      float* xout = keep ? keep->x(ws, j) : pp[j & 1];
      hipLaunchKernelGGL(skel_fwd_kernel<false>, grid, block, 0, st, xin, sprev, H, W, t.tx, t.ty, xout, sout);
      xin = xout;
    }
    sprev = sout;
  }
}

// gx = d<gs_k, S_k(x0)>/dx0 from the levels launch_skel_fwd kept; gs_k = gskel, or coef[0] * (ymap - coef[1])
void launch_skel_bwd(const float* x0, int N, int H, int W, int k, const SkelWorkspace& lay, void* ws, const float* gskel,
                     const float* coef, const float* ymap, float* gx, hipStream_t st) {
  const Tiles t(N, H, W);
  const dim3 grid((unsigned)t.blocks), block(256);
  const float* gs = gskel;
  const float* gxn = nullptr;
  for (int j = k; j >= 0; --j) {
    const float* xj = j == 0 ? x0 : lay.x(ws, j);
    const float* sprev = j == 0 ? nullptr : lay.s(ws, j - 1);
    float* gsprev = j == 0 ? nullptr : lay.scratch(ws, j & 1);
    float* gxo = j == 0 ? gx : lay.scratch(ws, 2 + (j & 1));
    const bool top = j == k && coef;
    hipLaunchKernelGGL(skel_bwd_kernel, grid, block, 0, st, xj, sprev, top ? nullptr : gs, top ? coef : nullptr,
                       top ? ymap : nullptr, gxn, H, W, t.tx, t.ty, gsprev, gxo);
    gs = gsprev;
    gxn = gxo;
  }
}

// the loss's workspace: p | y | hl | S(p) | S(y) | Gx_0 | the skeleton's | part [4][kCdGrid] | coef
struct CdWorkspace {
  SkelWorkspace sk;
  size_t skel, part, coef, bytes;
  CdWorkspace(size_t total, int iters) : sk(total, iters) {
    skel = 6 * sk.map;
    part = skel + sk.bytes;
    coef = part + up256(4 * kCdGrid * sizeof(double));
    bytes = coef + 256;
  }
  float* map(void* ws, int i) const { return (float*)((uint8_t*)ws + sk.map * (size_t)i); }
};

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// host only
UNETSEG_API size_t unetseg_soft_skel_workspace(int N, int H, int W, int iters) {
  if (!Tiles::shape_ok(N, H, W) || iters < 0 || iters > kMaxIters) return 0;
  return SkelWorkspace((size_t)N * H * W, iters).bytes;
}

#define CD_CHECK_SKEL(name)                                                                                     \
  US_CHECK_ARG(Tiles::shape_ok(N, H, W), name ": bad shape N=%d H=%d W=%d", N, H, W);                               \
  US_CHECK_ARG(iters >= 0 && iters <= kMaxIters, name ": iters %d must be 0 .. %d", iters, kMaxIters);          \
  US_CHECK_ARG(ws_bytes >= unetseg_soft_skel_workspace(N, H, W, iters), name ": workspace too small");          \
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, name ": the workspace must be 16-byte aligned")

// skel [N][H][W] = S_iters(x); x_1 .. x_k and s_0 .. s_{k-1} stay in ws for unetseg_soft_skel_bwd
UNETSEG_API int unetseg_soft_skel_fwd(const float* x, int N, int H, int W, int iters, void* ws, size_t ws_bytes,
                                      float* skel, void* stream) {
  US_CHECK_ARG(x && ws && skel, "soft_skel_fwd: null pointer");
  CD_CHECK_SKEL("soft_skel_fwd");
  const SkelWorkspace lay((size_t)N * H * W, iters);
  launch_skel_fwd(x, N, H, W, iters, &lay, ws, nullptr, skel, (hipStream_t)stream);
  US_LAUNCH_CHECK("soft_skel_fwd");
  return 0;
}

// gx [N][H][W] = the gradient of sum(gskel * S_iters(x)) by x, with the subgradient rules of the head of this
// file; ws as unetseg_soft_skel_fwd left it for the same x, shape and iters
UNETSEG_API int unetseg_soft_skel_bwd(const float* x, int N, int H, int W, int iters, void* ws, size_t ws_bytes,
                                      const float* gskel, float* gx, void* stream) {
  US_CHECK_ARG(x && ws && gskel && gx, "soft_skel_bwd: null pointer");
  CD_CHECK_SKEL("soft_skel_bwd");
  const SkelWorkspace lay((size_t)N * H * W, iters);
  launch_skel_bwd(x, N, H, W, iters, lay, ws, gskel, nullptr, nullptr, gx, (hipStream_t)stream);
  US_LAUNCH_CHECK("soft_skel_bwd");
  return 0;
}

// host only
UNETSEG_API size_t unetseg_cldice_workspace(int B, int H, int W, int iters) {
  if (!Tiles::shape_ok(B, H, W) || iters < 0 || iters > kMaxIters) return 0;
  return CdWorkspace((size_t)B * H * W, iters).bytes;
}

// the soft-clDice loss of the head of this file.  out planar fp32 [B][nch][H][W]; tgt int64 [B][H][W];
// loss[0] = L (unweighted); gz [B][H][W] (may be NULL) = weight * dL/dz, added to gz when accumulate != 0
UNETSEG_API int unetseg_cldice_fwd(const float* out, int nch, const int64_t* tgt, int B, int H, int W, long ignore_index,
                                   int iters, float smooth, float weight, void* ws, size_t ws_bytes, float* gz,
                                   int accumulate, float* loss, void* stream) {
  US_CHECK_ARG(out && tgt && ws && loss, "cldice_fwd: null pointer");  // gz may be NULL
  US_CHECK_ARG(nch == 1 || nch == 2, "cldice_fwd: nch %d must be 1 or 2", nch);
  US_CHECK_ARG(Tiles::shape_ok(B, H, W), "cldice_fwd: bad shape B=%d H=%d W=%d", B, H, W);
  US_CHECK_ARG(iters >= 0 && iters <= kMaxIters, "cldice_fwd: iters %d must be 0 .. %d", iters, kMaxIters);
  US_CHECK_ARG(smooth > 0.f, "cldice_fwd: smooth %g must be > 0", (double)smooth);
  US_CHECK_ARG(ignore_index != 1, "cldice_fwd: ignore_index is the foreground class 1");
  US_CHECK_ARG(ws_bytes >= unetseg_cldice_workspace(B, H, W, iters), "cldice_fwd: workspace too small");
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, "cldice_fwd: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)H * W, total = (long)B * P;
  const CdWorkspace lay((size_t)total, iters);
  float *p = lay.map(ws, 0), *y = lay.map(ws, 1), *hl = lay.map(ws, 2), *sp = lay.map(ws, 3), *sy = lay.map(ws, 4),
        *gx0 = lay.map(ws, 5);
  void* skws = (uint8_t*)ws + lay.skel;
  double* part = (double*)((uint8_t*)ws + lay.part);
  float* coef = (float*)((uint8_t*)ws + lay.coef);
  const int G = grid_for((total + 3) / 4, kCdGrid);
  hipLaunchKernelGGL(cd_maps_kernel, dim3(G), dim3(256), 0, st, out, nch, P, tgt, total, ignore_index, p, y, hl);
  launch_skel_fwd(p, B, H, W, iters, &lay.sk, skws, nullptr, sp, st);
  // S(y) needs no backward: its levels alternate between the maps the backward of S(p) uses afterwards
  float* pp[4] = {lay.sk.scratch(skws, 0), lay.sk.scratch(skws, 1), lay.sk.scratch(skws, 2), lay.sk.scratch(skws, 3)};
  launch_skel_fwd(y, B, H, W, iters, nullptr, nullptr, pp, sy, st);
  hipLaunchKernelGGL(cd_sums_kernel, dim3(G), dim3(256), 0, st, (const float*)sp, (const float*)sy, (const float*)p,
                     (const float*)y, total, part);
  hipLaunchKernelGGL(cd_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, G, smooth, coef, loss);
  if (gz) {
    launch_skel_bwd(p, B, H, W, iters, lay.sk, skws, nullptr, coef, y, gx0, st);
    hipLaunchKernelGGL(cd_gz_kernel, dim3(G), dim3(256), 0, st, (const float*)gx0, (const float*)sy, (const float*)hl,
                       (const float*)coef, total, weight, gz, accumulate);
  }
  US_LAUNCH_CHECK("cldice_fwd");
  return 0;
}
