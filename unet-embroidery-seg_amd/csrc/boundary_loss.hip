// Boundary (distance-map) loss of Kervadec et al., MIDL 2019, for the binary and multitask heads
// (unetseg_hip/losses.py: boundary_loss, signed_distance, boundary_weight= of the region losses; no
// reference counterpart).  L = inv_norm / Nvalid * sum over the valid pixels of sigmoid(z) * phi, with phi
// the signed distance to the target's contour, from the exact distance transform of boundary.hip.
//
// Definition.  Target t int64 [B][H][W], class c, `ignore` (-1: none).  Per image, fg = {t == c},
// bg = {t != c, t != ignore}; ignored pixels are neither.  d2fg / d2bg = the exact squared distance to
// the nearest fg / bg pixel of the same image, kEdtInf where the image has none.
//   phi(q) = +sqrt(d2fg(q))        for q in bg
//            -(sqrt(d2bg(q)) - 1)  for q in fg
//            0                     for ignored q, and wherever the distance it would use is kEdtInf
// (one_hot2dist of the paper: edt(neg) * neg - (edt(pos) - 1) * pos), so an image without foreground and
// one without background contribute 0 at every pixel without any per-image reduction.  p = sigmoid(z),
// z = o1 - o0 (nch 2) or o0 (nch 1).  Nvalid = the non-ignored pixels of the batch;
//   L = inv_norm / Nvalid * sum_valid p phi,   gz = p (1 - p) phi inv_norm / Nvalid   (0 on ignored pixels),
// both 0 when Nvalid == 0.
//
// Launches, all on the caller's stream, none waits on the host:
//   1. sites:  reads t once, writes both uint8 site maps [2][B][H][W] (fg maps, then bg maps) and the
//              valid pixels each block saw.                          8 B read, 2 B written per pixel
//   2. count:  one block sums the blocks' counts: Nvalid and scale = inv_norm / Nvalid (0 if none), so
//              gz is written once, already divided; no second pass over gz.
//   3. the distance transform of boundary.hip over N = 2 B images (two or three launches; 1 B read and
//              4 B written, read and written again by each further launch)
//   4. loss:   one pass: logits (4 nch B), t (8 B), d2fg and d2bg (8 B) in; gz (4 B, + 4 B read when it
//              accumulates) and phi (4 B, optional) out; a partial sum of p * phi per block, in double.
//   5. final:  one block sums the partials in a fixed order: loss = sum * inv_norm / Nvalid.
// Every sum has a fixed order and the distances are integers, so loss, gz and phi are bitwise reproducible.
//
// Rounding (DESIGN.md has the bound the tests hold): phi is exact up to the one rounding of the square
// root (taken in double, so a d2 above 2^24 is not rounded first; r - 1 is exact).  With
// e = expf(-|z|), d = 1 + e, hi = 1 / d = sigmoid(|z|), lo = e / d = sigmoid(-|z|): p = hi or lo by the
// sign of z, and p (1 - p) = hi * lo, which keeps its relative accuracy where 1 - p would cancel.
#include "boundary_edt.h"
#include "seg_pixel.h"

namespace {

constexpr int kBlGrid = 2048;  // block cap of the sites and loss kernels (their partial buffers are sized by it)

// ---- 1. site maps ------------------------------------------------------------------------------------
// thread = 4 consecutive pixels of the flat batch; fg / bg uint8 [total]; cnt[block] = valid pixels seen
__global__ __launch_bounds__(256) void bl_sites_kernel(const int64_t* tgt, long total, int c, long ignore,
                                                       uint8_t* fg, uint8_t* bg, unsigned* cnt) {
  __shared__ unsigned sred[16];
  const bool has_ign = ignore != -1;
  const long groups = (total + 3) / 4;
  unsigned n = 0;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;  // pixels of the group inside the batch
    long t[4] = {0, 0, 0, 0};
    ld_group(tgt + i0, m, t);
    unsigned f = 0, b = 0;  // the group's site bytes, pixel k in byte k
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool in = k < m, ign = has_ign && t[k] == ignore, isfg = t[k] == c;
      f |= (in && isfg ? 1u : 0u) << (8 * k);
      b |= (in && !isfg && !ign ? 1u : 0u) << (8 * k);
      n += in && !ign;
    }
    // fg is 4-byte aligned (the workspace is); bg = fg + total is when total is a multiple of 4
    if (m == 4 && ((uintptr_t)(bg + i0) & 3) == 0) {
      *reinterpret_cast<unsigned*>(fg + i0) = f;
      *reinterpret_cast<unsigned*>(bg + i0) = b;
    } else {
      for (int k = 0; k < m; ++k) {
        fg[i0 + k] = (uint8_t)(f >> (8 * k));
        bg[i0 + k] = (uint8_t)(b >> (8 * k));
      }
    }
  }
  n = block_sum(n, sred);
  if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// ---- 2. Nvalid and the factor of every term ------------------------------------------------------------
__global__ __launch_bounds__(256) void bl_count_kernel(const unsigned* cnt, int G, float inv_norm, double* nvalid,
                                                       float* scale) {
  __shared__ unsigned long long sred[16];
  const unsigned long long n = sum_parts(cnt, G, sred);
  if (threadIdx.x == 0) {
    nvalid[0] = (double)n;
    scale[0] = n > 0 ? (float)((double)inv_norm / (double)n) : 0.f;
  }
}

// ---- 4. the loss pass ------------------------------------------------------------------------------------
// thread = 4 consecutive pixels of the flat batch.  d2fg / d2bg int32 [total]; gz, phi fp32 [total] (either
// may be NULL); part[block] = the block's sum of p * phi over its valid pixels
__global__ __launch_bounds__(256) void bl_loss_kernel(const float* out, int nch, long P, const int64_t* tgt,
                                                      const int* d2fg, const int* d2bg, long total, int c,
                                                      long ignore, const float* scale, float weight, float* gz,
                                                      int accumulate, float* phi, double* part) {
  // gz is base + weight * term as a product and a sum, never one fused multiply-add: accumulating onto a
  // zeroed gz and writing gz then give the same bits
#pragma clang fp contract(off)
  __shared__ double sred[16];
  const bool has_ign = ignore != -1;
  const float sc = scale[0];
  const long groups = (total + 3) / 4;
  double s = 0.0;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const int m = total - i0 < 4 ? (int)(total - i0) : 4;
    long t[4] = {0, 0, 0, 0};
    int df[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};
    float z[4] = {0.f, 0.f, 0.f, 0.f}, acc[4] = {0.f, 0.f, 0.f, 0.f};
    ld_group(tgt + i0, m, t);
    ld_group(d2fg + i0, m, df);
    ld_group(d2bg + i0, m, db);
    if (accumulate && gz) ld_group(gz + i0, m, acc);
    ld_logit_group(out, nch, P, i0, m, z);
    float f[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = k < m && !(has_ign && t[k] == ignore), isfg = t[k] == c;
      const int d2 = isfg ? db[k] : df[k];
      const float r = (float)sqrt((double)d2);  // one rounding: the double root of an integer, cast
      f[k] = !valid || d2 == kEdtInf ? 0.f : (isfg ? 1.f - r : r);  // r >= 1 on fg; r - 1 is exact
      const Sigmoid sg = sigmoid_parts(z[k]);
      const float term = valid ? ((sg.hi * sg.lo) * f[k]) * sc : 0.f;
      v[k] = acc[k] + weight * term;
      if (valid) s += (double)sg.p * (double)f[k];
    }
    if (gz) st_group(gz + i0, m, v);
    if (phi) st_group(phi + i0, m, f);
  }
  s = block_sum(s, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ---- 5. loss = inv_norm / Nvalid * sum of the partials (fixed order) ---------------------------------------
__global__ __launch_bounds__(256) void bl_final_kernel(const double* part, int G, const double* nvalid,
                                                       float inv_norm, float* loss) {
  __shared__ double sred[16];
  const double s = sum_parts(part, G, sred);
  if (threadIdx.x == 0) loss[0] = nvalid[0] > 0.0 ? (float)(s * (double)inv_norm / nvalid[0]) : 0.f;
}

// the workspace: sites uint8 [2][total] | d2 int32 [2][total] | cnt [kBlGrid] | part [kBlGrid], nvalid | scale
struct BlWorkspace {
  size_t d2, cnt, part, scale, bytes;
  explicit BlWorkspace(size_t total) {
    d2 = up256(2 * total);
    cnt = d2 + up256(2 * total * sizeof(int32_t));
    part = cnt + up256(kBlGrid * sizeof(unsigned));
    scale = part + up256((kBlGrid + 1) * sizeof(double));
    bytes = scale + 256;
  }
};

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// host only
UNETSEG_API size_t unetseg_boundary_loss_workspace(int B, int H, int W) {
  const size_t total = B > 0 && H > 0 && W > 0 ? (size_t)B * H * W : 0;
  return BlWorkspace(total).bytes;
}

// the boundary loss of the head of this file.  out planar fp32 [B][nch][H][W]; tgt int64 [B][H][W];
// loss[0] = L (unweighted); gz [B][H][W] (may be NULL) = weight * dL/dz, added to gz when accumulate != 0;
// phi [B][H][W] (may be NULL) = the signed distance map
UNETSEG_API int unetseg_boundary_loss_fwd(const float* out, int nch, const int64_t* tgt, int B, int H, int W, int c,
                                          long ignore_index, float inv_norm, float weight, void* ws, size_t ws_bytes,
                                          float* gz, int accumulate, float* phi, float* loss, void* stream) {
  US_CHECK_ARG(out && tgt && ws && loss, "boundary_loss_fwd: null pointer");  // gz and phi may be NULL
  US_CHECK_ARG(nch == 1 || nch == 2, "boundary_loss_fwd: nch %d must be 1 or 2", nch);
  US_CHECK_ARG(B > 0 && H > 0 && W > 0, "boundary_loss_fwd: bad shape B=%d H=%d W=%d", B, H, W);
  US_CHECK_ARG(H <= kEdtMax && W <= kEdtMax, "boundary_loss_fwd: H=%d W=%d exceed %d (the distance transform's limit)",
               H, W, kEdtMax);
  US_CHECK_ARG(B <= (1 << 30) / 2, "boundary_loss_fwd: B=%d: the transform's 2 B images must fit an int", B);
  US_CHECK_ARG(ignore_index != (long)c, "boundary_loss_fwd: ignore_index %ld is the class c", ignore_index);
  US_CHECK_ARG(ws_bytes >= unetseg_boundary_loss_workspace(B, H, W), "boundary_loss_fwd: workspace too small");
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, "boundary_loss_fwd: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)H * W, total = (long)B * P;
  const BlWorkspace lay((size_t)total);
  uint8_t* base = (uint8_t*)ws;
  uint8_t* sites = base;
  int32_t* d2 = (int32_t*)(base + lay.d2);
  unsigned* cnt = (unsigned*)(base + lay.cnt);
  double* part = (double*)(base + lay.part);
  double* nvalid = part + kBlGrid;
  float* scale = (float*)(base + lay.scale);
  const int G = grid_for((total + 3) / 4, kBlGrid);
  hipLaunchKernelGGL(bl_sites_kernel, dim3(G), dim3(256), 0, st, tgt, total, c, ignore_index, sites, sites + total,
                     cnt);
  hipLaunchKernelGGL(bl_count_kernel, dim3(1), dim3(256), 0, st, cnt, G, inv_norm, nvalid, scale);
  launch_edt_sqdist(sites, 2 * B, H, W, d2, st);
  hipLaunchKernelGGL(bl_loss_kernel, dim3(G), dim3(256), 0, st, out, nch, P, tgt, (const int*)d2,
                     (const int*)(d2 + total), total, c, ignore_index, (const float*)scale, weight, gz, accumulate, phi,
                     part);
  hipLaunchKernelGGL(bl_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, G, (const double*)nvalid,
                     inv_norm, loss);
  US_LAUNCH_CHECK("boundary_loss_fwd");
  return 0;
}
