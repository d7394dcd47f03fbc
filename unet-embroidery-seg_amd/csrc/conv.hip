// The conv dispatch: the C ABI of the 2-D convolutions for NHWC activations on gfx950, host code only.
//
// Replaces every nn.Conv2d of the reference hot path:
//   model/resnet_backbone.py:19,33,126,167   model/unet_resnet.py:17,19,72,74,78
//   model/unet_plain.py:9,12,69              model/unet_attention.py:16,20,24,76
//   model/unet_multitask.py:17-18,62,64,69
//
// Argument checks, the plan builders that choose a kernel family per call, the host-only queries that
// report that choice, and calls to the families' launch_* functions: the generic kernels and the
// split-K reduce (conv_generic.h), the bf16 fast families (conv_fast.h).  No kernel lives here; the
// three GEMM views of a conv are described in conv_generic.hip, the weight packers are conv_pack.hip.
// tests/golden/conv_dispatch.json pins the rules of this file entry by entry.
#include <cstdlib>

#include "common.h"
#include "conv_fast.h"
#include "conv_generic.h"

namespace {

// bf16 fast path (conv_fast.hip) when channels are 64-aligned and every buffer fits 31-bit offsets
bool fast_tn_args(const IgemmArgs& a, FastTNArgs& f) {
  if (getenv("UNETSEG_NO_FAST")) return false;
  const long src_pix = (long)a.N * a.H * a.W;
  const long b1 = src_pix * a.ldc1 * 2, b2 = a.c2 ? src_pix * a.ldc2 * 2 : 0;
  const long bw = (long)a.Ng * a.ldw * 2;
  if (b1 >= (1L << 31) || b2 >= (1L << 31) || bw >= (1L << 31)) return false;
  f = FastTNArgs{};
  f.x1 = a.x1; f.x2 = a.c2 ? a.x2 : nullptr; f.x1_bytes = (unsigned)b1; f.x2_bytes = (unsigned)b2;
  f.ldc1b = a.ldc1 * 2; f.ldc2b = a.ldc2 * 2; f.c1 = a.c1; f.cin = a.cin;
  f.H = a.H; f.W = a.W; f.hc = a.hc; f.wc = a.wc; f.istride = a.istride;
  f.r0 = a.r0; f.rs = a.rs; f.nr = a.nr; f.dh0 = a.dh0; f.dhs = a.dhs;
  f.s0 = a.s0; f.ss = a.ss; f.ns = a.ns; f.dw0 = a.dw0; f.dws = a.dws; f.S = a.S;
  f.wt = a.wt; f.w_bytes = (unsigned)bw; f.ldwb = (int)(a.ldw * 2); f.Ng = a.Ng;
  f.ostride = a.ostride; f.ph = a.ph; f.pw = a.pw; f.OH = a.OH; f.OW = a.OW;
  f.y = a.y; f.ldy = a.ldy; f.accumulate = a.accumulate; f.bias = a.bias; f.relu = a.relu;
  f.stats = a.stats; f.stats_ld = a.stats_ld; f.M = a.M;
  f.in_sc = a.in_sc; f.in_sh = a.in_sh;
  return tn_fast_ok(f);
}

}  // namespace

// =========================================================================================
// C ABI
//
// Which kernel a conv call runs is decided once per call by a plan builder (plan_fwd, plan_dgrad,
// plan_wgrad, plan_stem).  The launching entry points and the host-only queries -- the *_config
// queries the parity tests and the benchmark's table read, the *_tile_m / *_workspace / rows queries
// that size the buffers the op layer allocates before the launch -- all consume that plan, so a query
// cannot drift from the launch it describes.  A query plans with the pointers it is not given
// replaced by a placeholder address (the dispatch only tests them for NULL) or by NULL.
// =========================================================================================

static const void* const kSomePtr = reinterpret_cast<const void*>(uintptr_t{256});
static void* const kSomeOut = const_cast<void*>(kSomePtr);

UNETSEG_API int unetseg_conv_tile_m(void) { return kBM; }

// ---- forward -------------------------------------------------------------------------------
// x = cat([x1 (c1 ch, pixel stride ldc1), x2 (c2 ch, ldc2)], C) NHWC [n,h,w,*];
// wk: dtype [cout][r][s][c1+c2]; y: NHWC [n,p,q,*] pixel stride ldy.
static IgemmArgs fwd_args(const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2, int n, int h, int w,
                          const void* wk, int cout, int r, int s, int stride, int pad) {
  const int p = (h + 2 * pad - r) / stride + 1, q = (w + 2 * pad - s) / stride + 1;
  IgemmArgs a{};
  a.x1 = x1; a.x2 = x2; a.c1 = c1; a.c2 = c2; a.ldc1 = ldc1; a.ldc2 = ldc2;
  a.N = n; a.H = h; a.W = w; a.hc = p; a.wc = q; a.istride = stride;
  a.r0 = 0; a.rs = 1; a.nr = r; a.dh0 = -pad; a.dhs = 1;
  a.s0 = 0; a.ss = 1; a.ns = s; a.dw0 = -pad; a.dws = 1;
  a.S = s; a.cin = c1 + c2; a.wt = wk; a.ldw = (long)r * s * (c1 + c2); a.Ng = cout;
  a.ostride = 1; a.ph = 0; a.pw = 0; a.OH = p; a.OW = q;
  a.M = n * p * q;
  return a;
}

// Epilogue: + bias[cout] (fp32, may be NULL), ReLU if relu, and when stats != NULL the per-row-tile
// BN partials stats[ceil(M/tile)][2][cout] (column sum, M2 about the tile mean) of the rounded y,
// tile = the plan's tile_m (the launch sets stats_ld from it).
static void set_epilogue(IgemmArgs& a, void* y, int ldy, const float* bias, int relu, float* stats) {
  a.y = y; a.ldy = ldy; a.accumulate = 0; a.bias = bias; a.relu = relu; a.stats = stats;
}

static bool first_ok(int dtype, const IgemmArgs& a, int ldy) {
  return a.x2 == nullptr && a.c2 == 0 && a.nr == a.ns && a.dh0 == a.dw0 &&
         first3x3_ok(dtype, a.c1, a.ldc1, a.c2, a.N, a.H, a.W, a.Ng, a.nr, a.ns, a.istride, -a.dh0, ldy);
}

enum { kFwdFirst3x3, kFwdFast, kFwdGeneric };
struct FwdPlan {
  int kind;
  FastTNArgs f;  // kFwdFast
  int tile_m;    // row tile of the BN partial statistics
};

// The forward dispatch: the packed-image first conv (conv_first.hip), else the bf16 fast kernels
// (conv_fast.hip / conv_halo.hip) when the shape and the buffer extents allow, else the generic kernel.
// The affine epilogue exists in the generic kernel only (the bf16 fast kernels take the BN scale folded
// into their packed weights instead).  a.ldy == 0 is unetseg_conv2d_fwd_tile_m, which is not told the
// output stride: first3x3 then assumes a dense output, and the fast kernels' output-extent tests pass.
static FwdPlan plan_fwd(int dtype, const IgemmArgs& a) {
  FwdPlan p{};
  if (!a.escale && first_ok(dtype, a, a.ldy ? a.ldy : a.Ng)) {
    p.kind = kFwdFirst3x3;
    p.tile_m = first3x3_tile_m();
  } else if (!a.escale && dtype == DT_BF16 && fast_tn_args(a, p.f)) {
    p.kind = kFwdFast;
    p.tile_m = tn_fast_tile_m(p.f);
  } else {
    p.kind = kFwdGeneric;
    p.tile_m = kBM;
  }
  return p;
}

// kCfg* code (and compile-time taps of an LDS-DMA ring) of a forward plan
static int fwd_plan_config(const FwdPlan& p, int* taps_out) {
  if (taps_out) *taps_out = 0;
  if (p.kind == kFwdFirst3x3) return kCfgFirst3x3;
  return p.kind == kFwdFast ? tn_fast_config(p.f, taps_out) : kCfgGeneric;
}

static int launch_fwd(int dtype, IgemmArgs& a, hipStream_t st) {
  FwdPlan p = plan_fwd(dtype, a);
  a.stats_ld = p.f.stats_ld = ceil_div(a.M, p.tile_m);
  if (p.kind == kFwdGeneric) return launch_generic(dtype, a, st);
  if (p.kind == kFwdFirst3x3) {
    launch_first3x3(a.x1, a.ldc1, a.wt, a.bias, a.relu, a.y, a.ldy, a.stats, a.N, a.H, a.W, st);
    US_LAUNCH_CHECK("first3x3");
    return 0;
  }
  launch_tn_fast(p.f, st);
  US_LAUNCH_CHECK("tn_fast");
  return 0;
}

// argument checks shared by unetseg_conv2d_fwd and _fwd_affine; `name` prefixes the messages
static int check_fwd_args(const char* name, int dtype, const void* x2, int c1, int ldc1, int c2, int ldc2, int n, int h,
                          int w, int cout, int r, int s, int stride, int pad, int ldy) {
  US_CHECK_CONV_GEOM(name, n, h, w, r, s, stride, pad);
  US_CHECK_ARG(cout > 0 && ldc1 >= c1 && (c2 == 0 || ldc2 >= c2), "%s: pixel strides below the channel counts", name);
  US_CHECK_ARG((c1 + c2) % 8 == 0 && c1 % 8 == 0, "%s: channels must be multiples of 8 (c1=%d c2=%d)", name, c1, c2);
  US_CHECK_ARG(c2 == 0 || x2, "%s: c2>0 needs x2", name);
  US_CHECK_ARG(ldc1 % 8 == 0 && (c2 == 0 || ldc2 % 8 == 0) && ldy >= cout, "%s: bad strides", name);
  US_CHECK_ARG(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype", name);
  return 0;
}

// Row tile of the BN partial statistics written by unetseg_conv2d_fwd for this shape:
// stats is [ceil(n*p*q / tile)][2][cout].
UNETSEG_API int unetseg_conv2d_fwd_tile_m(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w,
                                          int cout, int r, int s, int stride, int pad) {
  return plan_fwd(dtype, fwd_args(nullptr, c1, ldc1, nullptr, c2, ldc2, n, h, w, nullptr, cout, r, s, stride, pad)).tile_m;
}

// Kernel configuration unetseg_conv2d_fwd runs for this shape (kCfg* code, conv_fast.h), planned with a
// dense output and without bias / stats
UNETSEG_API int unetseg_conv2d_fwd_config(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w,
                                          int cout, int r, int s, int stride, int pad, int* taps_out) {
  IgemmArgs a = fwd_args(kSomePtr, c1, ldc1, c2 ? kSomePtr : nullptr, c2, ldc2, n, h, w, kSomePtr, cout, r, s, stride,
                         pad);
  a.ldy = cout;
  return fwd_plan_config(plan_fwd(dtype, a), taps_out);
}

UNETSEG_API int unetseg_conv2d_fwd(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2,
                                   int n, int h, int w, const void* wk, int cout, int r, int s, int stride,
                                   int pad, const float* bias, int relu, void* y, int ldy, float* stats,
                                   void* stream) {
  US_CHECK_ARG(x1 && wk && y, "conv2d_fwd: null pointer");
  if (check_fwd_args("conv2d_fwd", dtype, x2, c1, ldc1, c2, ldc2, n, h, w, cout, r, s, stride, pad, ldy)) return 1;
  IgemmArgs a = fwd_args(x1, c1, ldc1, x2, c2, ldc2, n, h, w, wk, cout, r, s, stride, pad);
  set_epilogue(a, y, ldy, bias, relu, stats);
  return launch_fwd(dtype, a, (hipStream_t)stream);
}

// Forward conv with a per-output-channel affine epilogue: y = [relu](conv(x, wk) * escale + bias)
// -- eval-mode BatchNorm applied on the fp32 accumulator (model.eval() conv -> BN -> ReLU,
// model/resnet_backbone.py:58-61, model/unet_plain.py:8-15) with the same arithmetic as the separate
// BN pass, so fp32 results match the unfolded path.  Runs the generic implicit-GEMM kernel (plan_fwd).
UNETSEG_API int unetseg_conv2d_fwd_affine(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2,
                                          int ldc2, int n, int h, int w, const void* wk, int cout, int r, int s,
                                          int stride, int pad, const float* escale, const float* bias, int relu,
                                          void* y, int ldy, void* stream) {
  US_CHECK_ARG(x1 && wk && y && escale && bias, "conv2d_fwd_affine: null pointer");
  US_CHECK_DTYPE(dtype, "conv2d_fwd_affine");
  if (check_fwd_args("conv2d_fwd_affine", dtype, x2, c1, ldc1, c2, ldc2, n, h, w, cout, r, s, stride, pad, ldy)) return 1;
  IgemmArgs a = fwd_args(x1, c1, ldc1, x2, c2, ldc2, n, h, w, wk, cout, r, s, stride, pad);
  set_epilogue(a, y, ldy, bias, relu, nullptr);
  a.escale = escale;
  return launch_fwd(dtype, a, (hipStream_t)stream);
}

// Forward 1x1 / stride-1 conv whose input is the BN-ReLU output of the producer, never
// materialised: x1 holds the BN input z and the conv stages relu(z * in_sc[c] + in_sh[c]) (the
// bn_apply arithmetic, rounded to bf16) between its global loads and LDS stores -- the ResNet
// bottleneck's bn2 -> ReLU -> conv3 (model/resnet_backbone.py:58-62).  bf16 only, single source,
// register-staged fast configurations; epilogue as unetseg_conv2d_fwd (bias, ReLU, BN partials of
// its own output; the prologue moves a shape between configurations of one row tile only, so the
// tile is unetseg_conv2d_fwd_tile_m's for the 1x1 shape).
static IgemmArgs bnrelu_in_args(const void* x1, int c1, int ldc1, int n, int h, int w, const void* wk, int cout,
                                const float* in_sc, const float* in_sh) {
  IgemmArgs a = fwd_args(x1, c1, ldc1, nullptr, 0, 0, n, h, w, wk, cout, 1, 1, 1, 0);
  a.in_sc = in_sc; a.in_sh = in_sh;
  return a;
}

UNETSEG_API int unetseg_conv2d_fwd_bnrelu_in(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w,
                                             const void* wk, int cout, const float* in_sc, const float* in_sh,
                                             const float* bias, int relu, void* y, int ldy, float* stats,
                                             void* stream) {
  US_CHECK_ARG(dtype == DT_BF16, "conv2d_fwd_bnrelu_in: bf16 only");
  US_CHECK_ARG(x1 && wk && y && in_sc && in_sh, "conv2d_fwd_bnrelu_in: null pointer");
  US_CHECK_ARG(c1 % 64 == 0 && ldc1 % 8 == 0 && ldy >= cout && c1 <= 2048, "conv2d_fwd_bnrelu_in: bad channels");
  IgemmArgs a = bnrelu_in_args(x1, c1, ldc1, n, h, w, wk, cout, in_sc, in_sh);
  set_epilogue(a, y, ldy, bias, relu, stats);
  FwdPlan p = plan_fwd(dtype, a);
  US_CHECK_ARG(p.kind == kFwdFast, "conv2d_fwd_bnrelu_in: shape has no fast path");
  p.f.stats_ld = ceil_div(a.M, p.tile_m);
  US_CHECK_ARG(launch_tn_fast(p.f, (hipStream_t)stream) == 0, "conv2d_fwd_bnrelu_in: no register-staged tile");
  US_LAUNCH_CHECK("tn_fast_bnrelu_in");
  return 0;
}

// configuration unetseg_conv2d_fwd_bnrelu_in runs for this shape (host only; -1: no fast path)
UNETSEG_API int unetseg_conv2d_fwd_bnrelu_in_config(int dtype, int c1, int ldc1, int n, int h, int w, int cout) {
  static const float kOne = 1.f;
  IgemmArgs a = bnrelu_in_args(kSomePtr, c1, ldc1, n, h, w, kSomePtr, cout, &kOne, &kOne);
  a.ldy = cout;
  const FwdPlan p = plan_fwd(dtype, a);
  return p.kind == kFwdFast ? tn_fast_config(p.f, nullptr) : -1;
}

// The decoder's last 3x3 conv (64 -> 64, stride 1, pad 1, bias, ReLU; model/unet_resnet.py:77-78
// up_conv[3..4]) with the model's 1x1 head (model/unet_resnet.py:79 `final`, 64 -> head_k logits,
// head_k = 1 or 2) fused into its epilogue: y as unetseg_conv2d_fwd, plus fp32 planar NCHW logits
// computed from the stored (rounded) y -- the separate head pass (unetseg_pw_small_fwd) would
// re-read all of y.  bf16, halo path only (unetseg_conv2d_fwd_head_ok).
static bool head_args(const void* x1, int ldc1, int n, int h, int w, const void* wk, const float* bias, void* y,
                      int ldy, FastTNArgs& f) {
  IgemmArgs a = fwd_args(x1, 64, ldc1, nullptr, 0, 0, n, h, w, wk, 64, 3, 3, 1, 1);
  set_epilogue(a, y, ldy, bias, 1, nullptr);
  return fast_tn_args(a, f) && halo3_ok(f);
}

UNETSEG_API int unetseg_conv2d_fwd_head_ok(int dtype, int ldc1, int n, int h, int w, int ldy, int head_k) {
  FastTNArgs f;
  return dtype == DT_BF16 && (head_k == 1 || head_k == 2) && ldy >= 64 && ldc1 % 8 == 0 &&
         head_args(kSomePtr, ldc1, n, h, w, kSomePtr, nullptr, nullptr, ldy, f);
}

UNETSEG_API int unetseg_conv2d_fwd_head(int dtype, const void* x1, int ldc1, int n, int h, int w, const void* wk,
                                        const float* bias, void* y, int ldy, int head_k, const float* head_w,
                                        const float* head_b, float* logits, void* stream) {
  US_CHECK_ARG(x1 && wk && bias && y && head_w && head_b && logits, "conv2d_fwd_head: null pointer");
  US_CHECK_ARG(unetseg_conv2d_fwd_head_ok(dtype, ldc1, n, h, w, ldy, head_k),
               "conv2d_fwd_head: needs bf16, 64 -> 64 channels on the halo path and head_k 1 or 2");
  FastTNArgs f;
  head_args(x1, ldc1, n, h, w, wk, bias, y, ldy, f);
  f.head_w = head_w; f.head_b = head_b; f.head_y = logits; f.head_k = head_k;
  US_CHECK_ARG(launch_halo3(f, (hipStream_t)stream) == 0, "conv2d_fwd_head: launch refused");
  US_LAUNCH_CHECK("conv2d_fwd_head");
  return 0;
}

// 3x3 conv, 64 -> 64 channels, + bias + ReLU (the decoder's 512^2 up_conv conv1,
// model/unet_resnet.py:90-97) that also stores its output's ReLU mask as bits, mbits[pixel][8] (bit e
// of byte b = channel 8b + e > 0): the consumer conv's data gradient masks with them (post 4 of
// unetseg_conv2d_dgrad_post) instead of re-reading the 64-channel activation.  mbits == NULL: returns 1
// when the shape has this kernel (the halo path), else 0; nothing is launched.
UNETSEG_API int unetseg_conv2d_fwd_mask(int dtype, const void* x1, int ldc1, int n, int h, int w, const void* wk,
                                        const float* bias, void* y, int ldy, unsigned char* mbits, void* stream) {
  FastTNArgs f;
  const bool ok = dtype == DT_BF16 && ldy >= 64 && ldy % 8 == 0 && ldc1 % 8 == 0 &&
                  head_args(x1 ? x1 : kSomePtr, ldc1, n, h, w, wk ? wk : kSomePtr, bias, y, ldy, f);
  if (!mbits) return ok ? 1 : 0;
  US_CHECK_ARG(ok, "conv2d_fwd_mask: needs bf16, 64 -> 64 channels on the halo path");
  US_CHECK_ARG(x1 && wk && bias && y, "conv2d_fwd_mask: null pointer");
  f.mbits_out = mbits;
  US_CHECK_ARG(launch_halo3(f, (hipStream_t)stream) == 0, "conv2d_fwd_mask: launch refused");
  US_LAUNCH_CHECK("conv2d_fwd_mask");
  return 0;
}

// ---- data gradient -------------------------------------------------------------------------
// dy: NHWC [n,p,q,cout] (pixel stride ldy); wt: dtype [cin][r][s][cout]; dx: NHWC [n,h,w,*] pixel
// stride ldx.  A stride-2 data gradient is one GEMM per output-parity class (ph, pw): the taps of the
// filter that reach the pixels of that parity.  Returns false for a class without pixels.
static bool dgrad_class(const void* dy, int ldy, int n, int p, int q, const void* wt, int cout, int cin, int r, int s,
                        int stride, int pad, void* dx, int ldx, int h, int w, int ph, int pw, IgemmArgs& a) {
  a = IgemmArgs{};
  a.x1 = dy; a.x2 = nullptr; a.c1 = cout; a.c2 = 0; a.ldc1 = ldy; a.ldc2 = 0;
  a.N = n; a.H = p; a.W = q; a.istride = 1;
  a.hc = (h - ph + stride - 1) / stride; a.wc = (w - pw + stride - 1) / stride;
  if (a.hc <= 0 || a.wc <= 0) return false;
  a.r0 = (ph + pad) % stride; a.rs = stride; a.nr = (r - a.r0 + stride - 1) / stride;
  a.dh0 = (ph + pad - a.r0) / stride; a.dhs = -1;
  a.s0 = (pw + pad) % stride; a.ss = stride; a.ns = (s - a.s0 + stride - 1) / stride;
  a.dw0 = (pw + pad - a.s0) / stride; a.dws = -1;
  if (a.nr < 0) a.nr = 0;
  if (a.ns <= 0) { a.ns = 1; a.nr = 0; }
  a.S = s; a.cin = cout; a.wt = wt; a.ldw = (long)r * s * cout; a.Ng = cin;
  a.ostride = stride; a.ph = ph; a.pw = pw; a.OH = h; a.OW = w;
  a.y = dx; a.ldy = ldx; a.accumulate = 0; a.bias = nullptr; a.relu = 0;
  a.M = n * a.hc * a.wc; a.stats = nullptr;
  return a.M > 0;
}

struct DgradClass {
  IgemmArgs a;
  FastTNArgs f;  // when fast
  bool fast;     // on the bf16 fast kernels (else the generic kernel, which has no post-op epilogue)
  bool merged;   // one of the classes of the merged launch
  int rows;      // partial rows (ppart) a fused post-op writes for this class
  int slot;      // ph * stride + pw
};

struct DgradPlan {
  DgradClass c[4];
  int n = 0;             // classes launched, in (ph, pw) order
  bool all_fast = true;
  int merged_bm = -1;    // row tile of the merged launch (64 / 128), -1: none
  int rows = 0;          // sum of the classes' partial rows
};

// The data-gradient dispatch.  `post` (may be NULL) carries the fused post-op's fields (post, aux,
// ld_aux, psc, psh, pmean, pinv, mbits): they take part in the choice (the halo path bounds the aux
// extent).  A parity class no tap reaches (e.g. odd pixels of a 1x1 stride-2 conv) contributes zeros:
// written when the call initialises dx, dropped when it accumulates.
// The parity classes with taps run as one merged launch (launch_tn_multi) when every class of the call
// is fast and at least two of them share a register-staged tile; a class no tap reaches only writes
// zeros and keeps its own launch.  Merged classes share the launch's row tile, and their partial rows
// follow it.
static void plan_dgrad(DgradPlan& pl, int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt, int cout,
                       int cin, int r, int s, int stride, int pad, void* dx, int ldx, int h, int w, int accumulate,
                       const FastTNArgs* post) {
  for (int ph = 0; ph < stride; ++ph)
    for (int pw = 0; pw < stride; ++pw) {
      DgradClass& c = pl.c[pl.n];
      if (!dgrad_class(dy, ldy, n, p, q, wt, cout, cin, r, s, stride, pad, dx, ldx, h, w, ph, pw, c.a)) continue;
      if (c.a.nr == 0 && accumulate) continue;
      c.a.accumulate = accumulate;
      c.slot = ph * stride + pw;
      c.merged = false;
      c.rows = 0;
      c.fast = dtype == DT_BF16 && fast_tn_args(c.a, c.f);
      if (c.fast && post) {
        c.f.post = post->post; c.f.aux = post->aux; c.f.ld_aux = post->ld_aux; c.f.mbits = post->mbits;
        c.f.psc = post->psc; c.f.psh = post->psh; c.f.pmean = post->pmean; c.f.pinv = post->pinv;
      }
      pl.all_fast = pl.all_fast && c.fast;
      ++pl.n;
    }
  if (!pl.all_fast) return;
  FastTNArgs m[4];
  int k = 0;
  for (int i = 0; i < pl.n; ++i)
    if (pl.c[i].f.nr > 0) m[k++] = pl.c[i].f;
  pl.merged_bm = tn_multi_tile_m(m, k);
  for (int i = 0; i < pl.n; ++i) {
    DgradClass& c = pl.c[i];
    c.merged = pl.merged_bm > 0 && c.f.nr > 0;
    c.rows = c.merged ? ceil_div(c.f.M, pl.merged_bm) : tn_fast_post_rows(c.f);
    pl.rows += c.rows;
  }
}

// the classes of a plan in order, the merged ones as one launch after the others
static int launch_dgrad(const char* name, int dtype, const DgradPlan& pl, hipStream_t st) {
  FastTNArgs m[4];
  int k = 0;
  for (int i = 0; i < pl.n; ++i) {
    const DgradClass& c = pl.c[i];
    if (c.merged) {
      m[k++] = c.f;
    } else if (c.fast) {
      US_CHECK_ARG(launch_tn_fast(c.f, st) == 0, "%s: no fused kernel", name);
      US_LAUNCH_CHECK("tn_fast");
    } else if (int rc = launch_generic(dtype, c.a, st)) {
      return rc;
    }
  }
  if (k > 0) {
    US_CHECK_ARG(launch_tn_multi(m, k, st) == 0, "%s: merged launch refused", name);
    US_LAUNCH_CHECK("conv2d_dgrad (merged parity classes)");
  }
  return 0;
}

// dx written, or added to when accumulate
UNETSEG_API int unetseg_conv2d_dgrad(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt,
                                     int cout, int cin, int r, int s, int stride, int pad, void* dx, int ldx,
                                     int h, int w, int accumulate, void* stream) {
  US_CHECK_ARG(dy && wt && dx, "conv2d_dgrad: null pointer");
  US_CHECK_DTYPE(dtype, "conv2d_dgrad");
  US_CHECK_CONV_GEOM("conv2d_dgrad", n, h, w, r, s, stride, pad);
  US_CHECK_ARG(cin > 0 && cout > 0 && ldy >= cout && ldx >= cin, "conv2d_dgrad: bad channel counts / strides");
  US_CHECK_ARG(cout % 8 == 0 && ldy % 8 == 0, "conv2d_dgrad: cout/ldy must be multiples of 8");
  US_CHECK_ARG(stride == 1 || stride == 2, "conv2d_dgrad: stride must be 1 or 2");
  US_CHECK_ARG(p == (h + 2 * pad - r) / stride + 1 && q == (w + 2 * pad - s) / stride + 1, "conv2d_dgrad: shape mismatch");
  DgradPlan pl;
  plan_dgrad(pl, dtype, dy, ldy, n, p, q, wt, cout, cin, r, s, stride, pad, dx, ldx, h, w, accumulate, nullptr);
  return launch_dgrad("conv2d_dgrad", dtype, pl, (hipStream_t)stream);
}

// Data gradient with a post-op fused into the epilogue (bf16 fast path only).  The produced
// gradient belongs to a tensor that was the output of a ReLU (post 1: aux = that output; post 4: aux =
// its mask bits, unetseg_conv2d_fwd_mask -- the 64-channel halo kernel only) or of a BN-ReLU (post 2:
// aux = the BN input z, psc/psh its affine, pmean/pinv its batch statistics); what is stored is the
// masked gradient d, and part[row][2][cin] receives per-row-tile column sums of d and (post 2) of
// d * (z - mean) * inv -- the first pass of the ReLU bias / BN backward.
// part == NULL: returns the number of partial rows for this shape, or -1 if the shape has no fused
// path (the caller then runs the plain dgrad and the separate reduction): every parity class must take
// the fast path.
UNETSEG_API int unetseg_conv2d_dgrad_post(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt,
                                          int cout, int cin, int r, int s, int stride, int pad, void* dx, int ldx,
                                          int h, int w, int post, const void* aux, int ld_aux, const float* psc,
                                          const float* psh, const float* pmean, const float* pinv, float* part,
                                          int rows, void* stream) {
  US_CHECK_ARG(post == 1 || post == 2 || post == 4,
               "conv2d_dgrad_post: post must be 1 (ReLU), 2 (BN-ReLU) or 4 (ReLU from mask bits)");
  if (dtype != DT_BF16 || stride < 1 || stride > 2 || cout % 8 || ldy % 8) return -1;
  FastTNArgs po{};
  po.post = post; po.aux = aux; po.ld_aux = ld_aux; po.psc = psc; po.psh = psh; po.pmean = pmean; po.pinv = pinv;
  if (post == 4) po.mbits = static_cast<const unsigned char*>(aux);
  DgradPlan pl;
  plan_dgrad(pl, dtype, dy, ldy, n, p, q, wt, cout, cin, r, s, stride, pad, dx, ldx, h, w, 0, &po);
  if (!pl.all_fast) return -1;
  for (int i = 0; i < pl.n; ++i)
    if (post == 4 && tn_fast_config(pl.c[i].f, nullptr) != kCfgHalo) return -1;
  if (!part) return pl.rows;
  US_CHECK_ARG(dy && wt && dx && aux, "conv2d_dgrad_post: null pointer");
  US_CHECK_ARG(rows == pl.rows, "conv2d_dgrad_post: rows %d != %d", rows, pl.rows);
  US_CHECK_ARG(post != 2 || (psc && psh && pmean && pinv), "conv2d_dgrad_post: BN post needs its coefficients");
  int off = 0;
  for (int i = 0; i < pl.n; ++i) {
    pl.c[i].f.ppart = part + (long)off * 2 * cin;
    off += pl.c[i].rows;
  }
  return launch_dgrad("conv2d_dgrad_post", dtype, pl, (hipStream_t)stream);
}

// Data gradient of a 1x1 stride-1 conv accumulated onto the residual gradient already in dx, with the
// residual-BN backward's first pass in the epilogue (post 3, conv_fast.h): dx = mask * bf16(dgrad + dx),
// mask = the block output's packed ReLU bits (unetseg_bn_apply_mask), part[tile][2 or 3][cin] = sum d,
// sum d * xhat1 [, sum d * xhat2] with xhat_b = (y_b - mean_b) * inv_b.  Replaces the separate
// unetseg_bn_bwd_reduce pass over dx of model/resnet_backbone.py:110-113 (bn3 + residual add + ReLU)
// when this conv (the next block's conv1, :88) is the last consumer to deliver its gradient.
// part == NULL: returns the partial rows a call writes, or 0 when the shape has no fused kernel.
UNETSEG_API int unetseg_conv2d_dgrad_post_res(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt,
                                              int cout, int cin, void* dx, int ldx, const void* y1, int ld1,
                                              const float* mean1, const float* inv1, const unsigned char* mbits,
                                              const void* y2, int ld2, const float* mean2, const float* inv2,
                                              float* part, int rows, void* stream) {
  if (dtype != DT_BF16 || n <= 0 || p <= 0 || q <= 0 || cout % 8 || ldy % 8 || cin % 8 || ldx < cin || ldx % 8)
    return 0;
  // not accumulate: the residual gradient is added in registers before the mask
  FastTNArgs po{};
  po.post = 3;
  DgradPlan pl;
  plan_dgrad(pl, dtype, dy ? dy : kSomePtr, ldy, n, p, q, wt ? wt : kSomePtr, cout, cin, 1, 1, 1, 0, dx ? dx : kSomeOut,
             ldx, p, q, 0, &po);
  if (pl.n != 1 || !pl.all_fast || !tn_fast_post_res_ok(pl.c[0].f)) return 0;
  if (!part) return pl.rows;
  US_CHECK_ARG(dy && wt && dx && y1 && mean1 && inv1 && mbits, "conv2d_dgrad_post_res: null pointer");
  US_CHECK_ARG(!y2 || (mean2 && inv2 && ld2 >= cin), "conv2d_dgrad_post_res: second branch needs y2, mean2, inv2");
  US_CHECK_ARG(ld1 >= cin, "conv2d_dgrad_post_res: ld1 < cin");
  US_CHECK_ARG(rows == pl.rows, "conv2d_dgrad_post_res: rows %d != %d", rows, pl.rows);
  FastTNArgs& f = pl.c[0].f;
  f.aux = y1; f.ld_aux = ld1; f.pmean = mean1; f.pinv = inv1; f.mbits = mbits;
  f.aux2 = y2; f.ld_aux2 = ld2; f.pmean2 = mean2; f.pinv2 = inv2;
  f.ppart = part;
  return launch_dgrad("conv2d_dgrad_post_res", dtype, pl, (hipStream_t)stream);
}

// Configuration of each output-parity class of unetseg_conv2d_dgrad (initialising dx) / _dgrad_post:
// cfg_out[ph * stride + pw] (kCfg* codes; -1 = class not launched), taps_out likewise (may be NULL).
// Returns the number of classes launched.
UNETSEG_API int unetseg_conv2d_dgrad_config(int dtype, int ldy, int n, int p, int q, int cout, int cin, int r, int s,
                                            int stride, int pad, int ldx, int h, int w, int* cfg_out, int* taps_out) {
  US_CHECK_ARG(cfg_out && (stride == 1 || stride == 2), "conv2d_dgrad_config: bad args");
  for (int k = 0; k < stride * stride; ++k) {
    cfg_out[k] = -1;
    if (taps_out) taps_out[k] = 0;
  }
  DgradPlan pl;
  plan_dgrad(pl, dtype, kSomePtr, ldy, n, p, q, kSomePtr, cout, cin, r, s, stride, pad, kSomeOut, ldx, h, w, 0, nullptr);
  for (int i = 0; i < pl.n; ++i) {
    const DgradClass& c = pl.c[i];
    int taps = 0;
    if (c.merged) cfg_out[c.slot] = pl.merged_bm == 64 ? kCfgMulti64 : kCfgMulti128;
    else cfg_out[c.slot] = c.fast ? tn_fast_config(c.f, &taps) : kCfgGeneric;
    if (taps_out) taps_out[c.slot] = taps;
  }
  return pl.n;
}

// ---- weight gradient -----------------------------------------------------------------------
// x = cat([x1, x2]) NHWC [n,h,w,*]; dy NHWC [n,p,q,cout] (pixel stride ldy); dw: fp32
// [cout][dw_c][r][s] (PyTorch layout; dw_c <= c1+c2 drops zero-padded input channels), written or
// accumulated.  Every family writes split-K slabs ws[split][cout][r*s*cin] that the deterministic
// reduce (conv_wgrad_reduce.hip) sums into dw; ws: fp32 workspace of unetseg_conv2d_wgrad_workspace() bytes.

// shape test of the fast bf16 family (conv_fast.hip; split rule: wgrad_fast_splits)
static bool wgrad_fast_eligible(int dtype, int cin, int cout) {
  return dtype == DT_BF16 && !getenv("UNETSEG_NO_FAST") && cin % 8 == 0 && cout % 64 == 0;
}

// shape test of the halo wgrad path (3x3, stride 1, pad 1, output grid == input grid; split rule:
// halo3_wgrad_splits on the fields filled here)
static bool halo_wgrad_args(int dtype, int c1, int cin, int n, int h, int w, int cout, int r, int s, int p, int q,
                            HaloWgradArgs& hw) {
  if (dtype != DT_BF16 || getenv("UNETSEG_NO_FAST") || r != 3 || s != 3 || p != h || q != w) return false;
  hw.c1 = c1; hw.cin = cin; hw.N = n; hw.H = h; hw.W = w; hw.Cout = cout;
  return halo3_wgrad_ok(hw);
}

// The query knows neither strides, pads nor pixel strides: the largest of the three families' slabs.
UNETSEG_API size_t unetseg_conv2d_wgrad_workspace(int dtype, int n, int p, int q, int cout, int cin, int r, int s) {
  const int Ng = r * s * cin;
  const long kpix = (long)n * p * q;
  int splits = wgrad_generic_splits(dtype, cout, Ng, kpix);
  if (wgrad_fast_eligible(dtype, cin, cout)) splits = std::max(splits, wgrad_fast_splits(cout, Ng, kpix));
  HaloWgradArgs hw{};
  if (halo_wgrad_args(dtype, cin, cin, n, p, q, cout, r, s, p, q, hw)) splits = std::max(splits, halo3_wgrad_splits(hw));
  return (size_t)splits * cout * Ng * sizeof(float);
}

struct WgradPlan {
  int kind;    // kWg* code (conv_fast.h)
  int splits;  // split-K slabs
  HaloWgradArgs hw;  // kWgHalo
  FastWgradArgs f;   // the fast family (kWgFast* / kWgRing*)
  WgradArgs a;       // kWgGeneric
};

// The weight-gradient dispatch: halo (3x3 / stride 1 / pad 1), else the fast bf16 family, else the
// generic kernel.  The halo and fast kernels address their operands with 32-bit byte offsets, so both
// need every buffer below 2^31 bytes.  in_sc / in_sh (may be NULL): the BN-ReLU input prologue of
// unetseg_conv2d_wgrad_bnrelu_in, which only the fast family has.
static void plan_wgrad(WgradPlan& pl, int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2,
                       int n, int h, int w, const void* dy, int ldy, int cout, int r, int s, int stride, int pad,
                       float* ws, const float* in_sc, const float* in_sh) {
  const int p = (h + 2 * pad - r) / stride + 1, q = (w + 2 * pad - s) / stride + 1;
  const int cin = c1 + c2, Ng = r * s * cin;
  const long kpix = (long)n * p * q, src_pix = (long)n * h * w;
  const long b1 = src_pix * ldc1 * 2, b2 = c2 ? src_pix * ldc2 * 2 : 0, bdy = kpix * ldy * 2;
  const bool fit = b1 < (1L << 31) && b2 < (1L << 31) && bdy < (1L << 31);
  pl.hw = HaloWgradArgs{};
  if (fit && !in_sc && stride == 1 && pad == 1 && halo_wgrad_args(dtype, c1, cin, n, h, w, cout, r, s, p, q, pl.hw)) {
    HaloWgradArgs& hw = pl.hw;
    hw.x1 = x1; hw.x2 = c2 ? x2 : nullptr; hw.x1_bytes = (unsigned)b1; hw.x2_bytes = (unsigned)b2;
    hw.ldc1b = ldc1 * 2; hw.ldc2b = ldc2 * 2; hw.dy = dy; hw.dy_bytes = (unsigned)bdy; hw.ldyb = ldy * 2;
    hw.ws = ws;
    pl.kind = kWgHalo;
    pl.splits = halo3_wgrad_splits(hw);
  } else if (fit && wgrad_fast_eligible(dtype, cin, cout) && c1 % 8 == 0) {
    FastWgradArgs& f = pl.f = FastWgradArgs{};
    f.x1 = x1; f.x2 = c2 ? x2 : nullptr; f.x1_bytes = (unsigned)b1; f.x2_bytes = (unsigned)b2;
    f.ldc1b = ldc1 * 2; f.ldc2b = ldc2 * 2; f.c1 = c1; f.cin = cin;
    f.H = h; f.W = w; f.P = p; f.Q = q; f.stride = stride; f.pad = pad; f.padw = pad; f.S = s;
    f.dy = dy; f.dy_bytes = (unsigned)bdy; f.ldyb = ldy * 2; f.Cout = cout; f.Ng = Ng; f.Kpix = kpix;
    f.ws = ws; f.in_sc = in_sc; f.in_sh = in_sh;
    pl.kind = wgrad_fast_kind(f);
    pl.splits = wgrad_fast_splits(cout, Ng, kpix);
  } else {
    WgradArgs& a = pl.a = WgradArgs{};
    a.x1 = x1; a.x2 = x2; a.c1 = c1; a.c2 = c2; a.ldc1 = ldc1; a.ldc2 = ldc2;
    a.N = n; a.H = h; a.W = w; a.P = p; a.Q = q; a.stride = stride; a.pad = pad; a.R = r; a.S = s;
    a.dy = dy; a.ldy = ldy; a.Cout = cout; a.cin = cin; a.Ng = Ng; a.Kpix = kpix; a.ws = ws;
    pl.kind = kWgGeneric;
    pl.splits = wgrad_generic_splits(dtype, cout, Ng, kpix);
  }
}

// the planned kernel into the slabs, then the split-K reduce into the first dw_rows rows of dw
static int launch_wgrad(const char* name, int dtype, const WgradPlan& pl, int cout, int cin, int taps, float* ws,
                        size_t ws_bytes, float* dw, int dw_c, int accumulate, int dw_rows, hipStream_t st) {
  US_CHECK_ARG(ws_bytes >= (size_t)pl.splits * cout * taps * cin * sizeof(float), "%s: workspace too small", name);
  if (pl.kind == kWgHalo) {
    launch_halo3_wgrad(pl.hw, pl.splits, st);
    US_LAUNCH_CHECK("halo3_wgrad");
  } else if (pl.kind != kWgGeneric) {
    launch_wgrad_fast(pl.f, pl.splits, st);
    US_LAUNCH_CHECK("wgrad_fast");
  } else {
    launch_wgrad_generic(dtype, pl.a, pl.splits, st);
    US_LAUNCH_CHECK("wgrad");
  }
  launch_wgrad_reduce(ws, pl.splits, cout, cin, taps, dw, dw_c, accumulate, st, dw_rows);
  US_LAUNCH_CHECK("wgrad_reduce");
  return 0;
}

static int conv2d_wgrad_impl(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2, int n, int h,
                             int w, const void* dy, int ldy, int cout, int r, int s, int stride, int pad, float* ws,
                             size_t ws_bytes, float* dw, int dw_c, int accumulate, int dw_rows, void* stream) {
  US_CHECK_ARG(x1 && dy && ws && dw, "conv2d_wgrad: null pointer");
  US_CHECK_DTYPE(dtype, "conv2d_wgrad");
  US_CHECK_CONV_GEOM("conv2d_wgrad", n, h, w, r, s, stride, pad);
  // dw_c <= cin: the padded input channels of the first conv (3 -> 8) have no weight columns
  US_CHECK_ARG(cout > 0 && ldc1 >= c1 && (c2 == 0 || ldc2 >= c2) && ldy >= cout && dw_c > 0 && dw_c <= c1 + c2,
               "conv2d_wgrad: bad channel counts / strides");
  US_CHECK_ARG((c1 + c2) % 8 == 0 && c1 % 8 == 0 && cout % 8 == 0 && ldy % 8 == 0, "conv2d_wgrad: channel counts must be multiples of 8");
  WgradPlan pl;
  plan_wgrad(pl, dtype, x1, c1, ldc1, x2, c2, ldc2, n, h, w, dy, ldy, cout, r, s, stride, pad, ws, nullptr, nullptr);
  return launch_wgrad("conv2d_wgrad", dtype, pl, cout, c1 + c2, r * s, ws, ws_bytes, dw, dw_c, accumulate, dw_rows,
                      (hipStream_t)stream);
}

UNETSEG_API int unetseg_conv2d_wgrad(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2,
                                     int n, int h, int w, const void* dy, int ldy, int cout, int r, int s,
                                     int stride, int pad, float* ws, size_t ws_bytes, float* dw, int dw_c,
                                     int accumulate, void* stream) {
  return conv2d_wgrad_impl(dtype, x1, c1, ldc1, x2, c2, ldc2, n, h, w, dy, ldy, cout, r, s, stride, pad, ws, ws_bytes,
                           dw, dw_c, accumulate, cout, stream);
}

// The same with dW holding only the first dw_rows of the cout GEMM rows: a padded-K conv (cout = the
// 64-padded output channels, whose padded dY columns are zero) accumulates straight into its
// dw_rows-row gradient, without a padded fp32 copy and an add pass.
UNETSEG_API int unetseg_conv2d_wgrad_rows(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w,
                                          const void* dy, int ldy, int cout, int r, int s, int stride, int pad,
                                          float* ws, size_t ws_bytes, float* dw, int dw_c, int accumulate, int dw_rows,
                                          void* stream) {
  US_CHECK_ARG(dw_rows > 0 && dw_rows <= cout, "conv2d_wgrad_rows: bad dw_rows %d (cout %d)", dw_rows, cout);
  return conv2d_wgrad_impl(dtype, x1, c1, ldc1, nullptr, 0, 0, n, h, w, dy, ldy, cout, r, s, stride, pad, ws, ws_bytes,
                           dw, dw_c, accumulate, dw_rows, stream);
}

// Weight gradient of unetseg_conv2d_fwd_bnrelu_in's conv: X = relu(x1 * in_sc + in_sh) staged on the
// fly (fast bf16 family only), then the usual deterministic split-K reduce into dw (fp32 [cout][dw_c],
// (+)= with accumulate).
UNETSEG_API int unetseg_conv2d_wgrad_bnrelu_in(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w,
                                               const void* dy, int ldy, int cout, const float* in_sc,
                                               const float* in_sh, float* ws, size_t ws_bytes, float* dw, int dw_c,
                                               int accumulate, void* stream) {
  US_CHECK_ARG(dtype == DT_BF16, "conv2d_wgrad_bnrelu_in: bf16 only");
  US_CHECK_ARG(x1 && dy && ws && dw && in_sc && in_sh, "conv2d_wgrad_bnrelu_in: null pointer");
  US_CHECK_ARG(c1 % 8 == 0 && cout % 64 == 0 && ldy % 8 == 0 && dw_c > 0 && dw_c <= c1,
               "conv2d_wgrad_bnrelu_in: bad channels");
  WgradPlan pl;
  plan_wgrad(pl, dtype, x1, c1, ldc1, nullptr, 0, 0, n, h, w, dy, ldy, cout, 1, 1, 1, 0, ws, in_sc, in_sh);
  US_CHECK_ARG(pl.kind != kWgGeneric, "conv2d_wgrad_bnrelu_in: shape has no fast path");
  return launch_wgrad("conv2d_wgrad_bnrelu_in", dtype, pl, cout, c1, 1, ws, ws_bytes, dw, dw_c, accumulate, -1,
                      (hipStream_t)stream);
}

// Kernel unetseg_conv2d_wgrad runs for this shape: kWg* code; *splits_out = split-K slabs (summed by
// wgrad_reduce_kernel).
UNETSEG_API int unetseg_conv2d_wgrad_config(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w,
                                            int ldy, int cout, int r, int s, int stride, int pad, int* splits_out) {
  WgradPlan pl;
  plan_wgrad(pl, dtype, kSomePtr, c1, ldc1, c2 ? kSomePtr : nullptr, c2, ldc2, n, h, w, kSomePtr, ldy, cout, r, s, stride,
             pad, nullptr, nullptr, nullptr);
  if (splits_out) *splits_out = pl.splits;
  return pl.kind;
}

// =========================================================================================
// ResNet stem (model/resnet_backbone.py:126-131: conv 7x7 / stride 2 / pad 3, 3 -> 64, no bias)
// on the fast implicit-GEMM kernels.  The input is packed width-padded: xp bf16 [N][H][W+8][8]
// with image column w at packed column w+3 (zeros around, channels 3..7 zero).  For output
// column q and filter row r the 8 taps of the row (7 real + 1 zero-weight) then read 8
// consecutive packed pixels = 128 contiguous bytes, so the conv is a GEMM with K = 7 rows x 64
// (8 taps x 8 channels): one 64-wide K step per filter row, no per-tap column checks.
// wk: bf16 [K][7][64] with wk[k][r][s*8+c] = w[k][c][r][s] (s < 7, c < C), else 0.
// =========================================================================================
namespace {

IgemmArgs stem_args(const void* xp, int n, int h, int w, const void* wk, int K) {
  IgemmArgs a{};
  a.x1 = xp; a.x2 = nullptr; a.c1 = 64; a.c2 = 0; a.ldc1 = 8; a.ldc2 = 0;
  a.N = n; a.H = h; a.W = w + 8;
  a.hc = (h + 6 - 7) / 2 + 1; a.wc = (w + 6 - 7) / 2 + 1; a.istride = 2;
  a.r0 = 0; a.rs = 1; a.nr = 7; a.dh0 = -3; a.dhs = 1;
  a.s0 = 0; a.ss = 1; a.ns = 1; a.dw0 = 0; a.dws = 1;
  a.S = 1; a.cin = 64; a.wt = wk; a.ldw = 7 * 64; a.Ng = K;
  a.ostride = 1; a.ph = 0; a.pw = 0; a.OH = a.hc; a.OW = a.wc;
  a.M = n * a.hc * a.wc;
  return a;
}

FastWgradArgs stem_wgrad_args(const void* xp, int n, int h, int w, const void* dy, int ldy, int K) {
  const int p = (h + 6 - 7) / 2 + 1, q = (w + 6 - 7) / 2 + 1;
  FastWgradArgs f{};
  f.x1 = xp; f.x2 = nullptr; f.x1_bytes = (unsigned)((long)n * h * (w + 8) * 16); f.x2_bytes = 0;
  f.ldc1b = 16; f.ldc2b = 0; f.c1 = 64; f.cin = 64;
  f.H = h; f.W = w + 8; f.P = p; f.Q = q; f.stride = 2; f.pad = 3; f.padw = 0; f.S = 1;
  f.dy = dy; f.dy_bytes = (unsigned)((long)n * p * q * ldy * 2); f.ldyb = ldy * 2; f.Cout = K; f.Ng = 7 * 64;
  f.Kpix = (long)n * p * q;
  return f;
}

}  // namespace

enum { kStemHalo, kStemFast, kStemNone };
struct StemPlan {
  int kind;
  FastTNArgs f;  // kStemFast
};

// The stem's forward dispatch: the persistent-halo stem kernel (conv_halo.hip) when the output tiles
// into 16 x 32 pixels, else a TN tile of the fast kernels, else the shape is unsupported.
// The halo kernel always writes BN statistics, so unetseg_stem_fwd takes it only when the caller wants
// them (has_stats); the queries (unetseg_stem_fwd_tile_m, unetseg_stem_config) assume it does, and a
// dense output (ldy = K).
static StemPlan plan_stem(const void* xp, int n, int h, int w, const void* wk, int K, void* y, int ldy, float* stats,
                          bool has_stats) {
  StemPlan p{};
  p.kind = kStemNone;
  if (stem_halo_ok(n, h, w, K, ldy) && has_stats) {
    p.kind = kStemHalo;
    return p;
  }
  IgemmArgs a = stem_args(xp, n, h, w, wk, K);
  a.y = y; a.ldy = ldy; a.accumulate = 0; a.bias = nullptr; a.relu = 0; a.stats = stats;
  if (!fast_tn_args(a, p.f)) return p;
  p.kind = kStemFast;
  return p;
}

// row tile of the stem's BN partial statistics (stats is [ceil(M/tile)][2][K]; the halo kernel's 16 x
// 32-pixel tiles are all full); -1: shape unsupported
UNETSEG_API int unetseg_stem_fwd_tile_m(int n, int h, int w, int K) {
  const StemPlan p = plan_stem(nullptr, n, h, w, nullptr, K, nullptr, K, nullptr, true);
  if (p.kind == kStemHalo) return stem_halo_tile_m();
  return p.kind == kStemFast ? tn_fast_tile_m(p.f) : -1;
}

// split-K slabs of the stem's weight gradient and its arguments (the fast family on the width-packed
// input); the workspace holds the slabs followed by the [K][64][7] reduced virtual gradient
static int stem_wgrad_plan(const void* xp, int n, int h, int w, const void* dy, int ldy, int K, FastWgradArgs& f) {
  f = stem_wgrad_args(xp, n, h, w, dy, ldy, K);
  return wgrad_fast_splits(K, f.Ng, f.Kpix);
}
static size_t stem_wgrad_bytes(int splits, int K, const FastWgradArgs& f) {
  return ((size_t)splits + 1) * K * f.Ng * sizeof(float);
}

// TN configuration of unetseg_stem_fwd (-1: shape unsupported) and the split-K slabs of
// unetseg_stem_wgrad (*splits_out, may be NULL)
UNETSEG_API int unetseg_stem_config(int n, int h, int w, int K, int* splits_out) {
  FastWgradArgs g;
  if (splits_out) *splits_out = stem_wgrad_plan(kSomePtr, n, h, w, kSomePtr, K, K, g);
  const StemPlan p = plan_stem(kSomePtr, n, h, w, kSomePtr, K, nullptr, K, nullptr, true);
  if (p.kind == kStemHalo) return kCfgStemHalo;
  return p.kind == kStemFast ? tn_fast_config(p.f, nullptr) : -1;
}

UNETSEG_API int unetseg_stem_fwd(const void* xp, int n, int h, int w, const void* wk, int K, void* y, int ldy,
                                 float* stats, void* stream) {
  US_CHECK_ARG(xp && wk && y && K % 8 == 0 && ldy >= K, "stem_fwd: bad args");
  const StemPlan p = plan_stem(xp, n, h, w, wk, K, y, ldy, stats, stats != nullptr);
  US_CHECK_ARG(p.kind != kStemNone, "stem_fwd: shape not supported by the fast kernels");
  if (p.kind == kStemHalo) launch_stem_halo(xp, n, h, w, wk, y, ldy, stats, (hipStream_t)stream);
  else launch_tn_fast(p.f, (hipStream_t)stream);
  US_LAUNCH_CHECK("stem_fwd");
  return 0;
}

UNETSEG_API size_t unetseg_stem_wgrad_workspace(int n, int h, int w, int K) {
  FastWgradArgs f;
  const int splits = stem_wgrad_plan(nullptr, n, h, w, nullptr, K, K, f);
  return stem_wgrad_bytes(splits, K, f);
}

// dw: fp32 [K][C][7][7] (PyTorch layout), written or accumulated
UNETSEG_API int unetseg_stem_wgrad(const void* xp, int n, int h, int w, const void* dy, int ldy, int K, float* ws,
                                   size_t ws_bytes, float* dw, int C, int accumulate, void* stream) {
  US_CHECK_ARG(xp && dy && ws && dw && K % 64 == 0 && C >= 1 && C <= 8, "stem_wgrad: bad args");
  FastWgradArgs f;
  const int splits = stem_wgrad_plan(xp, n, h, w, dy, ldy, K, f);
  f.ws = ws;
  US_CHECK_ARG(ws_bytes >= stem_wgrad_bytes(splits, K, f), "stem_wgrad: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  launch_wgrad_fast(f, splits, st);
  // parallel deterministic split reduce into v = ws tail, [K][64 virtual channels][7 rows], then permute
  float* v = ws + (size_t)splits * K * f.Ng;
  launch_wgrad_reduce(ws, splits, K, 64, 7, v, 64, 0, st);
  launch_stem_wgrad_remap(v, K, C, dw, accumulate, st);
  US_LAUNCH_CHECK("stem_wgrad");
  return 0;
}
