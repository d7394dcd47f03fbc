/*
 * unetseg_hip.h -- C ABI of libunetseg_hip.so, the MI355X (gfx950) hot path of U-Net segmentation
 * training: conv fwd/dgrad/wgrad on MFMA, BatchNorm, pooling, bilinear upsampling, the attention
 * gate, the fused losses (Lovasz hinge, BCE-with-logits, cross entropy), binary confusion counts and
 * Adam.
 *
 * The reference (TariAgentBenchmark/unet-embroidery-seg) has no FFI: its hot path sits behind the
 * nn.Module protocol (model/model_factory.py:22 build_model, train.py:48 create_model,
 * <Model>.forward, the loss callables in model/unet_training.py:205,253 and
 * model/unet_multitask.py:119).  Each entry point below replaces the PyTorch/ATen operator the
 * reference calls at the cited line; the Python mirror (unet-embroidery-seg_amd/unetseg_hip/*.py)
 * binds them with ctypes and keeps the reference's module names, state_dict keys and errors.
 *
 * Conventions
 *  - All pointers are DEVICE pointers borrowed from the caller (PyTorch's caching allocator); the
 *    library allocates nothing.  `stream` is a hipStream_t (NULL = legacy default stream).
 *  - Activations are NHWC with an explicit pixel stride `ld*` (elements between consecutive pixels),
 *    so a tensor may be a channel slice of a wider buffer (virtual concat).  `M` = n*h*w pixels.
 *  - `dtype`: 0 = fp32, 1 = bf16 (activations).  Weights arrive fp32 and are packed by
 *    unetseg_pack_conv_weight; statistics, biases, BN parameters and losses are always fp32.
 *  - Return value 0 = ok; non-zero = error, message via unetseg_last_error() (thread-local).
 *    Launches are asynchronous: device faults surface at the caller's next synchronisation.
 */
#ifndef UNETSEG_HIP_H
#define UNETSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------ */
const char* unetseg_last_error(void);
int unetseg_abi_version(void);
int unetseg_device_arch(char* buf, int n);

/* ---- convolution (nn.Conv2d: model/resnet_backbone.py:19,33,126,167; model/unet_resnet.py:17,19,
 *      72,74,78; model/unet_plain.py:9,12,69; model/unet_attention.py:16,20,24,76;
 *      model/unet_multitask.py:17,18,62,64,69) and the concat feeding it
 *      (torch.cat: model/unet_resnet.py:34, model/unet_plain.py:46, model/unet_attention.py:54) ---
 *
 * The channel-slice contract (tests/test_gpu_conv_strided.py holds every kernel configuration to it).
 * Every activation operand of the entry points of this section is a channel slice [c0, c0 + C) of a buffer
 * whose pixels are `ld` elements apart: the call passes the address of channel c0 of the first pixel and ld.
 *  - Strides honoured: unetseg_conv2d_fwd / _fwd_affine ldc1, ldc2 (the two sources may differ) and ldy;
 *    _fwd_bnrelu_in, _fwd_head, _fwd_mask ldc1 and ldy (the mask bits stay dense, [M][8]); unetseg_conv2d_dgrad
 *    ldy (dy) and ldx (dx, written or accumulated); _dgrad_post ldy, ldx and ld_aux, each its own (post 4: the
 *    bits are dense and ld_aux is ignored); _dgrad_post_res ldy, ldx, ld1 (y1) and ld2 (y2), each its own (its
 *    bits dense, [M][cin / 8]); unetseg_conv2d_wgrad / _wgrad_rows / _wgrad_bnrelu_in ldc1, ldc2 and ldy (dy);
 *    unetseg_stem_fwd / unetseg_stem_wgrad ldy (y, dy; the packed input xp is dense).  The first-3x3 kernel is
 *    taken only with ldc1 == 8 (the packed image); any other ldc1 runs the generic kernel.  Weights, biases,
 *    statistics, partials, dw and the workspace are dense.
 *  - Alignment: every ld and every c0 is a multiple of 8 elements and the buffer's base is 16-byte aligned, so
 *    each pixel of a slice starts on a 16-byte boundary (fp32: the same element counts, 32 bytes).
 *  - Writes: no byte outside channels [c0, c0 + C) of the n*h*w pixels of an output is written -- not the
 *    channels beside the slice, not the pixels before or after the tensor -- and no input is written at all.
 *  - Reads: what lies outside a slice never influences a result.  The kernels address past a slice (padding
 *    taps, absent rows of a partial tile) only under a bounds test or through a buffer descriptor whose extent,
 *    pixels * ld * 2 bytes from the slice's first element, makes such a read return zero; the strided call
 *    therefore gives, bit for bit, what the packed call (ld == C, c0 == 0) of the same values gives.
 *  - The configuration a call runs depends on its pixel strides only through the operands' byte extents: every
 *    operand must span less than 2^31 bytes (pixels * ld * 2) for the fast bf16 kernels, and a gather ring
 *    keeps its compile-time taps only while its 32-bit gather offsets cover them. */

/* fp32 [K][C][R][S] -> wk dtype [K][R][S][Cpad] (fwd) and, if wt != NULL, wt dtype [C][R][S][K] (dgrad) */
int unetseg_pack_conv_weight(int dtype, const float* w, int K, int C, int R, int S, int Cpad, void* wk, void* wt,
                             void* stream);
/* one conv of a batched pack; `desc` arrays of these live in DEVICE memory */
typedef struct UnetsegPackDesc {
  const float* w;  /* fp32 [K][C][R][S] */
  void* wk;        /* dtype [K][R][S][Cpad] */
  void* wt;        /* dtype [C][R][S][Kld] or NULL (columns K..Kld-1 untouched: a zeroed padded image) */
  long long start; /* first tile of this conv (ascending, desc[0].start == 0; unetseg_pack_tiles tiles) */
  int K, C, R, S, Cpad, Kld; /* Kld: wt row length, 0 = K (the 64-padded dgrad image of a narrow 1x1 conv) */
} UnetsegPackDesc;
/* blocks unetseg_pack_conv_weights spends on one conv: desc[i+1].start = desc[i].start + this */
int unetseg_pack_tiles(int K, int Cpad, int taps);
/* every conv weight of a model in one launch (total = number of tiles) */
int unetseg_pack_conv_weights(int dtype, const void* desc, int n, long total, void* stream);
/* legacy generic row tile (kept for ABI v1 callers) */
int unetseg_conv_tile_m(void);
/* row tile of the BN partial statistics unetseg_conv2d_fwd writes for this shape */
int unetseg_conv2d_fwd_tile_m(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w, int cout, int r,
                              int s, int stride, int pad);
/* y[n,p,q,cout] = conv(cat(x1[.., c1], x2[.., c2]), wk) (+bias) (ReLU); stats (may be NULL):
 * fp32 [ceil(M/tile)][2][cout] = per-tile (sum, M2 about the tile mean) of the rounded y (BN train).
 * Tile g holds output rows [g * tile, (g + 1) * tile) (the last one ragged) on the TN tiles, the gather rings and
 * the generic kernel; on halo3, first3x3 and the halo-A rings it is the g-th (tile / 32) x 32 spatial block, dealt
 * row-major over (image, block row, block column).  The sum is exact whenever the tile's |y| sum to less than
 * 2^24 (tests/test_gpu_conv_fast_exact.py holds every configuration to it per tile). */
int unetseg_conv2d_fwd(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2, int n, int h,
                       int w, const void* wk, int cout, int r, int s, int stride, int pad, const float* bias, int relu,
                       void* y, int ldy, float* stats, void* stream);
/* 1x1 stride-1 conv reading relu(x1 * in_sc[c] + in_sh[c]) -- the producer's BN-ReLU output, never
 * stored (model/resnet_backbone.py:58-62 bn2 -> ReLU -> conv3); epilogue as unetseg_conv2d_fwd. bf16 */
int unetseg_conv2d_fwd_bnrelu_in(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w, const void* wk,
                                 int cout, const float* in_sc, const float* in_sh, const float* bias, int relu,
                                 void* y, int ldy, float* stats, void* stream);
/* TN configuration that call runs (host-only query, -1 = none) */
int unetseg_conv2d_fwd_bnrelu_in_config(int dtype, int c1, int ldc1, int n, int h, int w, int cout);
/* The decoder's last 3x3 conv (64 -> 64, stride 1, pad 1, bias + ReLU; reference model/unet_resnet.py:77-78)
 * with the final 1x1 conv (model/unet_resnet.py:79, 64 -> head_k in {1, 2}) fused into its epilogue:
 * y as unetseg_conv2d_fwd, logits fp32 [n][head_k][h][w] = head_b + head_w . y (the stored bf16 y).
 * Replaces the reference's Conv2d -> ReLU -> Conv2d(1x1) forward.  bf16, halo path only; the _ok
 * query (host only) says whether a shape qualifies. */
int unetseg_conv2d_fwd_head_ok(int dtype, int ldc1, int n, int h, int w, int ldy, int head_k);
int unetseg_conv2d_fwd_head(int dtype, const void* x1, int ldc1, int n, int h, int w, const void* wk,
                            const float* bias, void* y, int ldy, int head_k, const float* head_w, const float* head_b,
                            float* logits, void* stream);
/* The decoder's 512^2 up_conv conv1 (3x3, 64 -> 64, stride 1, pad 1, bias + ReLU; model/unet_resnet.py:
 * 90-97): y as unetseg_conv2d_fwd, plus the ReLU mask of the stored y packed to bits, mbits[pixel][8]
 * (bit e of byte b = y[pixel][8b + e] > 0), which its consumer's data gradient reads (post 4 of
 * unetseg_conv2d_dgrad_post) instead of the 64-channel activation.  bf16, halo path only; mbits ==
 * NULL: returns 1 when the shape qualifies, else 0 (host only, nothing launched). */
int unetseg_conv2d_fwd_mask(int dtype, const void* x1, int ldc1, int n, int h, int w, const void* wk,
                            const float* bias, void* y, int ldy, unsigned char* mbits, void* stream);
/* its weight gradient with the same input prologue (workspace: unetseg_conv2d_wgrad_workspace) */
int unetseg_conv2d_wgrad_bnrelu_in(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w, const void* dy,
                                   int ldy, int cout, const float* in_sc, const float* in_sh, float* ws,
                                   size_t ws_bytes, float* dw, int dw_c, int accumulate, void* stream);
/* y = [relu](conv(x, wk) * escale[cout] + bias[cout]): eval-mode BN on the accumulator (generic kernel) */
int unetseg_conv2d_fwd_affine(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2, int n,
                              int h, int w, const void* wk, int cout, int r, int s, int stride, int pad,
                              const float* escale, const float* bias, int relu, void* y, int ldy, void* stream);
/* Kernel-configuration queries (host only, nothing is launched; replace no reference operator:
 * they let the parity tests assert that they exercise every kernel configuration the benchmark
 * selects).  Codes: 0 = halo3 (64-channel 3x3 kernel), 2..13 = TN tile configuration
 * (conv_fast.hip tn_config: 2 256x128, 3 128x128, 4 128x128 one K step, 5 64x128,
 * 6 128x64, 7 256x128 LDS-DMA ring, 9 64x128 ring, 10 128x128 5-stage ring, 13 128x64 ring;
 * 1, 8, 11, 12 and 14 are retired and not reused), 17 / 18 = the parity classes of a stride-2 data gradient merged into one launch
 * on 128x128 / 64x128 tiles, 19 / 20 = short-K (2-4 steps) 128x128 / 128x64 tiles on one LDS stage,
 * 21 / 22 / 23 = halo-A ring 256x128 / 256x64 / 128x128, 24 / 25 = the first two persistent (several tiles per
 * block), 100 = generic igemm kernel (fp32 / unaligned channels).  *taps_out = the
 * compile-time tap count of an LDS-DMA ring (9 or 1; 0 = generic ring or not a ring). */
int unetseg_conv2d_fwd_config(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w, int cout, int r,
                              int s, int stride, int pad, int* taps_out);
/* per output-parity class of the data gradient: cfg_out/taps_out[ph*stride+pw] (-1: not launched);
 * returns the number of classes launched */
int unetseg_conv2d_dgrad_config(int dtype, int ldy, int n, int p, int q, int cout, int cin, int r, int s, int stride,
                                int pad, int ldx, int h, int w, int* cfg_out, int* taps_out);
/* weight-gradient kernel: 0 = halo3_wgrad, 1 = wgrad_fast 64x256 row-run, 2 = wgrad_fast 128x128
 * row-run, 3 / 4 = the same tiles with general pixel walks, 5 = generic; *splits_out = split-K
 * slabs (reduced by wgrad_reduce<16> from 16 slabs, <4> from 4, else <1>) */
int unetseg_conv2d_wgrad_config(int dtype, int c1, int ldc1, int c2, int ldc2, int n, int h, int w, int ldy, int cout,
                                int r, int s, int stride, int pad, int* splits_out);
/* dx[n,h,w,cin] (+)= conv_transpose(dy[n,p,q,cout], wt).  The gradient g is accumulated in fp32; accumulate == 0
 * stores bf16(g).  Rounding of accumulate != 0 in bf16, by kernel family (asserted per configuration, bit for bit,
 * by tests/test_gpu_conv_fast_exact.py):
 *   halo3 (the 64-channel 3x3 kernel)                           dx = bf16(g + dx): one rounding;
 *   every TN configuration (tiles, gather rings, halo-A rings,  dx = bf16(bf16(g) + dx): the epilogue rounds g as
 *   their persistent forms, the merged stride-2 classes)        the plain store would, then adds -- two roundings,
 *                                                               what autograd's accumulation of two bf16 tensors gives;
 *   the generic kernel                                          dx = bf16(g + dx), fp32: dx = g + dx. */
int unetseg_conv2d_dgrad(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt, int cout, int cin,
                         int r, int s, int stride, int pad, void* dx, int ldx, int h, int w, int accumulate,
                         void* stream);
/* data gradient whose epilogue applies the producer's ReLU (post 1: aux = ReLU output) or BN-ReLU
   (post 2: aux = BN input z; psc/psh = BN affine, pmean/pinv = batch stats) mask and writes the
   first backward reduction of that op: part[rows][2][cin] = (sum d, sum d*xhat) per row tile
   (fuses model/resnet_backbone.py:95-110 ReLU+BN backward pass 1 / unet_resnet.py:37-40 ReLU+bias
   into the consumer conv's dgrad).  post 4: post 1 with the mask read from the producer's packed
   ReLU bits (aux = mbits of unetseg_conv2d_fwd_mask, ld_aux ignored; 64-channel halo path only).
   part == NULL: returns rows, or -1 when the shape has no fused path (bf16 fast kernels only). */
int unetseg_conv2d_dgrad_post(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt, int cout,
                              int cin, int r, int s, int stride, int pad, void* dx, int ldx, int h, int w, int post,
                              const void* aux, int ld_aux, const float* psc, const float* psh, const float* pmean,
                              const float* pinv, float* part, int rows, void* stream);
/* 1x1 stride-1 data gradient accumulated onto the other consumers' gradient already in dx (pixel stride
   ldx >= cin, a multiple of 8: dx may be a channel slice of a skip-concat gradient), with the residual
   BN-add-ReLU backward's first pass in its epilogue (model/resnet_backbone.py:88,110-113: the next
   block's conv1 is the last consumer of the block output): dx = d = mask * bf16(bf16(dgrad) + dx) -- the
   TN rule of unetseg_conv2d_dgrad: the gradient is rounded to bf16, then added to the old value in fp32
   and rounded again, bit for bit what the accumulating unetseg_conv2d_dgrad followed by the mask stores --
   mask = the packed ReLU bits written by unetseg_bn_apply_mask, part[rows][2 or 3][cin] = (sum d,
   sum d * (y1 - mean1) * inv1 [, sum d * (y2 - mean2) * inv2]) per row tile (y2 = the downsample
   branch's BN input, NULL: none).  Replaces unetseg_bn_bwd_reduce over dx.  part == NULL: returns rows,
   or 0 when the shape has no fused kernel (bf16 only). */
int unetseg_conv2d_dgrad_post_res(int dtype, const void* dy, int ldy, int n, int p, int q, const void* wt, int cout,
                                  int cin, void* dx, int ldx, const void* y1, int ld1, const float* mean1,
                                  const float* inv1, const unsigned char* mbits, const void* y2, int ld2,
                                  const float* mean2, const float* inv2, float* part, int rows, void* stream);
size_t unetseg_conv2d_wgrad_workspace(int dtype, int n, int p, int q, int cout, int cin, int r, int s);
/* dw fp32 [cout][dw_c][r][s] (PyTorch layout) (+)= sum_pix dy x; ws of the size queried above */
int unetseg_conv2d_wgrad(int dtype, const void* x1, int c1, int ldc1, const void* x2, int c2, int ldc2, int n, int h,
                         int w, const void* dy, int ldy, int cout, int r, int s, int stride, int pad, float* ws,
                         size_t ws_bytes, float* dw, int dw_c, int accumulate, void* stream);
/* the same for one source with dw holding only the first dw_rows (<= cout) GEMM rows: a padded-K conv
   (the attention gates' theta / phi, model/unet_attention.py:12-19: cout = the 64-padded output
   channels, whose dY columns are zero) accumulates straight into its real [dw_rows][dw_c][r][s] gradient */
int unetseg_conv2d_wgrad_rows(int dtype, const void* x1, int c1, int ldc1, int n, int h, int w, const void* dy,
                              int ldy, int cout, int r, int s, int stride, int pad, float* ws, size_t ws_bytes,
                              float* dw, int dw_c, int accumulate, int dw_rows, void* stream);

/* ---- ResNet stem on the fast kernels (model/resnet_backbone.py:126-131, conv 7x7/s2/p3) -------
   xp: width-padded bf16 [n][h][w+8][8] from unetseg_pack_input_stem (image column at +3);
   wk: bf16 [K][7][64] from unetseg_stem_pack_weight (k, filter row, filter col*8 + channel) */
int unetseg_pack_input_stem(const float* x, int n, int c, int h, int w, void* xp, void* stream);
int unetseg_stem_pack_weight(const float* w, int K, int C, void* wk, void* stream);
int unetseg_stem_fwd_tile_m(int n, int h, int w, int K);
/* configuration of unetseg_stem_fwd (30 = the persistent-halo stem kernel: 64 output channels, even
   input sizes whose output tiles into 16 x 32 pixels; else a TN code, -1: unsupported) and split-K
   slabs of unetseg_stem_wgrad */
int unetseg_stem_config(int n, int h, int w, int K, int* splits_out);
int unetseg_stem_fwd(const void* xp, int n, int h, int w, const void* wk, int K, void* y, int ldy, float* stats,
                     void* stream);
size_t unetseg_stem_wgrad_workspace(int n, int h, int w, int K);
int unetseg_stem_wgrad(const void* xp, int n, int h, int w, const void* dy, int ldy, int K, float* ws,
                       size_t ws_bytes, float* dw, int C, int accumulate, void* stream);
/* NCHW fp32 input [n][c][h][w] -> NHWC dtype [n][h][w][cpad] (zero channel padding), 1 <= c <= cpad.  Both packers
 * read and write dense arrays, write exactly the stated extent (pack_input_stem: the 3 left and 5 right border
 * columns and the channels >= c as zeros, 1 <= c <= 8) and return 0 without a launch, writing nothing, when n, h or
 * w is 0. */
int unetseg_pack_input(int dtype, const float* x, int n, int c, int h, int w, int cpad, void* y, void* stream);

/* ---- BatchNorm2d, training and eval (model/resnet_backbone.py:127,169; model/unet_plain.py:10,13;
 *      model/unet_attention.py:17,21,25) -------------------------------------------------------- */

/* Chan-merge conv partials part[G][2][C] -> batch mean/invstd, scale/shift; update running stats (momentum,
 * unbiased var) and num_batches_tracked when rmean != NULL */
int unetseg_bn_finalize(const float* part, int C, int G, long M, int tile, const float* gamma, const float* beta,
                        float* rmean, float* rvar, long long* nbt, float momentum, float eps, float* mean,
                        float* invstd, float* scale, float* shift, void* stream);
/* BN partials of an NHWC view no conv produced (model/unet_dualdense.py:9-10: BatchNorm over a dense
 * block's concatenation): part [ceil(M/tile)][2][C] = (sum, M2 about the tile mean), for bn_finalize */
int unetseg_channel_stats_tiles(long M, int tile);
int unetseg_channel_stats(int dtype, const void* x, int ldx, long M, int c, int tile, float* part, void* stream);
/* eval-mode BN folded into the conv epilogue (model/resnet_backbone.py:58-61, model/unet_plain.py:8-15
 * in .eval()): kscale = gamma / sqrt(running_var + eps), bias = beta - running_mean * kscale
 * (+ conv_bias * kscale), for unetseg_conv2d_fwd_affine */
int unetseg_bn_fold(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                    const float* conv_bias, float* kscale, float* bias, void* stream);
int unetseg_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                           float eps, float* scale, float* shift, void* stream);
/* out = [relu](y*sc + sh [+ r | + r*sc2 + sh2])   res_mode 0 none, 1 identity add, 2 BN'd add */
int unetseg_bn_apply(int dtype, const void* y, int ldy, const float* sc, const float* sh, const void* r, int ldr,
                     const float* sc2, const float* sh2, int res_mode, int relu, void* out, int ldo, long M, int C,
                     void* stream);
/* unetseg_bn_apply with relu = 1 that also writes the ReLU mask of `out` packed one byte per (pixel,
 * 16-B channel vector): mbits[p * C/V + c/V] bit (c % V) = (stored out[p][c] > 0), V = 8 (bf16) / 4
 * (fp32).  The backward below reads it (A = mbits, lda = 0) instead of the activation: the residual
 * BN-add-ReLU of the ResNet bottleneck (model/resnet_backbone.py:66-76), 1/16 of the bytes. */
int unetseg_bn_apply_mask(int dtype, const void* y, int ldy, const float* sc, const float* sh, const void* r, int ldr,
                          const float* sc2, const float* sh2, int res_mode, void* out, int ldo, long M, int C,
                          unsigned char* mbits, void* stream);
/* partial-buffer geometry of the channel reductions below: returns G (row groups) */
int unetseg_reduce_tiles(int dtype, long M, int C, int* tv_out, int* ppb_out);
/* backward through [relu](BN(y1) [+ BN(y2)]): per-channel partials of dz and dz*xhat.  The ReLU
 * mask comes from the activation A, from the packed mask of unetseg_bn_apply_mask (A = mbits with
 * lda == 0), or (A == NULL, msc != NULL: no residual) is recomputed from y1 as fmaf(y1, msc, msh) > 0
 * -- the forward's BN scale/shift -- saving one tensor read.  unetseg_bn_bwd_apply likewise. */
int unetseg_bn_bwd_reduce(int dtype, const void* dA, int ldd, const void* A, int lda, const float* msc,
                          const float* msh, const void* y1, int ld1, const float* mean1, const float* inv1,
                          const void* y2, int ld2, const float* mean2, const float* inv2, long M, int C, float* part,
                          int G, void* stream);
int unetseg_bn_bwd_finalize(const float* part, int C, int G, long M, int nbranch, const float* g1, const float* inv1,
                            float* dg1, float* db1, const float* g2, const float* inv2, float* dg2, float* db2,
                            float* coef, void* stream);
int unetseg_bn_bwd_apply(int dtype, const void* dA, int ldd, const void* A, int lda, const float* msc,
                         const float* msh, const void* y1, int ld1, const float* mean1, const float* inv1, void* dy1,
                         int ldo1, const void* y2, int ld2,
                         const float* mean2, const float* inv2, void* dy2, int ldo2, const float* coef, void* dzout,
                         int ldz, int dz_acc, long M, int C, void* stream);
/* ReLU backward (mask from the activation A) + per-channel bias-grad partials */
int unetseg_relu_bwd_bias(int dtype, const void* dA, int ldd, const void* A, int lda, void* dY, int ldy, long M, int C,
                          float* part, int G, void* stream);
int unetseg_colsum_finalize(const float* part, int C, int G, float* out, int accumulate, void* stream);
/* BN backward coefficients / ReLU bias gradient from the row partials part[G][2][C] written by
   unetseg_conv2d_dgrad_post (model/resnet_backbone.py BatchNorm2d backward, unet_resnet.py ReLU) */
int unetseg_bn_bwd_finalize_rows(const float* part, int C, int G, long M, const float* g1, const float* inv1,
                                 float* dg1, float* db1, float* coef, void* stream);
/* the same for the residual post-op's part[G][1+nbranch][C] (unetseg_conv2d_dgrad_post_res): coefficients
   of both branches as unetseg_bn_bwd_finalize, coef [3*nbranch][C].  nbranch == 1: g2, inv2, dg2, db2 may be NULL
   and only coef rows 0..2 are written; nbranch == 2: db2 and coef[4] take the same sum of dz as db1 and coef[1] */
int unetseg_bn_bwd_finalize_rows_res(const float* part, int C, int G, long M, int nbranch, const float* g1,
                                     const float* inv1, float* dg1, float* db1, const float* g2, const float* inv2,
                                     float* dg2, float* db2, float* coef, void* stream);
int unetseg_colsum_rows(const float* part, int C, int G, int k, float* out, int accumulate, void* stream);
/* Row partials [G][nq][C] -> [ceil(G/16)][nq][C] (16 consecutive rows merged; nq 2 or 3), run ahead of the
   finalizes above when G is large.  tile > 0: the rows are BN statistics (sum, M2 about the row mean) of
   `tile` pixels each (the last min(tile, M - g*tile)) merged by Chan's formula (nq == 2), so the merged
   partials feed unetseg_bn_finalize with tile * 16; tile == 0: plain sums.  No reference operator: an
   internal reduction stage of BatchNorm2d's statistics / backward sums. */
int unetseg_fin_merge_rows(const float* part, int C, int G, long M, int tile, int nq, float* out, void* stream);

/* ---- pooling / resampling (nn.MaxPool2d: model/resnet_backbone.py:131, model/unet_plain.py:25,
 *      model/unet_attention.py:66-69; UpsamplingBilinear2d / Upsample / interpolate:
 *      model/unet_resnet.py:21,71, model/unet_plain.py:36, model/unet_attention.py:32,41,53) ------- */
int unetseg_maxpool_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c, int k, int s, int ceil_mode,
                        void* y, int ldy, uint8_t* idx, int* p_out, int* q_out, void* stream);
int unetseg_maxpool_bwd(int dtype, const void* dy, int ldy, const uint8_t* idx, int n, int h, int w, int c, int k,
                        int s, int p, int q, void* dx, int ldx, int accumulate, void* stream);
int unetseg_upsample2x_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c, int align_corners, void* y,
                           int ldy, void* stream);
int unetseg_upsample2x_bwd(int dtype, const void* dy, int ldy, int n, int h, int w, int c, int align_corners,
                           void* dx, int ldx, int accumulate, void* stream);
/* upsample2x_bwd with the backward of the ReLU that produced x fused in (x = A, that ReLU's output, the
 * upsample its sole consumer; reference model/unet_resnet.py:25-33 unetUp conv2 -> ReLU -> next
 * block's UpsamplingBilinear2d): dx = (A > 0) ? adjoint(dy) : 0 (no accumulate); part fp32
 * [rows][2][c], slot 0 = per-block column sums of dx (the conv's bias-gradient partials,
 * unetseg_colsum_rows); rows = unetseg_upsample2x_bwd_tiles(...).  The channel vectors c / V must divide 256
 * (the block's column-sum layout); any other count is an argument error. */
int unetseg_upsample2x_bwd_tiles(int dtype, int n, int h, int w, int c);
int unetseg_upsample2x_bwd_relu(int dtype, const void* dy, int ldy, int n, int h, int w, int c, int align_corners,
                                const void* a, int lda, void* dx, int ldx, float* part, int rows, void* stream);
int unetseg_add(int dtype, const void* x, int ldx, void* out, int ldo, long M, int c, void* stream);
/* general bilinear resize to (oh, ow) with ATen's source-index rule (F.interpolate(size=...):
 * model/unet_attention.py:31-33,52-53, model/unet_dualdense.py:57-58; align_corners=True for the
 * multiclass losses' logit resize, model/unet_training.py:14-15); backward is a deterministic gather.
 * Per axis, in fp32: align_corners: src = dst * ((in-1)/(out-1)) (scale 0 when out == 1); otherwise
 * src = max(0, fma(dst + 0.5, in/out, -0.5)) -- one fused multiply-add, rounded once: this library's rule.
 * ATen builds that contract the expression (its GPU kernels, its AVX2 and later CPU kernels) evaluate the same;
 * one that rounds the product first differs in l1 by at most 2^-24 * src.
 * i0 = (int)src (at most in-1), i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1. */
int unetseg_resize_bilinear_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c, int oh, int ow,
                                int align_corners, void* y, int ldy, void* stream);
int unetseg_resize_bilinear_bwd(int dtype, const void* dy, int ldy, int n, int h, int w, int c, int oh, int ow,
                                int align_corners, void* dx, int ldx, int accumulate, void* stream);
/* zero padding x [n][h][w] into y [n][oh][ow] at (top, left) (F.pad, model/unet_plain.py:42-45) and its
 * backward dx (+)= the (top, left) window of dy */
int unetseg_pad2d_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c, int top, int left, int oh,
                      int ow, void* y, int ldy, void* stream);
int unetseg_pad2d_bwd(int dtype, const void* dy, int ldy, int n, int h, int w, int c, int top, int left, int oh,
                      int ow, void* dx, int ldx, int accumulate, void* stream);

/* ---- narrow 1x1 heads (final / outc / seg_head / psi: model/unet_resnet.py:78,
 *      model/unet_plain.py:69, model/unet_multitask.py:69, model/unet_attention.py:24) ------------
 *
 * The pointwise contract (tests/test_gpu_pointwise_contract.py holds every entry point named here to it, element
 * by element; tests/test_pointwise_args_cpu.py the refusals).  It covers unetseg_pw_small_fwd / _bwd / _bwd_relu,
 * unetseg_pw_head_fwd / _bwd, unetseg_attn_apply / _bwd1 / _bwd2, unetseg_gap_fwd / _bwd and the two input packers.
 *  - Strides: every NHWC operand (x, dx, skip, gated, dg, dskip, f, dzf) is a channel slice [c0, c0 + c) of a buffer
 *    whose pixels are `ld` elements apart, each operand with its own ld >= c; the call passes the address of channel
 *    c0 of the first pixel.  An ld below c is refused.  Everything else is dense: weights, biases, the planar fp32
 *    images y / dy [n][k][hw] (M = n * hw), the per-pixel fp32 vectors psi, alpha, dpsibn [M], the BatchNorm scalars
 *    and the partial arrays.
 *  - Alignment: the kernels move 16-byte vectors (V = 8 bf16 / 4 fp32 elements), so c, every ld and every c0 are
 *    multiples of V and the buffer's base is 16-byte aligned; an ld that is no multiple of V is refused.  The
 *    exceptions access by element and take any ld >= c and any c0: unetseg_pw_head_bwd (c divides 256),
 *    unetseg_gap_fwd / _bwd (any c > 0).
 *  - Writes: no byte outside channels [c0, c0 + c) of the M pixels of an output, and nothing past the stated length
 *    of a dense output, is written; no input is written.  Written outputs (y, stats, alpha, gated, dpsibn, dzf, g,
 *    every partial array, dx / dskip without the accumulate flag) need no initialisation; with dx_acc / ds_acc /
 *    accumulate != 0 the old value is read and the sum stored (one more rounding).  A NULL dx (pw_small_bwd,
 *    pw_head_bwd) skips dx; lddx is then ignored.
 *  - Aliasing: no output may overlap an input or another output of the same call.  Two inputs may be the same
 *    buffer, and two operands may be disjoint channel slices of one buffer (the op layer's concat and dense-block
 *    slices).
 *  - Partials: one slot per pixel tile g, the sum over that tile's pixels [g * tile, min(M, (g + 1) * tile)), plainly
 *    stored (never accumulated), to be summed over g by unetseg_colsum_finalize / unetseg_bn_bwd_finalize:
 *      pw_small_bwd / _bwd_relu  part_w [k][c][G], part_b [k][G], part_d [G][2][c];  G = unetseg_pw_small_tiles(M),
 *                                tile = unetseg_pw_small_tile(M)
 *      pw_small_fwd              stats [G][2] = (sum, M2 about the tile's own mean) of y, the same G and tile
 *      pw_head_bwd               part_w [k][c][G], part_b [k][G];  G = unetseg_pw_head_tiles(M), tile = 2048
 *      attn_bwd1                 part [2][G1];  G1 = unetseg_attn_bwd1_tiles(M), tile = 128
 *      attn_bwd2                 part_w [c][G], part_b [G];  G and tile as pw_small_bwd
 *  - M == 0 (gap: B == 0, gap_bwd also HW == 0; the packers: n, h or w == 0) returns 0 and launches nothing; no
 *    pointer is looked at.  Otherwise every pointer not marked "may be NULL" is required and NULL is refused.
 *    Negative sizes, and hw <= 0 with M > 0, are refused. */
int unetseg_pw_small_tile(long M); /* pixels per tile (2048, smaller when M gives < 512 tiles) */
int unetseg_pw_small_tiles(long M);
/* y fp32 planar [n][k][hw] = x . W^T + b, k = 1 or 2, W fp32 [k][c], b fp32 [k] (may be NULL: no bias); c / V a power
 * of two <= 64; stats (k == 1 only, may be NULL) [unetseg_pw_small_tiles(M)][2] */
int unetseg_pw_small_fwd(int dtype, const void* x, int ldx, long M, int hw, int c, int k, const float* w,
                         const float* b, float* y, float* stats, void* stream);
/* dx (may be NULL) (+)= dy . W; k = 1 or 2 (anything else is refused); c / V divides 256 */
int unetseg_pw_small_bwd(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c, int k,
                         const float* w, void* dx, int lddx, int dx_acc, float* part_w, float* part_b, void* stream);
/* pw_small_bwd with the producer ReLU's backward fused (x = ReLU output, sole consumer; bf16):
 * dx = (x > 0) ? dy.W : 0 (written, exactly 0 where x <= 0); part_d [G][2][c], slot 0 = column sums of the stored
 * (rounded) dx, slot 1 = 0 (replaces the
 * reference autograd's ReLU backward + conv bias grad of up_conv's last conv, model/unet_resnet.py:70-78,100-103). */
int unetseg_pw_small_bwd_relu(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c, int k,
                              const float* w, void* dx, int lddx, float* part_w, float* part_b, float* part_d,
                              void* stream);

/* ---- attention gate (AttentionGate.forward: model/unet_attention.py:28-36) -------------------- */
/* The pointwise contract above applies (strides lds_ / ldg / ldds / ldf / lddz, alignment, writes, M == 0).
 * alpha [M] = sigmoid(psi * sc[0] + sh[0]) (fp32; within 4 fp32 ulps of the exact sigmoid of the fp32 argument);
 * gated = skip * alpha; c a multiple of V */
int unetseg_attn_apply(int dtype, const void* skip, int lds_, const float* psi, const float* sc, const float* sh,
                       float* alpha, void* gated, int ldg, long M, int c, void* stream);
/* dskip (+)= dg * alpha (ds_acc != 0 accumulates); dpsibn [M] = (sum_c dg * skip) * alpha * (1 - alpha), written;
 * part: [2][G1] (sum dpsibn, sum dpsibn * xhat with xhat = (psi - mean[0]) * inv[0]) per 128-pixel tile,
 * G1 = unetseg_attn_bwd1_tiles(M); c / V a power of two */
int unetseg_attn_bwd1_tiles(long M);
int unetseg_attn_bwd1(int dtype, const void* dg, int ldg, const void* skip, int lds_, const float* alpha,
                      const float* psi, const float* mean, const float* inv, void* dskip, int ldds, int ds_acc,
                      float* dpsibn, long M, int c, float* part, void* stream);
/* dpsi = coef[0] * (dpsibn - coef[1] - xhat * coef[2]) (coef: the first three of unetseg_bn_bwd_finalize's table);
 * dzf = (f > 0) ? dpsi * wpsi : 0, written, exactly 0 where f <= 0 (f = the ReLU output psi's conv read);
 * part_w [c][G] = sum dpsi * f, part_b [G] = sum dpsi per tile of unetseg_pw_small_tile(M) pixels; c / V divides 256 */
int unetseg_attn_bwd2(int dtype, const float* dpsibn, const float* psi, const float* mean, const float* inv,
                      const float* coef, const void* f, int ldf, const float* wpsi, void* dzf, int lddz, long M, int c,
                      float* part_w, float* part_b, void* stream);

/* ---- losses and metrics ---------------------------------------------------------------------- */
/* Lovasz hinge, per-image mean (model/unet_training.py:219-280) on z = o[:,1]-o[:,0] (nch 2,
 * utils/train_and_eval.py:106-113) or o[:,0] (nch 1); gz = dloss/dz; loss fp32 scalar */
size_t unetseg_lovasz_workspace(int B, long P);
int unetseg_lovasz_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, void* ws, size_t ws_bytes,
                       float* gz, float* loss, void* stream);
/* per-image Lovasz over the pixels whose target is not ignore_index (model/unet_training.py:268-274) */
int unetseg_lovasz_fwd_masked(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index, void* ws,
                              size_t ws_bytes, float* gz, float* loss, void* stream);
/* BCE-with-logits mean with optional scalar pos_weight (model/unet_training.py:205-216) */
size_t unetseg_bce_workspace(int B, long P);
int unetseg_bce_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, const float* pos_weight, void* ws,
                    size_t ws_bytes, float* gz, float* loss, void* stream);
/* dout[n][ch][P] = gz * (s1*a1) [* (s2*a2)] with the two-class split of utils/train_and_eval.py:106 */
int unetseg_dz_to_dout(const float* gz, int B, long P, int nch, const float* s1, float a1, const float* s2, float a2,
                       float* scratch, float* dout, void* stream);
/* global tp/fp/fn/tn (argmax, tie -> class 0) of utils/train_and_eval.py:116-138,293 */
int unetseg_confusion(const float* out, int nch, const int64_t* tgt, int B, long P, unsigned long long* conf,
                      void* stream);
/* the same with ignore_index (utils/train_and_eval.py:125-126,172-176): pixels whose target equals
 * ignore_index are skipped by the counts and the losses.  masked loss kind 0 = BCE over the valid
 * pixels, 1 = the reference's Lovasz on the flattened valid pixels (a per-pixel hinge mean, since
 * lovasz_hinge_loss then loops over single elements: model/unet_training.py:267-276) */
int unetseg_confusion_masked(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index,
                             unsigned long long* conf, void* stream);
size_t unetseg_masked_loss_workspace(int B, long P);
int unetseg_masked_loss_fwd(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index, int kind,
                            const float* pos_weight, void* ws, size_t ws_bytes, float* gz, float* loss, void* stream);
/* cross entropy, mean over the batch (MultiTaskLoss: model/unet_multitask.py:119-139) */
int unetseg_ce_fwd(const float* logits, const int64_t* tgt, int B, int K, float* loss, float* dlog, void* stream);
int unetseg_scale_grad(const float* g, long n, const float* s1, float a1, const float* s2, float a2, float* out,
                       void* stream);

/* ---- multiclass task (model/unet_training.py:9-91 CE_Loss / Focal_Loss / Dice_loss;
 *      utils/train_and_eval.py:20-103 metrics; model/*.py outc/final with num_classes > 2;
 *      predict.py:79-93 post-processing).  Logits fp32 planar [B][C][P], C <= 32. ----------------- */
/* 1x1 head with 1 <= k <= 32 outputs: y fp32 [n][k][hw] = x . W^T + b (W fp32 [k][c]) */
int unetseg_pw_head_fwd(int dtype, const void* x, int ldx, long M, int hw, int c, int k, const float* w,
                        const float* b, float* y, void* stream);
int unetseg_pw_head_tiles(long M);
/* dx (may be NULL) (+)= dy . W; part_w [k][c][G], part_b [k][G] (G = unetseg_pw_head_tiles(M), 2048-pixel tiles);
 * c divides 256.  Both heads follow the pointwise contract stated with the narrow 1x1 heads above (pw_head_fwd
 * moves 16-byte vectors: c and ldx multiples of V; pw_head_bwd accesses by element: any ldx, lddx >= c) */
int unetseg_pw_head_bwd(int dtype, const float* dy, const void* x, int ldx, long M, int hw, int c, int k,
                        const float* w, void* dx, int lddx, int dx_acc, float* part_w, float* part_b, void* stream);
size_t unetseg_mc_loss_workspace(int B, int C, long P);
/* loss fp32[3] = (total, main, dice).  focal: main term 0 = CE (class weights cls_w or NULL, ignore_index),
 * 1 = Focal (alpha < 0: None, gamma), 2 = none; dice_t float [B][P][ct] one-hot (NULL: no Dice term) */
int unetseg_mc_loss_fwd(const float* out, const int64_t* tgt, int B, int C, long P, const float* cls_w,
                        long ignore_index, int focal, float alpha, float gamma, const float* dice_t, int ct,
                        float beta, float smooth, void* ws, size_t ws_bytes, float* loss, void* stream);
/* dout fp32 [B][C][P] = gscale[0] * d total / d out (same arguments and workspace as the forward) */
int unetseg_mc_loss_bwd(const float* out, const int64_t* tgt, int B, int C, long P, const float* cls_w,
                        long ignore_index, int focal, float alpha, float gamma, const float* dice_t, int ct,
                        float beta, float smooth, const void* ws, const float* gscale, float* dout, void* stream);
/* Lovasz-softmax (Berman et al., CVPR 2018, Alg. 1, class-averaged softmax errors) of fp32 planar logits
 * out [B][C][P], 2 <= C <= 32, against tgt int64 [B][P]; a label equal to ignore_index or outside [0, C) is
 * invalid.  Per present class c: e = |[tgt == c] - softmax_c| over the valid pixels, sorted descending (ties:
 * ascending pixel index), loss_c = sum_k e_(k) (J_k - J_{k-1}); a segment's loss is the mean over its present
 * classes.  per_image != 0: one segment per image, loss = mean over the B images (an image without a valid
 * pixel counts 0); per_image == 0: one segment of all B*P pixels.  dlogits (NULL: value only) fp32 [B][C][P] =
 * d loss / d out for a unit upstream gradient, exactly 0 at invalid pixels.  B*P < 2^31.
 * Workspace, with S segments of L keys and T = ceil(L / 4096) (per image S = B*C, L = P; else S = C, L = B*P):
 * 16 B C P + 4 S T (256 + 2) + 8 S + 256 bytes. */
size_t unetseg_lovasz_softmax_workspace(int B, int C, long P, int per_image);
int unetseg_lovasz_softmax_fwd(const float* out, const int64_t* tgt, int B, int C, long P, long ignore_index,
                               int per_image, void* ws, size_t ws_bytes, float* dlogits, float* loss, void* stream);
/* hist u64 [(C+1)][C] += (target row, argmax column); targets outside [0, C) count in row C */
int unetseg_mc_confusion(const float* out, const int64_t* tgt, int B, int C, long P, unsigned long long* hist,
                         void* stream);
/* one image: labels int32 [OH][OW] = argmax_c bilinear(align_corners=False)-resized softmax of the
 * logits [C][H][W] cropped to rows y0..y0+ch, cols x0..x0+cw */
int unetseg_softmax_resize_argmax(const float* logits, int C, int H, int W, int y0, int x0, int ch, int cw, int OH,
                                  int OW, int32_t* labels, void* stream);

/* ---- tiled full-resolution inference (no reference counterpart; predict.predict_labels_tiled) ------
 * Grid (utils/tiling.py): tile t, overlap o (0 <= o <= t / 2), stride s = t - o,
 * n = max(1, ceil((L - o) / s)) tiles per axis at origins i * s (they may hang over the far edge),
 * row-major tile index iy * nx + ix.  Window w(u) = min(1, (u + 1) / (o + 1), (t - u) / (o + 1)) in fp32;
 * blended probability = sum_i w_i softmax(logits_i) / sum_i w_i over the (at most 4) covering tiles in
 * ascending index.  2 <= C <= 32.  Tile ranges t0 .. t0+nt-1 may be issued in any split, in ascending
 * order on one stream: the accumulated bits do not depend on the split. */
/* host only: tiles per row (nx) and per column (ny) */
int unetseg_tile_count(int H, int W, int tile, int overlap, int* nx, int* ny);
/* out fp32 [nt][3][tile][tile] = img (uint8 HWC RGB, device) / 255, fill / 255 outside the image */
int unetseg_tile_gather(const uint8_t* img, int H, int W, int tile, int overlap, int t0, int nt, int fill,
                        float* out, void* stream);
/* acc fp32 [C][H][W] (zeroed by the caller) += window * softmax over C of logits fp32 [nt][C][tile][tile] */
int unetseg_tile_accum(const float* logits, int C, int H, int W, int tile, int overlap, int t0, int nt, float* acc,
                       void* stream);
/* probs fp32 [C][H][W] (may be NULL) = acc / total window weight; labels int32 [H][W] = argmax (a tie
 * goes to the lowest class) */
int unetseg_tile_finish(const float* acc, int C, int H, int W, int tile, int overlap, float* probs, int32_t* labels,
                        void* stream);

/* ---- flip / rotation test-time augmentation (no reference counterpart; unetseg_hip/tta.py) ----------
 * View k in 0..7: f = k & 1, r = k >> 1; view k of x[.., H, W] is the W-flip (if f) followed by r
 * counter-clockwise quarter turns: torch.rot90(torch.flip(x, [-1]) if f else x, r, (-2, -1)).  `views`
 * is an 8-bit mask in 1..255 (bit k = view k), slabs ordered by ascending k, K = popcount(views).  A
 * view with odd r (bits 2, 3, 6, 7) needs H == W.  Both calls check their arguments before any launch. */
/* out fp32 [K][B][C][H][W] = the K views of x fp32 [B][C][H][W]; a bit-exact permutation, one launch */
int unetseg_tta_views(const float* x, int B, int C, int H, int W, int views, float* out, void* stream);
/* out fp32 [B][C][H][W] (identity frame) from logits fp32 [K][B][C][H][W], slab k in view k's frame:
 * C >= 2: log(max(sum_k p_k[c] / K, FLT_MIN)), p_k the softmax over C of view k's logits at the pixel
 * view k maps (y, x) to, summed in ascending k from 0 with fp32 adds;
 * C == 1: log(max(mean_k sigmoid(z_k), FLT_MIN)) - log(max(mean_k sigmoid(-z_k), FLT_MIN)).
 * 1 <= C <= 32; every output is finite. */
int unetseg_tta_merge(const float* logits, int B, int C, int H, int W, int views, float* out, void* stream);

/* ---- connected components of a class map (no reference counterpart; unetseg_hip/ccl.py) -----------
 * cls int32 [N][H][W]: values are compared for equality only, class 0 is background.  Two pixels of one
 * image are joined iff they have equal class and are edge neighbours, or diagonal neighbours where that
 * class is 8-connected: the non-zero classes have `connectivity` (4 or 8), class 0 the dual (4 for 8,
 * 8 for 4).  A component's name is its root: the smallest raster index y * W + x among its pixels.
 * H * W <= 2^31 - 1 per image; offsets across the batch are 64-bit.  Every call checks its arguments
 * before any launch; none waits on the host. */
/* the tile of the label pass (host only): its seams lie at the multiples of *tw and *th */
int unetseg_ccl_tile(int* tw, int* th);
/* root int32 [N][H][W] = the root of every pixel's component; also the pass's only scratch */
int unetseg_ccl_label(const int32_t* cls, int N, int H, int W, int connectivity, int32_t* root, void* stream);
/* stats int32 [4][N][H][W], planes area, ymax, xmin, xmax, from root as unetseg_ccl_label wrote it:
 * meaningful at root positions; elsewhere area is 0 and the rest unspecified.  ymin is the root's row. */
int unetseg_ccl_stats(const int32_t* root, int N, int H, int W, int32_t* stats, void* stream);
/* out int32 [N][H][W] (not cls) = cls with every component of area < threshold relabelled; root and
 * stats as the two calls above wrote them for cls.  step 1: components of a non-zero class become 0.
 * step 2: class-0 components that touch no image border take the class of the pixel above their root. */
int unetseg_ccl_filter(const int32_t* cls, const int32_t* root, const int32_t* stats, int N, int H, int W, int step,
                       int threshold, int32_t* out, void* stream);

/* ---- boundary quality of class maps (no reference counterpart; unetseg_hip/boundary.py) -------------
 * Maps are [N][H][W] with H, W <= 16384; `ignore` = -1 means no ignored value.  Everything is integer
 * and bitwise reproducible.  Every call checks its arguments before any launch; none waits on the host. */
#define UNETSEG_EDT_INF (1 << 30)
/* edge uint8 = 1 where cls int32 == c, is not `ignore`, and one of the four edge neighbours lies inside
 * the image, is not `ignore` and has a class != c; 0 elsewhere (the image frame is no boundary) */
int unetseg_boundary_edges(const int32_t* cls, int N, int H, int W, int c, int ignore, uint8_t* edge, void* stream);
/* d2 int32 = the exact squared Euclidean distance to the nearest non-zero pixel of the same image of
 * sites uint8; UNETSEG_EDT_INF everywhere in an image without one.  d2 is the only scratch. */
int unetseg_edt_sqdist(const uint8_t* sites, int N, int H, int W, int32_t* d2, void* stream);
/* host only: the distance transform works on column segments and row chunks of *len pixels, so its seams
 * lie at the multiples of *len */
int unetseg_edt_chunk(int* len);
/* counts int64 [2 (K + 2) + 2] +=, with eP / eG = the edge maps of pred / target for class c and dP / dG
 * their distance transforms: [0 .. K+1] the histogram of min(dG, K + 1) over the edge pixels of eP,
 * [K+2 .. 2K+3] that of min(dP, K + 1) over the edge pixels of eG, [2K+4] and [2K+5] the size of the
 * intersection and of the union of {pred == c, dP <= biou_d2} and {target == c, dG <= biou_d2} without the
 * pixels whose target is `ignore`.  0 <= biou_d2 <= K <= 65536. */
int unetseg_boundary_counts(const int32_t* pred, const int32_t* target, const uint8_t* eP, const uint8_t* eG,
                            const int32_t* dP, const int32_t* dG, int N, int H, int W, int c, int ignore, int K,
                            int biou_d2, int64_t* counts, void* stream);

/* ---- boundary (distance-map) loss (Kervadec et al., MIDL 2019; no reference counterpart) -------------
 * out planar fp32 [B][nch][H][W] (nch 2: z = o1 - o0, nch 1: z = o0), tgt int64 [B][H][W], class c,
 * ignore_index (-1: none).  Per image fg = {t == c}, bg = {t != c, t != ignore_index}; d2fg / d2bg the
 * exact squared distance to the nearest fg / bg pixel of the image (unetseg_edt_sqdist over both site maps of
 * the batch in one call).  phi = +sqrt(d2fg) on bg, -(sqrt(d2bg) - 1) on fg, 0 on ignored pixels and wherever
 * the distance it would use is UNETSEG_EDT_INF (so an image without fg, or without bg, contributes 0).
 * With p = sigmoid(z) and Nvalid the non-ignored pixels of the batch:
 *   loss[0] = inv_norm / Nvalid * sum_valid p phi          (0 when Nvalid == 0; never weighted)
 *   gz [B][H][W] (may be NULL) = weight * p (1 - p) phi inv_norm / Nvalid on valid pixels, 0 on ignored ones;
 *   added to gz when accumulate != 0, so the term lands on a region loss's gz (unetseg_dz_to_dout then spreads
 *   the sum).  phi [B][H][W] (may be NULL) receives the signed distance map.
 * Nvalid is counted on the device while the site maps are written and 1 / Nvalid enters gz as it is written:
 * no host wait and no second pass.  loss, gz and phi are bitwise reproducible.  Checked before any launch:
 * null out / tgt / ws / loss, nch in {1, 2}, B, H, W > 0, H, W <= 16384, ignore_index != c, ws_bytes, and a
 * 16-byte aligned ws.  Nothing past the B * H * W elements of gz and phi and past ws_bytes is written. */
size_t unetseg_boundary_loss_workspace(int B, int H, int W); /* host only */
int unetseg_boundary_loss_fwd(const float* out, int nch, const int64_t* tgt, int B, int H, int W, int c,
                              long ignore_index /* -1: none */, float inv_norm, float weight, void* ws,
                              size_t ws_bytes, float* gz, int accumulate, float* phi /* may be NULL */, float* loss,
                              void* stream);

/* ---- soft skeleton and soft-clDice loss (Shit et al., CVPR 2021; no reference counterpart) -----------------
 * x fp32 [H][W] in [0, 1]; windows are clipped to the image, a pixel outside it never takes part.
 *   E(x)(q) = min over q and its four edge neighbours       window order: up, left, centre, right, down
 *   D(x)(q) = max over the 3 x 3 neighbourhood of q         window order: row-major
 *   O(x)    = D(E(x))
 * Soft skeleton S_k(x), k = iters (the published soft_skel):
 *   x_0 = x,            s_0 = relu(x_0 - O(x_0))
 *   x_j = E(x_{j-1}),   d_j = relu(x_j - O(x_j)),   s_j = s_{j-1} + relu(d_j - s_{j-1} d_j)     j = 1 .. k
 *   S_k = s_k
 * Subgradients: relu'(a) = 1 iff a > 0; the gradient of a min or max window goes entirely to the first element
 * that attains the extreme in window order.  x_j and O(x_j) are selections of input values (exact); each level
 * rounds d_j and s_j in fp32 (four roundings, no fused multiply-add).
 *
 * unetseg_soft_skel_fwd: skel [N][H][W] = S_iters(x), x fp32 [N][H][W]; iters + 1 launches.  The levels the
 * backward needs stay in ws (2 iters + 4 maps of N H W floats, each rounded up to 256 bytes).
 * unetseg_soft_skel_bwd: gx [N][H][W] = the gradient of sum(gskel * S_iters(x)) by x, from the ws that
 * unetseg_soft_skel_fwd filled for the same x, shape and iters; iters + 1 launches in gather form, every sum in a
 * fixed order, no atomics.
 *
 * unetseg_cldice_fwd: out planar fp32 [B][nch][H][W] (nch 2: z = o1 - o0, nch 1: z = o0), tgt int64 [B][H][W],
 * ignore_index (-1: none).  y = [t == 1], p = sigmoid(z); ignored pixels enter as y = 0, p = 0 and get zero
 * gradient.  With every sum over the whole batch:
 *   tprec = (sum S_k(p) y + smooth) / (sum S_k(p) + smooth)
 *   tsens = (sum S_k(y) p + smooth) / (sum S_k(y) + smooth)
 *   loss[0] = 1 - 2 tprec tsens / (tprec + tsens)                               (never weighted)
 *   gz [B][H][W] (may be NULL) = weight * dloss/dz, dloss/dz = (dloss/dp) p (1 - p); added to gz when
 *   accumulate != 0 (as a product, then a sum), so the term lands on a region loss's gz.
 * The four sums are per-block double partials added by one block in a fixed order; the backward reads
 * dloss/dtprec and dloss/dtsens from device scalars: no host wait.  loss, gz and the skeletons are bitwise
 * reproducible.  The published defaults are iters = 3, smooth = 1.
 *
 * Checked before any launch: null pointers (gz of unetseg_cldice_fwd may be NULL), nch in {1, 2}, N / B, H, W > 0,
 * 0 <= iters <= 64, smooth > 0, ignore_index != 1, ws_bytes, and a 16-byte aligned ws.  Nothing past the N H W
 * elements of skel, gx and gz and past ws_bytes is written.  The workspace queries return 0 for a shape or iters
 * they refuse. */
size_t unetseg_soft_skel_workspace(int N, int H, int W, int iters); /* host only */
int unetseg_soft_skel_fwd(const float* x, int N, int H, int W, int iters, void* ws, size_t ws_bytes, float* skel,
                          void* stream);
int unetseg_soft_skel_bwd(const float* x, int N, int H, int W, int iters, void* ws, size_t ws_bytes,
                          const float* gskel, float* gx, void* stream);
size_t unetseg_cldice_workspace(int B, int H, int W, int iters); /* host only */
int unetseg_cldice_fwd(const float* out, int nch, const int64_t* tgt, int B, int H, int W,
                       long ignore_index /* -1: none */, int iters, float smooth, float weight, void* ws,
                       size_t ws_bytes, float* gz /* may be NULL */, int accumulate, float* loss, void* stream);

/* ---- hard skeleton (thinning) and the clDice metric's counts (Shit et al., CVPR 2021, section 3; no
 * ---- reference counterpart) ------------------------------------------------------------------------
 * Thinning is Guo & Hall's two-subiteration algorithm (CACM 32(3), 1989, algorithm A1), per class of a class
 * map cls int32 [N][H][W].  Class 0 is background; the classes are 1 .. 255, any other value counts as
 * background and comes out 0.  A neighbour of pixel q counts as set iff it lies inside the image and has the
 * class of q: thinning a multi-class map is the union of thinning each class mask on its own.  Neighbours of
 * (y, x):
 *   P9 (y-1, x-1)   P2 (y-1, x)   P3 (y-1, x+1)
 *   P8 (y,   x-1)                 P4 (y,   x+1)
 *   P7 (y+1, x-1)   P6 (y+1, x)   P5 (y+1, x+1)
 *   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)
 *   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
 *   N  = min(N1, N2)
 * A subiteration deletes (sets to 0) every non-zero pixel with C == 1, 2 <= N <= 3 and m == 0; the first
 * subiteration of a pass has m = (P6|P7|!P9) & P8, the second m = (P2|P3|!P5) & P4.  Each subiteration is
 * evaluated on the map as it stood before it.  A pass is the two subiterations in that order; thinning of an
 * image ends after the first pass that deletes nothing, or after max_passes passes.
 *
 * unetseg_skel_thin: out = cls with the deleted pixels set to 0; unconverged int32 [N] (may be NULL) = 1 iff
 * the last pass executed on image n still deleted a pixel.  max_passes = 0 runs no pass: out = cls (classes
 * outside 1 .. 255 zeroed) and unconverged = 0.  2 + ceil(max_passes / passes_per_launch) launches whatever
 * the data; none waits on the host; an image that has converged costs one flag read per block and launch.
 * ws: unetseg_skel_workspace(N, H, W) bytes, 16-byte aligned.  The result is bitwise reproducible and shows
 * neither the tile nor passes_per_launch.
 *
 * unetseg_skel_counts: out int64 [6] += over the pixels whose target is not `ignore` (-1: none)
 *   [0] #(skel_pred == c and target == c)   [1] #(skel_pred == c)
 *   [2] #(skel_target == c and pred == c)   [3] #(skel_target == c)
 *   [4] the number of images n with unconv_pred[n] | unconv_target[n]   [5] N
 * skel_pred / skel_target are unetseg_skel_thin's results for pred / target (with the ignored pixels set to 0
 * in both before thinning), unconv_* its unconverged arrays.
 *
 * Checked before any launch: null pointers (unconverged of unetseg_skel_thin may be NULL), N, H, W > 0,
 * max_passes >= 0, ws_bytes and a 16-byte aligned ws, 1 <= c <= 255, ignore != c.  The workspace query returns 0
 * for a shape it refuses. */
/* host only: the tile seams lie at the multiples of *tw and *th; one launch runs *passes_per_launch passes */
int unetseg_skel_tile(int* tw, int* th, int* passes_per_launch);
size_t unetseg_skel_workspace(int N, int H, int W); /* host only */
int unetseg_skel_thin(const int32_t* cls, int N, int H, int W, int max_passes, int32_t* out,
                      int32_t* unconverged /* [N], may be NULL */, void* ws, size_t ws_bytes, void* stream);
int unetseg_skel_counts(const int32_t* pred, const int32_t* target, const int32_t* skel_pred,
                        const int32_t* skel_target, const int32_t* unconv_pred, const int32_t* unconv_target, int N,
                        int H, int W, int c, int ignore, int64_t* out /* [6], accumulates */, void* stream);

/* ---- score histogram of the binary head: operating-point and calibration metrics (no reference
 * ---- counterpart) ---------------------------------------------------------------------------------
 * unetseg_curve_hist: hist u64 [2][K] += per valid pixel: row = (tgt == 1), column = bin(z).
 *   Layout.  out is planar fp32 [B][nch][P], nch in {1, 2}; tgt int64 [B][P].
 *   Score.   z = o0 for nch == 1; for nch == 2, z = o1 - o0, one IEEE fp32 subtraction (as the loss kernels
 *            form it).
 *   Edges.   edges is device fp32 [K - 1], ascending, 2 <= K <= unetseg_curve_max_bins() = 4096.
 *   Bin.     bin(z) = the number of edges theta with z > theta, in 0 .. K - 1.  A value equal to an edge goes
 *            to the lower bin; NaN compares false everywhere and lands in bin 0; -inf lands in bin 0 and +inf
 *            in bin K - 1.
 *   No arithmetic on z beyond that subtraction and comparisons (no expf): a CPU reference that holds the
 *            same edge array reproduces every count exactly.
 *   Unsorted edges: the bins are unspecified, but the bin index is computed so that it stays in 0 .. K - 1
 *            for any edge array: no write leaves hist.
 *   Ignored. Pixels with tgt == ignore_index are skipped; -1 means none.
 *   Positives.  A positive is tgt == 1 (the rule of unetseg_confusion); every other valid target is a negative.
 * One launch on the caller's stream, no host wait; integer counts and integer atomics only, so hist is bitwise
 * reproducible.  Thresholding at edge k - 1 (prediction = bin >= k, which is z > edges[k - 1]) gives tp / fp /
 * fn / tn as suffix sums of the two rows.
 * Checked before any launch: null pointers, nch in {1, 2}, 2 <= K <= 4096, B >= 0, P >= 0, B * P <= 2^40.  An
 * empty input (B * P == 0) launches nothing and returns 0. */
int unetseg_curve_max_bins(void); /* host only: the largest K */
int unetseg_curve_hist(const float* out, int nch, const int64_t* tgt, int B, long P, long ignore_index /* -1: none */,
                       const float* edges /* [K - 1] */, int K, unsigned long long* hist /* [2][K], accumulates */,
                       void* stream);

/* ---- object-level agreement of two class maps: Panoptic Quality, object F1, splits and merges (no
 * ---- reference counterpart; unetseg_hip/objects.py) ------------------------------------------------
 * pred, target int32 [N][H][W] (the caller sets the pixels outside the domain to 0 in both).  For a class c in
 * 1 .. 255 an object is a connected component of class c (unetseg_ccl_label at `connectivity`), named by its
 * root; a predicted object p and a target object g overlap when some pixel has pred == c, target == c,
 * root_pred == p and root_target == g; inter(p, g) is the number of such pixels and union = area_p + area_g -
 * inter.  The three stages share a workspace of unetseg_objects_workspace(N, H, W) bytes, 16-byte aligned:
 *   unetseg_objects_label: roots and stats of both maps (the ccl entry points), once per pair of maps;
 *   unetseg_objects_pairs: the table of the overlapping pairs of class c with their inter, one open-addressing
 *     table per image of cap = the smallest power of two >= max(H W, 2) slots (at most ceil(H W / 2) pairs are
 *     distinct: csrc/objects.hip).  aggregate != 0 gathers a block's runs in LDS first (the product path);
 *     0 sends every run to the table (the timing tool's comparison);
 *   unetseg_objects_match: out int64 [20] += from that table
 *     [0] target objects                       [1] predicted objects
 *     [2] target objects with >= 1 partner     [3] predicted objects with >= 1 partner
 *     [4] target objects with >= 2 (splits)    [5] predicted objects with >= 2 (merges)
 *     [6 + j], j = 0 .. 9: the pairs with 20 inter > (10 + j) union (IoU > 0.5, 0.55, .. 0.95), 64-bit integers
 *     [16] the sum over the pairs with 2 inter > union of floor(inter 2^32 / union), unsigned 64-bit
 *     [17] distinct overlapping pairs          [18] table insertions that found no slot (0 unless there is a bug)
 *     [19] N
 * All integer, integer atomics only, bitwise reproducible, on the caller's stream without a host wait; the number
 * of launches depends on the shape only.  Checked before any launch: null pointers, N, H, W >= 0, H W <= 2^31 - 1,
 * N H W <= 2^40, connectivity 4 or 8, 1 <= c <= 255, ws_bytes and the alignment of ws.  An empty batch
 * (N H W == 0) launches nothing and returns 0; the workspace query returns 0 for it and for a refused shape. */
/* host only: the pair kernel gathers the runs of a tile of *tw x *th pixels per block */
int unetseg_objects_tile(int* tw, int* th);
size_t unetseg_objects_workspace(int N, int H, int W); /* host only */
/* host only: at[0 .. 5) = byte offsets in the workspace of roots int32 [2][N][H][W], stats int32 [2][4][N][H][W],
 * keys u64 [N][cap] ((root_pred << 32) | root_target, all ones = empty), inter u32 [N][cap], degrees int32
 * [2][N][H][W] (pred before target); at[5] = cap */
int unetseg_objects_layout(int N, int H, int W, int64_t* at /* [6] */);
int unetseg_objects_label(const int32_t* pred, const int32_t* target, int N, int H, int W, int connectivity, void* ws,
                          size_t ws_bytes, void* stream);
int unetseg_objects_pairs(const int32_t* pred, const int32_t* target, int N, int H, int W, int c, int aggregate,
                          void* ws, size_t ws_bytes, void* stream);
int unetseg_objects_match(const int32_t* pred, const int32_t* target, int N, int H, int W, int c,
                          int64_t* out /* [20], accumulates */, void* ws, size_t ws_bytes, void* stream);

/* ---- vector contours of a class map: crack loops, vertices, signed areas (no reference counterpart;
 * ---- unetseg_hip/contours.py, predict.py --polygons) --------------------------------------------------
 * cls int32 [N][H][W], class 0 background, components and roots those of unetseg_ccl_label at `connectivity`.
 * Pixel (y, x) covers [x, x+1] x [y, y+1].  A crack is a side of a pixel of a non-zero class whose 4-neighbour
 * across it has another class or lies outside the image; side 0 top (x, y) -> (x+1, y), 1 right, 2 bottom, 3 left,
 * clockwise on screen with the owner on the right; crack id = (y W + x) 4 + side.  At the head corner, with F the
 * pixel ahead on the owner's side and D the pixel ahead on the other side ("in" = inside the image and of the
 * owner's class): connectivity 8: D in -> D's crack (left turn), else F in -> F's (straight on), else the owner's
 * next side (right turn); connectivity 4: F out -> right turn, else D out -> straight on, else left turn.  The
 * successor map is a bijection: the cracks fall into closed loops.  A loop's leader is its smallest crack id; it
 * is the outer loop of its component iff leader == 4 root, else a hole.  A vertex is the tail corner of a crack
 * whose side differs from its predecessor's.  The stages, on the caller's stream, no block waiting on another:
 *   unetseg_contours_mask: mask uint8 [N][H][W] (bit s = side s is a crack) and seg int32 [N][H][ceil(W / 64)],
 *     the cracks of every 64-pixel row segment.  The caller scans seg (exclusive, int64): base, and the total M;
 *     dense crack indices 0 .. M-1 are in crack-id order.  The other stages share a workspace of
 *     unetseg_contours_workspace(M) bytes, 16-byte aligned, which scales with M and not with the pixels;
 *   unetseg_contours_link: off int32 [N][H][W] (the dense index of each pixel's first crack) and, per crack, its
 *     id in the flat batch, its successor and whether its tail is a vertex;
 *   unetseg_contours_rank: pointer doubling, 2 R + 2 launches with R = ceil(log2 M) rounded up to even: the leader
 *     of every crack, then the cracks, vertices and doubled shoelace area (64-bit) from every crack to the end of
 *     its loop cut before the leader; a leader holds its loop's totals;
 *   unetseg_contours_emit: the rows (image, class, root, hole, first, count, area, cracks) of the loops led by
 *     `leaders` (the caller orders them by (image, root, leader) and scans their vertex counts into `first`) and
 *     the vertices (x, y) of loop i at first[i] onward, in travel order from the first vertex at or after the
 *     leader's tail.  area = the signed shoelace area (> 0 outer, < 0 hole), cracks = the loop's length.
 * All integer and a function of the input only.  Checked before any launch: null pointers, N, H, W >= 0,
 * H W <= 2^29 (no id, count or area leaves int32), connectivity 4 or 8, 1 <= M <= 2^31 - 1, ws_bytes and the
 * alignment of ws.  An empty batch launches nothing and returns 0.  The failure word counts successors that were
 * no crack (0 unless there is a bug; such a crack becomes its own successor, so nothing is read out of bounds). */
/* host only: the mask kernel holds a tile of *tw x *th pixels and its halo in LDS */
int unetseg_contours_tile(int* tw, int* th);
size_t unetseg_contours_workspace(long M); /* host only; 0 for a refused M */
/* host only: at[0 .. 7) = byte offsets in the workspace of the crack ids int64 [M] ((n H W + y W + x) 4 + side),
 * successors, vertex flags and leaders int32 [M], and rank's cracks int32 [M], vertices int32 [M] and doubled
 * areas int64 [M]; at[7] = the failure word uint32 */
int unetseg_contours_layout(long M, int64_t* at /* [8] */);
int unetseg_contours_mask(const int32_t* cls, int N, int H, int W, uint8_t* mask, int32_t* seg, void* stream);
int unetseg_contours_link(const int32_t* cls, const uint8_t* mask, const int64_t* base, int N, int H, int W,
                          int connectivity, long M, int32_t* off, void* ws, size_t ws_bytes, void* stream);
int unetseg_contours_rank(int N, int H, int W, long M, void* ws, size_t ws_bytes, void* stream);
int unetseg_contours_emit(const int32_t* cls, const int32_t* root, int N, int H, int W, long M,
                          const int32_t* leaders, const int32_t* first, int L, int32_t* loops /* [L][8] */,
                          int32_t* vertices /* [V][2] */, long V, void* ws, size_t ws_bytes, void* stream);

/* ---- device augmentation of the loader (utils/hf_dataloader.py:67-105, 111-180, 183-213) -------
 * Replaces HFUnetDataset.get_random_data + preprocess + hf_unet_dataset_collate for one batch:
 * PIL BICUBIC image / NEAREST mask resize (bit-exact), flip, paste on the grey / zero canvas,
 * OpenCV-style HSV jitter (hsv flag), /255, label binarise / clamp, one-hot.
 * desc: int64 [B][20] per-sample descriptors (host copy for validation + device copy), tables:
 * int32 per-sample resize / nearest / LUT tables (host + device), src / msk: packed uint8 RGB images
 * and L masks, tmp / rsz: uint8 scratch.  Outputs: img fp32 [B][3][H][W], png int64 [B][H][W],
 * onehot fp32 [B][H][W][num_classes+1] (may be NULL). */
int unetseg_augment_tables_len(long long nw, long long nh, long long ksh, long long ksv, long long hsv);
int unetseg_augment_batch(const long long* desc_host, const long long* desc, int B, const int* tables_host,
                          const int* tables, long long n_tables, const uint8_t* src, long long src_bytes,
                          const uint8_t* msk, long long msk_bytes, uint8_t* tmp, long long tmp_bytes, uint8_t* rsz,
                          long long rsz_bytes, int H, int W, int num_classes, int binary, float* img, long long* png,
                          float* onehot, void* stream);
/* The same with the per-sample tables built on the device (aug_tables: Resample.c precompute_coeffs /
 * normalize_coeffs_8bpc, Geometry.c ImagingScaleAffine and the reference's HSV LUTs restated in
 * float64, bit-identical to utils/augment_tables.py): hsv_r float64 [B][3] (device; the drawn HSV
 * factors, hf_dataloader.py:166), tables: device int32 scratch of n_tables entries at the
 * descriptors' offsets.  The host decodes, draws and packs pixels only. */
int unetseg_augment_batch_dev(const long long* desc_host, const long long* desc, int B, const double* hsv_r,
                              int* tables, long long n_tables, const uint8_t* src, long long src_bytes,
                              const uint8_t* msk, long long msk_bytes, uint8_t* tmp, long long tmp_bytes,
                              uint8_t* rsz, long long rsz_bytes, int H, int W, int num_classes, int binary, float* img,
                              long long* png, float* onehot, void* stream);
/* the device-built tables alone (parity tests); max_tasks >= max over samples of nw + nh + 2 (+768) */
int unetseg_augment_tables_dev(const long long* desc, int B, const double* hsv_r, int* tables, int max_tasks,
                               void* stream);

/* ---- streams ---------------------------------------------------------------------------------- */
/* `waiter` waits for everything enqueued so far on `signaler` (device-scope release event; no
   reference counterpart: orders the weight-gradient stream against the compute stream) */
int unetseg_stream_wait(void* waiter, void* signaler);
/* a stream restricted to the CUs set in mask[0 .. n_words) (bit i of word w = CU 32 w + i); *out = the
   hipStream_t (no reference counterpart: keeps the weight-gradient stream's persistent kernels off
   part of the chip, UNETSEG_SIDE_CUMASK) */
int unetseg_stream_create_cumask(const unsigned* mask, int n_words, void** out);

/* ---- multitask classification head (model/unet_multitask.py:73-80) -------------------------- */
/* global average pooling over x NHWC [B][HW][C], a channel slice of pixel stride ldx >= C (accessed by element: any
 * C > 0, ldx and c0): g fp32 [B][C] = the mean over the HW pixels (summed in double), written; its backward
 * dx (+)= dg / HW at every pixel (accumulate != 0 adds onto dx).  B == 0 (gap_bwd: or HW == 0) returns 0 without a
 * launch; gap_fwd refuses HW == 0 with B > 0 (a mean over no pixels).  Nothing outside channels [c0, c0 + C) of the
 * B * HW pixels of dx, and nothing past g's B * C floats, is written. */
int unetseg_gap_fwd(int dtype, const void* x, int ldx, int B, int HW, int C, float* g, void* stream);
int unetseg_gap_bwd(int dtype, const float* dg, int B, int HW, int C, void* dx, int ldx, int accumulate,
                    void* stream);
/* y = [dropout(relu(.))] (x W^T + b); act 1 = ReLU+dropout(p_drop) with hashed mask from seed or mask_in */
int unetseg_linear_fwd(const float* x, const float* W, const float* bias, int B, int I, int O, int act, float p_drop,
                       unsigned long long seed, const float* mask_in, float* mask_out, float* pre, float* y,
                       void* stream);
int unetseg_linear_bwd(const float* dy, const float* pre, const float* mask, float p_drop, int act, const float* x,
                       const float* W, int B, int I, int O, float* dx, float* dW, float* db, float* scratch,
                       void* stream);

/* ---- optimizer: torch.optim.Adam with coupled weight decay (train.py:62-78) over one flat fp32
 *      arena; grad_scale (device pointer, may be NULL) is the loss scale the gradients carry: g is
 *      divided by grad_scale[0] first (GradScaler's unscale), as g * (1 / grad_scale[0]) ------------ */
int unetseg_adam(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 float wd, int step, const float* grad_scale, void* stream);
/* capturable Adam (hipGraph replay): hyper[0] = lr and *step (steps taken; advanced by one after the
   update) are read from device memory */
int unetseg_adam_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, float beta1,
                     float beta2, float eps, float wd, const float* grad_scale, void* stream);
/* Adam fused with an exponential moving average of the weights: the step of unetseg_adam (p, m, v bit-identical to
   it) and, in the same pass, ema = ema + one_minus_decay * (p_new - ema).  one_minus_decay in [0, 1]: the host
   forms 1 - d_t in double and rounds it once.  Any 4-byte-aligned slices; n == 0 launches nothing. */
int unetseg_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float beta1,
                     float beta2, float eps, float wd, int step, float one_minus_decay, const float* grad_scale,
                     void* stream);
/* the capturable form: 1 - d_t is formed in the kernel, in double, from the device step count t = *step + 1, with
   d_t = min(decay, (1 + t) / (10 + t)) when warmup != 0 and d_t = decay otherwise; then *step advances as in
   unetseg_adam_dev */
int unetseg_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, long n, const float* hyper,
                         int* step, float beta1, float beta2, float eps, float wd, float decay, int warmup,
                         const float* grad_scale, void* stream);
/* exchanges two fp32 arrays in place, bit for bit (a and b must not overlap) */
int unetseg_swap_f32(float* a, float* b, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNETSEG_HIP_H */
