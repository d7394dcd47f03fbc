// Argument blocks and launchers of the generic conv kernels (conv_generic.hip: the fp32 parity path and
// the bf16 fallback) and of the split-K reduce every weight-gradient family feeds
// (conv_wgrad_reduce.hip), dispatched from conv.hip.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kBM = 128;  // GEMM M tile of the TN kernel (also the BN-statistics row tile)

struct IgemmArgs {
  const void* x1;
  const void* x2;
  int c1, c2, ldc1, ldc2;  // concat sources (c2 may be 0); channel counts and pixel strides
  int N, H, W;             // gather-source tensor
  int hc, wc;              // GEMM-row pixel grid per image
  int istride;             // source row = hh*istride + dh
  int r0, rs, nr, dh0, dhs;
  int s0, ss, ns, dw0, dws;
  int S;                   // kernel width of the weight image
  int cin;                 // GEMM K per tap = c1 + c2
  const void* wt;
  long ldw;                // weight row length (R*S*cin)
  int Ng;                  // GEMM N
  int ostride, ph, pw, OH, OW;  // output pixel = (n, hh*ostride+ph, ww*ostride+pw)
  void* y;
  int ldy, accumulate;
  const float* bias;
  const float* escale;     // per-output-channel epilogue scale (generic kernel only; may be NULL)
  const float* in_sc;      // input BN-ReLU prologue (fast register-staged kernels only; may be NULL)
  const float* in_sh;
  int relu;
  float* stats;            // [M tiles][2][Ng] (sum, M2 about the tile mean)
  int stats_ld;
  int M;
};

struct WgradArgs {
  const void* x1;
  const void* x2;
  int c1, c2, ldc1, ldc2;
  int N, H, W, P, Q, stride, pad, R, S;
  const void* dy;
  int ldy, Cout;
  int cin, Ng;
  long Kpix;
  int kt_per_split;  // set by launch_wgrad_generic
  float* ws;  // [split][Cout][Ng]
};

// the generic implicit-GEMM kernel: either dtype, and the only one with the affine epilogue (escale)
int launch_generic(int dtype, const IgemmArgs& a, hipStream_t st);
// split-K slabs of the generic weight-gradient kernel, and its launch into a.ws
int wgrad_generic_splits(int dtype, int Cout, int Ng, long Kpix);
int launch_wgrad_generic(int dtype, WgradArgs a, int splits, hipStream_t st);

// dW[k][c][tap] (+)= sum_z ws[z][k][tap*cin + c] for c < dw_c, deterministic.
// rows_out (<= cout; -1 = cout): dW rows written -- the rest are the zero-padded output channels of a
// padded-K GEMM (unetseg_conv2d_wgrad_rows), summed in the slabs but never stored
void launch_wgrad_reduce(const float* ws, int splits, int cout, int cin, int taps, float* dw, int dw_c,
                         int accumulate, hipStream_t st, int rows_out = -1);
// dw[k][c][r][s] (+)= v[k][s*8 + c][r] (c < C, s < 7): the stem's reduced virtual gradient into [K][C][7][7]
void launch_stem_wgrad_remap(const float* v, int K, int C, float* dw, int accumulate, hipStream_t st);
