// Implicit-GEMM 2-D convolution for NHWC activations on CDNA4 MFMA (gfx950).
//
// Replaces every nn.Conv2d of the reference hot path:
//   model/resnet_backbone.py:19,33,126,167   model/unet_resnet.py:17,19,72,74,78
//   model/unet_plain.py:9,12,69              model/unet_attention.py:16,20,24,76
//   model/unet_multitask.py:17-18,62,64,69
//
// Three GEMM views of one conv (x: [N,H,W,Cin] NHWC, y: [N,P,Q,Cout], w: [Cout][Cin][R][S]):
//   fwd   : Y[m=(n,p,q)][k_out]  = sum_{(r,s,c)} X[n][p*st-pad+r][q*st-pad+s][c] * Wk[k_out][r][s][c]
//   dgrad : dX[m=(n,h,w)][c]     = sum_{(r,s,k)} dY[n][(h+pad-r)/st][(w+pad-s)/st][k] * Wt[c][r][s][k]
//           (stride 2: four output-parity classes, each a stride-1 gather over its own tap subset)
//   wgrad : dW[k_out][(r,s,c)]   = sum_{m=(n,p,q)} dY[m][k_out] * X[n][p*st-pad+r][q*st-pad+s][c]
// fwd and dgrad are the same "TN" kernel (both operands K-contiguous, gathered with 16-B loads);
// wgrad has both operands pixel-major and reads MFMA fragments with ds_read_b64_tr_b16.
//
// bf16 path: v_mfma_f32_16x16x32_bf16, fp32 accumulate.  fp32 path (parity mode):
// v_mfma_f32_16x16x4_f32 (exact f32 fma chain).  256 threads = 4 waves in 2x2, one 16x16
// accumulator per (i,j) subtile; register-staged global->LDS double buffering, one barrier per
// K step; LDS rows are 128 B (TN) / 256 B (wgrad) with XOR chunk swizzles chosen so that the
// fragment reads are bank-conflict free.
#include <cstdlib>

#include "common.h"
#include "conv_fast.h"

namespace {

constexpr int kBM = 128;  // GEMM M tile of the TN kernel (also the BN-statistics row tile)

// TN kernel LDS image: [row][8 x 16B chunks], chunk swizzle makes ds_read_b128 fragment reads
// (16 rows x one chunk per 16-lane group) conflict free.
__device__ __forceinline__ int swz8(int row, int ch) { return ch ^ ((row >> 1) & 7); }
// wgrad LDS image: [k row][>=16 chunks]; rows {q, 8+q} (q<4) land on distinct chunk pairs so
// the transposed 4x16 reads of a 32-lane half are conflict free.
__device__ __forceinline__ int swz_tr(int row) { return ((row & 3) | ((row >> 1) & 4)) << 1; }

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

template <typename T, int BN>
__global__ __launch_bounds__(256) void igemm_tn_kernel(IgemmArgs a) {
  constexpr bool kBF = sizeof(T) == 2;
  constexpr int VE = 16 / sizeof(T);
  constexpr int BK = 8 * VE;
  constexpr int BM = kBM;
  constexpr int A_PER = BM / 32, B_PER = BN / 32;
  constexpr int FM = BM / 32, FN = BN / 32;
  __shared__ __attribute__((aligned(16))) uint4 lds[2][(BM + BN) * 8];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int kv = tid & 7, rb = tid >> 3;
  const int hw = a.hc * a.wc;

  int a_nb[A_PER], a_ih[A_PER], a_iw[A_PER];
  bool a_ok[A_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    int m = m0 + rb + 32 * i;
    a_ok[i] = m < a.M;
    int mm = a_ok[i] ? m : 0;
    int nb = mm / hw, rem = mm - nb * hw;
    int hh = rem / a.wc, ww = rem - hh * a.wc;
    a_nb[i] = nb * a.H;
    a_ih[i] = hh * a.istride;
    a_iw[i] = ww * a.istride;
  }
  const T* x1 = (const T*)a.x1;
  const T* x2 = (const T*)a.x2;
  const T* wt = (const T*)a.wt;

  int kc = kv * VE, jr = 0, js = 0;
  while (kc >= a.cin) {
    kc -= a.cin;
    if (++js == a.ns) { js = 0; ++jr; }
  }
  const long Ktot = (long)a.nr * a.ns * a.cin;
  const int nkt = (int)((Ktot + BK - 1) / BK);

  uint4 ra[A_PER], rbv[B_PER];
  auto gload = [&]() {
    const bool kok = jr < a.nr;
    const int r = a.r0 + a.rs * jr, s = a.s0 + a.ss * js;
    const int dh = a.dh0 + a.dhs * jr, dw = a.dw0 + a.dws * js;
    const bool first = kc < a.c1;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      int ih = a_ih[i] + dh, iw = a_iw[i] + dw;
      bool ok = kok && a_ok[i] && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ok) {
        long pix = (long)(a_nb[i] + ih) * a.W + iw;
        const T* p = first ? x1 + pix * a.ldc1 + kc : x2 + pix * a.ldc2 + (kc - a.c1);
        v = *reinterpret_cast<const uint4*>(p);
      }
      ra[i] = v;
    }
    const long wofs = (long)(r * a.S + s) * a.cin + kc;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      int n = n0 + rb + 32 * i;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (kok && n < a.Ng) v = *reinterpret_cast<const uint4*>(wt + (long)n * a.ldw + wofs);
      rbv[i] = v;
    }
    kc += BK;
    while (kc >= a.cin) {
      kc -= a.cin;
      if (++js == a.ns) { js = 0; ++jr; }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      int row = rb + 32 * i;
      lds[buf][row * 8 + swz8(row, kv)] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      int row = rb + 32 * i;
      lds[buf][(BM + row) * 8 + swz8(row, kv)] = rbv[i];
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nkt > 0) {
    gload();
    sstore(0);
    __syncthreads();
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) gload();
    const uint4* As = &lds[cur][0];
    const uint4* Bs = &lds[cur][BM * 8];
    if constexpr (kBF) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + (lane >> 4);
        bf16x8 af[FM], bfr[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          int row = wm * (BM / 2) + i * 16 + (lane & 15);
          uint4 v = As[row * 8 + swz8(row, ch)];
          af[i] = *reinterpret_cast<bf16x8*>(&v);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          int row = wn * (BN / 2) + j * 16 + (lane & 15);
          uint4 v = Bs[row * 8 + swz8(row, ch)];
          bfr[j] = *reinterpret_cast<bf16x8*>(&v);
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    } else {
      const float* Af = reinterpret_cast<const float*>(As);
      const float* Bf = reinterpret_cast<const float*>(Bs);
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        float af[FM], bfr[FN];
        const int e = lane >> 4;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          int row = wm * (BM / 2) + i * 16 + (lane & 15);
          af[i] = Af[(row * 8 + swz8(row, kk)) * 4 + e];
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          int row = wn * (BN / 2) + j * 16 + (lane & 15);
          bfr[j] = Bf[(row * 8 + swz8(row, kk)) * 4 + e];
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) sstore(cur ^ 1);
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  T* y = (T*)a.y;
  const int ohw = a.hc * a.wc;
  float colsum[FN], colm2[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) colsum[j] = colm2[j] = 0.f;
  float vals[FM][FN][4];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + wm * (BM / 2) + i * 16 + (lane >> 4) * 4 + e;
      const bool mok = m < a.M;
      long opix = 0;
      if (mok) {
        int nb = m / ohw, rem = m - nb * ohw;
        int hh = rem / a.wc, ww = rem - hh * a.wc;
        opix = ((long)nb * a.OH + hh * a.ostride + a.ph) * a.OW + ww * a.ostride + a.pw;
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 16 + (lane & 15);
        float v = acc[i][j][e];
        float vr = 0.f;
        if (mok && n < a.Ng) {
          if (a.escale) v = fmaf(v, a.escale[n], a.bias ? a.bias[n] : 0.f);  // == bn_apply's fmaf
          else if (a.bias) v += a.bias[n];
          if (a.relu) v = fmaxf(v, 0.f);
          T* p = y + opix * a.ldy + n;
          if (a.accumulate) v += (float)(*p);
          T t = (T)v;
          *p = t;
          vr = (float)t;
          colsum[j] += vr;
        }
        vals[i][j][e] = vr;
      }
    }
  }
  if (a.stats) {  // per-tile column sum and M2 about the tile mean (Chan merge in bn_finalize)
    __syncthreads();
    float* red = reinterpret_cast<float*>(&lds[0][0]);  // [0,2BN): sums per (wm, col); [2BN,4BN): M2
    const int cnt = min(BM, a.M - m0);
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      float s = colsum[j];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) red[wm * BN + wn * (BN / 2) + j * 16 + lane] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = wn * (BN / 2) + j * 16 + (lane & 15);
      const float mean = (red[col] + red[BN + col]) / (float)cnt;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + wm * (BM / 2) + i * 16 + (lane >> 4) * 4 + e;
          if (m < a.M) {
            const float d = vals[i][j][e] - mean;
            q += d * d;
          }
        }
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      colm2[j] = q;
    }
#pragma unroll
    for (int j = 0; j < FN; ++j)
      if (lane < 16) red[2 * BN + wm * BN + wn * (BN / 2) + j * 16 + lane] = colm2[j];
    __syncthreads();
    for (int c = tid; c < BN; c += 256) {
      const int n = n0 + c;
      if (n < a.Ng) {
        a.stats[(long)blockIdx.x * 2 * a.Ng + n] = red[c] + red[BN + c];
        a.stats[(long)blockIdx.x * 2 * a.Ng + a.Ng + n] = red[2 * BN + c] + red[3 * BN + c];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// wgrad: C[k_out][(r,s,c)] = sum_pix dY[pix][k_out] * im2col(X)[pix][(r,s,c)], split-K over pixels
// ---------------------------------------------------------------------------------------
struct WgradArgs {
  const void* x1;
  const void* x2;
  int c1, c2, ldc1, ldc2;
  int N, H, W, P, Q, stride, pad, R, S;
  const void* dy;
  int ldy, Cout;
  int cin, Ng;
  long Kpix;
  int kt_per_split;
  float* ws;  // [split][Cout][Ng]
};

template <typename T>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
  constexpr bool kBF = sizeof(T) == 2;
  constexpr int VE = 16 / sizeof(T);
  constexpr int BM = 128, BN = 128;
  constexpr int CPR = BM * (int)sizeof(T) / 16;  // 16-B chunks per LDS row
  constexpr int BKW = kBF ? 32 : 16;             // pixels per K step
  constexpr int RPP = 256 / CPR;                 // rows per load pass
  constexpr int PASSES = BKW / RPP;
  constexpr int FM = 4, FN = 4;
  __shared__ __attribute__((aligned(16))) uint4 lds[2][2 * BKW * CPR];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int cv = tid % CPR, rr = tid / CPR;
  const long nkt_total = (a.Kpix + BKW - 1) / BKW;
  const long kt0 = (long)blockIdx.z * a.kt_per_split;
  const long kt1 = min(nkt_total, kt0 + a.kt_per_split);

  const T* dy = (const T*)a.dy;
  const int cout = m0 + cv * VE;
  const bool a_col_ok = cout < a.Cout;
  const int nn = n0 + cv * VE;
  const bool b_col_ok = nn < a.Ng;
  int tap = b_col_ok ? nn / a.cin : 0;
  int cc = b_col_ok ? nn - tap * a.cin : 0;
  const int rr_ = tap / a.S, ss_ = tap - rr_ * a.S;
  const int dh = rr_ - a.pad, dw = ss_ - a.pad;
  const bool first = cc < a.c1;
  const T* xb = first ? (const T*)a.x1 + cc : (const T*)a.x2 + (cc - a.c1);
  const int ldx = first ? a.ldc1 : a.ldc2;

  // pixel state of each of this thread's rows
  int pn[PASSES], pp[PASSES], pq[PASSES];
  long pk[PASSES];
#pragma unroll
  for (int i = 0; i < PASSES; ++i) {
    long k = kt0 * BKW + rr + RPP * i;
    pk[i] = k;
    long kk = k < a.Kpix ? k : 0;
    int nb = (int)(kk / ((long)a.P * a.Q));
    int rem = (int)(kk - (long)nb * a.P * a.Q);
    pn[i] = nb;
    pp[i] = rem / a.Q;
    pq[i] = rem - pp[i] * a.Q;
  }
  uint4 ra[PASSES], rbv[PASSES];
  auto gload = [&]() {
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const bool kok = pk[i] < a.Kpix;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (kok && a_col_ok) v = *reinterpret_cast<const uint4*>(dy + pk[i] * a.ldy + cout);
      ra[i] = v;
      uint4 u = make_uint4(0, 0, 0, 0);
      const int ih = pp[i] * a.stride + dh, iw = pq[i] * a.stride + dw;
      if (kok && b_col_ok && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
        u = *reinterpret_cast<const uint4*>(xb + ((long)(pn[i] * a.H + ih) * a.W + iw) * ldx);
      rbv[i] = u;
      pk[i] += BKW;
      pq[i] += BKW;
      while (pq[i] >= a.Q) {
        pq[i] -= a.Q;
        if (++pp[i] >= a.P) { pp[i] = 0; ++pn[i]; }
      }
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
      const int row = rr + RPP * i;
      lds[buf][row * CPR + (cv ^ swz_tr(row))] = ra[i];
      lds[buf][(BKW + row) * CPR + (cv ^ swz_tr(row))] = rbv[i];
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (int)(kt1 - kt0);
  if (nkt > 0) {
    gload();
    sstore(0);
    __syncthreads();
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) gload();
    const uint4* As = &lds[cur][0];
    const uint4* Bs = &lds[cur][BKW * CPR];
    if constexpr (kBF) {
      const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
      bf16x8 af[FM], bfr[FN];
      auto trfrag = [&](const uint4* base, int col0) -> bf16x8 {
        const int chunk = (col0 >> 3) + (p >> 1);
        const int r_a = 8 * g + q, r_b = 8 * g + q + 4;
        const char* b = reinterpret_cast<const char*>(base);
        const char* pa = b + r_a * (CPR * 16) + ((chunk ^ swz_tr(r_a)) * 16) + (p & 1) * 8;
        const char* pb = b + r_b * (CPR * 16) + ((chunk ^ swz_tr(r_b)) * 16) + (p & 1) * 8;
        s16x4 va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(pa));
        s16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(pb));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        s16x8 v = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
        return *reinterpret_cast<bf16x8*>(&v);
      };
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = trfrag(As, wm * 64 + i * 16);
#pragma unroll
      for (int j = 0; j < FN; ++j) bfr[j] = trfrag(Bs, wn * 64 + j * 16);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    } else {
      const float* Af = reinterpret_cast<const float*>(As);
      const float* Bf = reinterpret_cast<const float*>(Bs);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = kk * 4 + (lane >> 4);
        float af[FM], bfr[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int m = wm * 64 + i * 16 + (lane & 15);
          af[i] = Af[k * (CPR * 4) + (((m >> 2) ^ swz_tr(k)) << 2) + (m & 3)];
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = wn * 64 + j * 16 + (lane & 15);
          bfr[j] = Bf[k * (CPR * 4) + (((n >> 2) ^ swz_tr(k)) << 2) + (n & 3)];
        }
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
    if (kt + 1 < nkt) sstore(cur ^ 1);
    __syncthreads();
  }
  float* ws = a.ws + (long)blockIdx.z * a.Cout * a.Ng;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + e;
      if (m >= a.Cout) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * 64 + j * 16 + (lane & 15);
        if (n < a.Ng) ws[(long)m * a.Ng + n] = acc[i][j][e];
      }
    }
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
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
      v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
      v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
    }
    for (; z < splits; z += SL) {
      const float4 a = p[z * s4];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
  }
  if constexpr (SL > 1) {
    red[sl][it] = v;
    __syncthreads();
    if (sl == 0)
      for (int j = 1; j < SL; ++j) {
        const float4 a = red[j][it];
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
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
      for (int u = 0; u < 8; ++u) {
        v.x += a[u].x; v.y += a[u].y; v.z += a[u].z; v.w += a[u].w;
      }
    }
    for (; z + 3 < z1; z += 4) {
      const float4 a = p[z * s4], b = p[(z + 1) * s4], c = p[(z + 2) * s4], d = p[(z + 3) * s4];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
      v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
      v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
      v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
    }
    for (; z < z1; ++z) {
      const float4 a = p[z * s4];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
    }
  }
  if constexpr (SL > 1) {
    red[sl][it] = v;
    __syncthreads();
    if (sl != 0) return;
    v = red[0][it];
    for (int j = 1; j < SL; ++j) {
      const float4 a = red[j][it];
      v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
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
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
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

// Few slabs of a multi-tap filter: the transposing kernel (coalesced dW runs, one lane group per
// block); otherwise the split-parallel kernel with ~4 (up to splits / 16) slabs per lane.
// rows_out (<= cout; -1 = cout): dW rows written -- the rest are the zero-padded output channels of a
// padded-K GEMM (unetseg_conv2d_wgrad_rows), summed in the slabs but never stored
static void launch_wgrad_reduce(const float* ws, int splits, int cout, int cin, int taps, float* dw, int dw_c,
                                int accumulate, hipStream_t st, int rows_out = -1) {
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

// fp32 [K][C][R][S] -> T [K][R][S][Cpad] (zero-padded channels) and optionally T [C][R][S][K]
template <typename T>
__global__ void pack_weights_kernel(const float* w, int K, int C, int R, int S, int Cpad, T* wk, T* wt) {
  const long total = (long)K * R * S * Cpad;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const int c = (int)(t % Cpad); t /= Cpad;
    const int s = (int)(t % S); t /= S;
    const int r = (int)(t % R); t /= R;
    const int k = (int)t;
    float v = c < C ? w[(((long)k * C + c) * R + r) * S + s] : 0.f;
    wk[i] = (T)v;
    if (wt && c < C) wt[(((long)c * R + r) * S + s) * K + k] = (T)v;
  }
}

// Batched pack of many conv weights: one block per (16 output channels x CT input channels) tile of
// one conv (desc[i].start = its first tile; unetseg_pack_tiles gives a conv's tile count).  The fp32
// source of a tile is 16 contiguous runs of CT*taps floats ([K][C][R][S] keeps c and the taps of
// one k together), read with unit-stride coalesced loads into LDS; the wk image ([K][R][S][Cpad])
// and the transposed wt image ([C][R][S][K]) are then written from LDS, channel-contiguous and
// k-contiguous respectively.  CT = pow2 in [8, 256] with CT * taps <= 512, so the tile fits the
// static LDS array; the odd row pitch (513) keeps both LDS read patterns conflict-free.
constexpr int kPackK = 16;

__host__ __device__ inline int pack_ct(int taps) {
  int ct = 256;
  while (ct > 8 && ct * taps > 512) ct >>= 1;
  return ct;
}

template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const UnetsegPackDesc* desc, int n) {
  __shared__ float tile[kPackK][513];
  const long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {  // last desc with start <= b
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].start <= b) lo = mid; else hi = mid - 1;
  }
  const UnetsegPackDesc d = desc[lo];
  const int taps = d.R * d.S;
  const int CT = pack_ct(taps);
  const int lt = (int)(b - d.start);
  const int ctiles = (d.Cpad + CT - 1) / CT;
  const int kt = lt / ctiles, ct = lt - kt * ctiles;
  const int k0 = kt * kPackK, c0 = ct * CT;
  const int run = CT * taps;                           // floats per k row of the tile
  const int vrun = max(0, min(CT, d.C - c0)) * taps;   // of which exist in the source
  const int t = threadIdx.x;
  if ((d.C * taps) % 4 == 0 && vrun % 4 == 0) {  // 16-B loads (rows start 16-B aligned)
    // every load of the tile issued before the first LDS store: unconditional (absent rows / columns
    // read the source's first float4 and are zeroed after); a load under the lane condition was
    // waited on by itself, one round trip per loop iteration
    const int run4 = run >> 2;
    constexpr int NIT = kPackK * 512 / 4 / 256;  // run <= 512
    float4 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = t + it * 256;
      const int kl = i / run4, j = (i - kl * run4) * 4;
      const int k = k0 + kl;
      const bool ok = i < kPackK * run4 && k < d.K && j < vrun;
      const float4 x = *reinterpret_cast<const float4*>(ok ? d.w + ((long)k * d.C + c0) * taps + j : d.w);
      v[it] = ok ? x : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = t + it * 256;
      if (i >= kPackK * run4) break;
      const int kl = i / run4, j = (i - kl * run4) * 4;
      tile[kl][j] = v[it].x;
      tile[kl][j + 1] = v[it].y;
      tile[kl][j + 2] = v[it].z;
      tile[kl][j + 3] = v[it].w;
    }
  } else {
    for (int i = t; i < kPackK * run; i += 256) {
      const int kl = i / run, j = i - kl * run;
      const int k = k0 + kl;
      tile[kl][j] = (k < d.K && j < vrun) ? d.w[((long)k * d.C + c0) * taps + j] : 0.f;
    }
  }
  __syncthreads();
  // wk[k][tap][c], c fastest, 4 channels per store (padding channels c in [C, Cpad) get the zeros
  // staged above)
  T* wk = reinterpret_cast<T*>(d.wk);
  if (d.Cpad % 4 == 0) {
    const int CT4 = CT >> 2;
    for (int i = t; i < kPackK * taps * CT4; i += 256) {
      const int c4 = i % CT4, rest = i / CT4;
      const int tap = rest % taps, kl = rest / taps;
      const int k = k0 + kl, c = c0 + c4 * 4;
      if (k >= d.K || c >= d.Cpad) continue;
      T o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)tile[kl][(c4 * 4 + e) * taps + tap];
      T* dst = wk + ((long)k * taps + tap) * d.Cpad + c;
      if (sizeof(T) == 2) *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(o);
      else *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
    }
  } else {
    for (int i = t; i < kPackK * taps * CT; i += 256) {
      const int cl = i % CT, rest = i / CT;
      const int tap = rest % taps, kl = rest / taps;
      const int k = k0 + kl, c = c0 + cl;
      if (k < d.K && c < d.Cpad) wk[((long)k * taps + tap) * d.Cpad + c] = (T)tile[kl][cl * taps + tap];
    }
  }
  if (d.wt) {  // wt[c][tap][k], k fastest, 8 output channels per store; rows of Kld (>= K) elements
    T* wt = reinterpret_cast<T*>(d.wt);
    const int ldk = d.Kld > 0 ? d.Kld : d.K;
    if (d.K % 8 == 0 && ldk % 8 == 0) {
      constexpr int K8 = kPackK / 8;
      for (int i = t; i < K8 * taps * CT; i += 256) {
        const int k8 = i % K8, rest = i / K8;
        const int tap = rest % taps, cl = rest / taps;
        const int k = k0 + k8 * 8, c = c0 + cl;
        if (k >= d.K || c >= d.C) continue;
        T o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (T)tile[k8 * 8 + e][cl * taps + tap];
        T* dst = wt + ((long)c * taps + tap) * ldk + k;
        if (sizeof(T) == 2) {
          *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
        } else {
          reinterpret_cast<uint4*>(dst)[0] = reinterpret_cast<const uint4*>(o)[0];
          reinterpret_cast<uint4*>(dst)[1] = reinterpret_cast<const uint4*>(o)[1];
        }
      }
    } else {
      for (int i = t; i < kPackK * taps * CT; i += 256) {
        const int kl = i % kPackK, rest = i / kPackK;
        const int tap = rest % taps, cl = rest / taps;
        const int k = k0 + kl, c = c0 + cl;
        if (k < d.K && c < d.C) wt[((long)c * taps + tap) * ldk + k] = (T)tile[kl][cl * taps + tap];
      }
    }
  }
}

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

// the generic implicit-GEMM kernel: either dtype, and the only one with the affine epilogue (escale)
template <typename T>
int launch_generic_t(const IgemmArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.Ng <= 0) return 0;
  US_CHECK_ARG(!a.in_sc, "conv: the BN-ReLU input prologue needs the fast bf16 path");
  dim3 grid(ceil_div(a.M, kBM), 1, 1);
  if (a.Ng <= 64) {
    grid.y = ceil_div(a.Ng, 64);
    hipLaunchKernelGGL((igemm_tn_kernel<T, 64>), grid, dim3(256), 0, st, a);
  } else {
    grid.y = ceil_div(a.Ng, 128);
    hipLaunchKernelGGL((igemm_tn_kernel<T, 128>), grid, dim3(256), 0, st, a);
  }
  US_LAUNCH_CHECK("igemm_tn");
  return 0;
}

int launch_generic(int dtype, const IgemmArgs& a, hipStream_t st) {
  return dtype == DT_BF16 ? launch_generic_t<bf16>(a, st) : launch_generic_t<float>(a, st);
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
// wgrad_reduce_kernel sums into dw; ws: fp32 workspace of unetseg_conv2d_wgrad_workspace() bytes.

// split-K slabs of the generic kernel (K steps of 32 pixels in bf16, 16 in fp32)
static int wgrad_generic_bk(int dtype) { return dtype == DT_BF16 ? 32 : 16; }
static int wgrad_generic_splits(int dtype, int Cout, int Ng, long Kpix) {
  const int bkw = wgrad_generic_bk(dtype);
  const int tiles = ceil_div(Cout, 128) * ceil_div(Ng, 128);
  const long nkt = (Kpix + bkw - 1) / bkw;
  int sp = ceil_div(768, tiles);
  if (sp < 1) sp = 1;
  const long max_sp = nkt / 8 > 0 ? nkt / 8 : 1;  // keep >= 8 K steps per split
  if (sp > max_sp) sp = (int)max_sp;
  if (sp > 64) sp = 64;
  return sp;
}

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
    const int bkw = wgrad_generic_bk(dtype);
    a.kt_per_split = (int)(((kpix + bkw - 1) / bkw + pl.splits - 1) / pl.splits);
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
    dim3 grid(ceil_div(cout, 128), ceil_div(pl.a.Ng, 128), pl.splits);
    if (dtype == DT_BF16)
      hipLaunchKernelGGL(wgrad_kernel<bf16>, grid, dim3(256), 0, st, pl.a);
    else
      hipLaunchKernelGGL(wgrad_kernel<float>, grid, dim3(256), 0, st, pl.a);
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

// All of a model's conv weights in one launch.  desc: DEVICE array of n UnetsegPackDesc with
// ascending `start` = first tile (desc[0].start == 0; a conv has ceil(K/32)*ceil(Cpad/64) tiles);
// total = number of tiles.
// blocks of unetseg_pack_conv_weights for one conv (its desc.start advances by this much)
UNETSEG_API int unetseg_pack_tiles(int K, int Cpad, int taps) {
  const int ct = pack_ct(taps);
  return ceil_div(K, kPackK) * ceil_div(Cpad, ct);
}

UNETSEG_API int unetseg_pack_conv_weights(int dtype, const void* desc, int n, long total, void* stream) {
  US_CHECK_ARG(desc && n > 0 && total > 0 && total < (1L << 31), "pack_conv_weights: bad args");
  hipStream_t st = (hipStream_t)stream;
  const UnetsegPackDesc* d = (const UnetsegPackDesc*)desc;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(pack_weights_batched_kernel<bf16>, dim3(total), dim3(256), 0, st, d, n);
  else
    hipLaunchKernelGGL(pack_weights_batched_kernel<float>, dim3(total), dim3(256), 0, st, d, n);
  US_LAUNCH_CHECK("pack_weights_batched");
  return 0;
}

// fp32 [K][C][R][S] -> dtype [K][R][S][Cpad] (+ optional dtype [C][R][S][K] for dgrad)
UNETSEG_API int unetseg_pack_conv_weight(int dtype, const float* w, int K, int C, int R, int S, int Cpad, void* wk,
                                         void* wt, void* stream) {
  US_CHECK_ARG(w && wk && Cpad >= C, "pack_conv_weight: bad args");
  const long total = (long)K * R * S * Cpad;
  int blocks = ceil_div(total, 256);
  if (blocks > 8192) blocks = 8192;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(pack_weights_kernel<bf16>, dim3(blocks), dim3(256), 0, st, w, K, C, R, S, Cpad, (bf16*)wk, (bf16*)wt);
  else
    hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(blocks), dim3(256), 0, st, w, K, C, R, S, Cpad, (float*)wk, (float*)wt);
  US_LAUNCH_CHECK("pack_weights");
  return 0;
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

__global__ void stem_pack_weight_kernel(const float* w, int K, int C, bf16* wk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over K*7*64
  if (i >= K * 7 * 64) return;
  const int k = i / 448, rem = i - k * 448, r = rem / 64, j = rem - r * 64;
  const int s = j >> 3, c = j & 7;
  wk[i] = (bf16)((s < 7 && c < C) ? w[((k * C + c) * 7 + r) * 7 + s] : 0.f);
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

UNETSEG_API int unetseg_stem_pack_weight(const float* w, int K, int C, void* wk, void* stream) {
  US_CHECK_ARG(w && wk && C >= 1 && C <= 8 && K % 8 == 0, "stem_pack_weight: bad args");
  hipLaunchKernelGGL(stem_pack_weight_kernel, dim3(ceil_div((long)K * 448, 256)), dim3(256), 0, (hipStream_t)stream, w,
                     K, C, (bf16*)wk);
  US_LAUNCH_CHECK("stem_pack_weight");
  return 0;
}

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
  hipLaunchKernelGGL(stem_wgrad_remap_kernel, dim3(ceil_div((long)K * C * 49, 256)), dim3(256), 0, st, v, K, C, dw,
                     accumulate);
  US_LAUNCH_CHECK("stem_wgrad");
  return 0;
}
