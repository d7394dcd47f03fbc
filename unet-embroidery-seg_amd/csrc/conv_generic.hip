// The generic implicit-GEMM 2-D convolution kernels for NHWC activations on CDNA4 MFMA (gfx950): the
// fp32 parity path and the bf16 fallback of the dispatch in conv.hip.
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
#include "common.h"
#include "conv_generic.h"

namespace {

// TN kernel LDS image: [row][8 x 16B chunks], chunk swizzle makes ds_read_b128 fragment reads
// (16 rows x one chunk per 16-lane group) conflict free.
__device__ __forceinline__ int swz8(int row, int ch) { return ch ^ ((row >> 1) & 7); }
// wgrad LDS image: [k row][>=16 chunks]; rows {q, 8+q} (q<4) land on distinct chunk pairs so
// the transposed 4x16 reads of a 32-lane half are conflict free.
__device__ __forceinline__ int swz_tr(int row) { return ((row & 3) | ((row >> 1) & 4)) << 1; }

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

// split-K slabs of the generic kernel (K steps of 32 pixels in bf16, 16 in fp32)
int wgrad_generic_bk(int dtype) { return dtype == DT_BF16 ? 32 : 16; }

}  // namespace

int launch_generic(int dtype, const IgemmArgs& a, hipStream_t st) {
  return dtype == DT_BF16 ? launch_generic_t<bf16>(a, st) : launch_generic_t<float>(a, st);
}

int wgrad_generic_splits(int dtype, int Cout, int Ng, long Kpix) {
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

int launch_wgrad_generic(int dtype, WgradArgs a, int splits, hipStream_t st) {
  const int bkw = wgrad_generic_bk(dtype);
  a.kt_per_split = (int)(((a.Kpix + bkw - 1) / bkw + splits - 1) / splits);
  dim3 grid(ceil_div(a.Cout, 128), ceil_div(a.Ng, 128), splits);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL(wgrad_kernel<bf16>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(wgrad_kernel<float>, grid, dim3(256), 0, st, a);
  return 0;
}
