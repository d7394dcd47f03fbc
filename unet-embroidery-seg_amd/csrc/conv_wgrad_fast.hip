// Register-staged bf16 weight-gradient kernel of the fast conv family and its host side (the LDS-DMA
// ring kernel it yields to where that applies is conv_wgrad_ring.hip).  Pixels are consumed 32 per K
// step; fragments come from LDS with ds_read_b64_tr_b16.
#include "common.h"
#include "conv_fast.h"
#include "fast_util.h"


namespace {

// ------------------------------------------------------------------------------------------
// wgrad: C[cout][(tap, c)] = sum_pix dY[pix][cout] * X[n][p*st+dh][q*st+dw][c];
// tile BM couts x BN (tap,c) columns, K step = kWgBK consecutive output pixels.  Each thread
// tracks (image, row, col) of the pixels it stages and advances them by one step at a time, so
// any output width works.
// ------------------------------------------------------------------------------------------

// ROW32 (Q % 32 == 0): the 32 pixels of a K step are one run of an output row, so (image, row,
// first column) is wave-uniform scalar state and each staged row's offset is a scalar base plus a
// per-lane constant (tap shift, column, channel): a few VALU per row instead of re-deriving the
// pixel, its bounds and its 32-bit offset every step.
// PRE: X = relu(x1 * in_sc[c] + in_sh[c]) for the rows that exist (padding / past-the-end rows
// stay zero); each thread's 8 channels are fixed, so their coefficients live in registers.
template <int BM, int BN, int NWM, int NWN, bool ROW32 = false, bool PRE = false>
__global__ __launch_bounds__(64 * NWM * NWN) void wgrad_fast_kernel(FastWgradArgs a) {
  constexpr int NT = 64 * NWM * NWN;
  constexpr int BKW = kWgBK;
  constexpr int CPA = BM / 8, CPB = BN / 8;  // 16-B chunks per LDS row
  constexpr int A_PER = BKW * CPA / NT, B_PER = BKW * CPB / NT;
  constexpr int WTM = BM / NWM, WTN = BN / NWN;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  constexpr int STAGE = BKW * (CPA + CPB);  // uint4
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];  // [2][STAGE]
  static_assert(A_PER >= 1 && B_PER >= 1, "tile too small for the block");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / NWN, wn = wid % NWN;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  const __amdgpu_buffer_rsrc_t rdy = srd(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t r1 = srd(a.x1, a.x1_bytes);
  const __amdgpu_buffer_rsrc_t r2 = srd(a.x2 ? a.x2 : a.x1, a.x2 ? a.x2_bytes : 0u);

  // A (dY) chunk: column cv fixed, rows ra_row + (NT/CPA)*i
  int a_cv[A_PER], a_row[A_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    const int id = tid + NT * i;
    a_cv[i] = id % CPA;
    a_row[i] = id / CPA;
  }
  // B (X) chunk: column fixed -> (tap, c) fixed; row -> a pixel whose (n, p, q) we track
  int b_row[B_PER], b_dh[B_PER], b_dw[B_PER], b_src[B_PER], b_cv[B_PER];
  int b_n[B_PER], b_p[B_PER], b_q[B_PER];
  unsigned b_cb[B_PER];
  const long nkt_total = (a.Kpix + BKW - 1) / BKW;
  const long kt0 = (long)blockIdx.z * a.kt_per_split;
  const long kt1 = min(nkt_total, kt0 + a.kt_per_split);
  const int PQ = a.P * a.Q;
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int id = tid + NT * i;
    const int cv = id % CPB;
    b_cv[i] = cv;
    b_row[i] = id / CPB;
    const int nn = n0 + cv * 8;
    if (nn < a.Ng) {
      const int tap = nn / a.cin, c = nn - tap * a.cin;
      const int r = tap / a.S, s = tap - r * a.S;
      b_dh[i] = r - a.pad;
      b_dw[i] = s - a.padw;
      b_src[i] = c < a.c1 ? 0 : 1;
      b_cb[i] = (unsigned)(c < a.c1 ? c : c - a.c1) * 2u;
    } else {
      b_dh[i] = -(1 << 20);  // never valid
      b_dw[i] = 0;
      b_src[i] = 0;
      b_cb[i] = 0;
    }
    const long k = kt0 * BKW + b_row[i];
    const int nb = (int)(k / PQ), rem = (int)(k - (long)nb * PQ);
    b_n[i] = nb;
    b_p[i] = rem / a.Q;
    b_q[i] = rem - b_p[i] * a.Q;
  }
  const unsigned a_colb0 = (unsigned)m0 * 2u;
  float pre_sc[PRE ? B_PER : 1][8], pre_sh[PRE ? B_PER : 1][8];
  if constexpr (PRE) {
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int nn = n0 + b_cv[i] * 8;
      const int c = nn < a.Ng ? nn % a.cin : 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pre_sc[i][e] = nn < a.Ng ? a.in_sc[c + e] : 0.f;
        pre_sh[i][e] = nn < a.Ng ? a.in_sh[c + e] : 0.f;
      }
    }
  }
  unsigned b_okm = 0u;  // rows of the staged X set that exist (PRE)

  uint4 ra[A_PER], rbv[B_PER];
  // ---- ROW32 addressing: lane constants and scalar (image, row, column) of the next K step ----
  unsigned a_off[A_PER], b_l1[B_PER], b_l2[B_PER];
  int b_lw[B_PER];
  bool a_ok[A_PER];
  int s_n = 0, s_p = 0, s_q = 0;
  if constexpr (ROW32) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      a_ok[i] = (m0 + a_cv[i] * 8) < a.Cout;
      a_off[i] = (unsigned)a_row[i] * (unsigned)a.ldyb + a_colb0 + a_cv[i] * 16u;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      b_lw[i] = b_row[i] * a.stride + b_dw[i];
      const int dpix = b_dh[i] * a.W + b_lw[i];  // relative to the step's (row, first column) pixel
      b_l1[i] = (unsigned)(dpix * a.ldc1b) + b_cb[i];
      b_l2[i] = (unsigned)(dpix * a.ldc2b) + b_cb[i];
    }
    const long k = kt0 * BKW;
    s_n = (int)(k / PQ);
    const int rem = (int)(k - (long)s_n * PQ);
    s_p = rem / a.Q;
    s_q = rem - s_p * a.Q;
  }
  auto gload_row = [&](long kt) {
    const unsigned abase = (unsigned)(kt * BKW) * (unsigned)a.ldyb;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) ra[i] = bload(rdy, a_ok[i] ? abase + a_off[i] : kOOB);
    const int ihb = s_p * a.stride, iwb = s_q * a.stride;
    const int pixb = (s_n * a.H + ihb) * a.W + iwb;
    const unsigned base1 = (unsigned)pixb * (unsigned)a.ldc1b, base2 = (unsigned)pixb * (unsigned)a.ldc2b;
    b_okm = 0u;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const bool ok = (unsigned)(ihb + b_dh[i]) < (unsigned)a.H && (unsigned)(iwb + b_lw[i]) < (unsigned)a.W;
      b_okm |= ok ? 1u << i : 0u;
      if (b_src[i] == 0)
        rbv[i] = bload(r1, ok ? base1 + b_l1[i] : kOOB);
      else
        rbv[i] = bload(r2, ok ? base2 + b_l2[i] : kOOB);
    }
    s_q += BKW;
    if (s_q == a.Q) {
      s_q = 0;
      if (++s_p == a.P) {
        s_p = 0;
        ++s_n;
      }
    }
  };
  auto gload = [&](long kt) {
    if constexpr (ROW32) {
      gload_row(kt);
      return;
    }
    const long k0 = kt * BKW;  // first pixel of the step (uniform)
    b_okm = 0u;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const long k = k0 + a_row[i];
      const bool ok = k < a.Kpix && (m0 + a_cv[i] * 8) < a.Cout;
      const unsigned off = (unsigned)k * (unsigned)a.ldyb + a_colb0 + a_cv[i] * 16u;
      ra[i] = bload(rdy, ok ? off : kOOB);
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int ih = b_p[i] * a.stride + b_dh[i];
      const int iw = b_q[i] * a.stride + b_dw[i];
      const bool ok = (k0 + b_row[i]) < a.Kpix && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
      b_okm |= ok ? 1u << i : 0u;
      const unsigned pixi = (unsigned)((b_n[i] * a.H + ih) * a.W + iw);
      if (b_src[i] == 0)
        rbv[i] = bload(r1, ok ? pixi * (unsigned)a.ldc1b + b_cb[i] : kOOB);
      else
        rbv[i] = bload(r2, ok ? pixi * (unsigned)a.ldc2b + b_cb[i] : kOOB);
      // advance this row's pixel by one K step
      int q = b_q[i] + BKW, p = b_p[i], nb = b_n[i];
      while (q >= a.Q) {
        q -= a.Q;
        if (++p == a.P) {
          p = 0;
          ++nb;
        }
      }
      b_q[i] = q;
      b_p[i] = p;
      b_n[i] = nb;
    }
  };
  auto sstore = [&](int buf) {
    uint4* L = lds + buf * STAGE;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int row = a_row[i];
      const int sw = CPA >= 16 ? swz_tr16(row) : swz_tr8(row);
      L[row * CPA + (a_cv[i] ^ sw)] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int row = b_row[i];
      const int sw = CPB >= 16 ? swz_tr16(row) : swz_tr8(row);
      uint4 v = rbv[i];
      if constexpr (PRE) {  // == bn_apply: (bf16) relu(fmaf(z, sc, sh)); absent rows stay zero
        if ((b_okm >> i) & 1u) {
          bf16* e8 = reinterpret_cast<bf16*>(&v);
#pragma unroll
          for (int e = 0; e < 8; ++e) e8[e] = (bf16)fmaxf(fmaf((float)e8[e], pre_sc[i][e], pre_sh[i][e]), 0.f);
        }
      }
      L[BKW * CPA + row * CPB + (b_cv[i] ^ sw)] = v;
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt = (int)(kt1 - kt0);
  if (nkt > 0) {
    gload(kt0);
    sstore(0);
    __syncthreads();
  }
  const int g = lane >> 4, i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3;
  // per-lane byte offsets of every transposed fragment read (rows 8g+qq and +4 of the K step,
  // 16-B chunk of the fragment's columns under the row swizzle): the loop adds only the stage base
  unsigned toffA[FM][2], toffB[FN][2];
  {
    const int ra_ = 8 * g + qq, rb_ = ra_ + 4;
    auto off = [&](int cpr, int col0, int row) -> unsigned {
      const int chunk = (col0 >> 3) + (pp >> 1);
      const int sw = cpr >= 16 ? swz_tr16(row) : swz_tr8(row);
      return (unsigned)(row * (cpr * 16) + ((chunk ^ sw) * 16) + (pp & 1) * 8);
    };
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      toffA[i][0] = off(CPA, wm * WTM + i * 16, ra_);
      toffA[i][1] = off(CPA, wm * WTM + i * 16, rb_);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      toffB[j][0] = BKW * CPA * 16 + off(CPB, wn * WTN + j * 16, ra_);
      toffB[j][1] = BKW * CPA * 16 + off(CPB, wn * WTN + j * 16, rb_);
    }
  }
  static_assert(BKW == 32, "one 32-pixel K half per step");
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) gload(kt0 + kt + 1);
    const char* base = reinterpret_cast<const char*>(lds + cur * STAGE);
    auto trpair = [&](unsigned o0, unsigned o1) -> bf16x8 {
      s16x4 va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + o0));
      s16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + o1));
      typedef short s16x8 __attribute__((ext_vector_type(8)));
      s16x8 v = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
      return *reinterpret_cast<bf16x8*>(&v);
    };
    {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = trpair(toffA[i][0], toffA[i][1]);
#pragma unroll
      for (int j = 0; j < FN; ++j) bfr[j] = trpair(toffB[j][0], toffB[j][1]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(cur ^ 1);
    __syncthreads();
  }
  // partial slab ws[z][cout][tap*cin + c] (coalesced; wgrad_reduce permutes into PyTorch order)
  float* ws = a.ws + (long)blockIdx.z * a.Cout * a.Ng;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + wm * WTM + i * 16 + (lane >> 4) * 4 + e;
      if (m >= a.Cout) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * WTN + j * 16 + (lane & 15);
        if (n < a.Ng) ws[(long)m * a.Ng + n] = acc[i][j][e];
      }
    }
}

}  // namespace

bool wgrad_fast_ok(const FastWgradArgs& a) {
  return a.cin % 8 == 0 && a.c1 % 8 == 0 && a.Cout % 64 == 0;
}

int wgrad_fast_splits(int Cout, int Ng, long Kpix) {
  const int bm = Cout <= 64 ? 64 : 128;
  const int bn = Cout <= 64 ? 256 : 128;
  const int tiles = ceil_div(Cout, bm) * ceil_div(Ng, bn);
  const long nkt = (Kpix + kWgBK - 1) / kWgBK;
  // 256 target blocks since round 5 (replayed step: +0.1-0.2 % over 1024 / 512, smaller split-K slabs)
  int sp = ceil_div(256, tiles);
  const long max_sp = nkt / 32 > 0 ? nkt / 32 : 1;  // >= 32 K steps per split
  if (sp > max_sp) sp = (int)max_sp;
  if (sp > 512) sp = 512;
  if (sp < 1) sp = 1;
  return sp;
}

template <int BM, int BN, int NWM, int NWN, bool ROW32, bool PRE = false>
static void launch_wgrad_cfg(const FastWgradArgs& a, int splits, hipStream_t st) {
  const size_t lds = 2 * (size_t)kWgBK * (BM / 8 + BN / 8) * 16;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_fast_kernel<BM, BN, NWM, NWN, ROW32, PRE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr = true;
  }
  dim3 grid(ceil_div(a.Cout, BM), ceil_div(a.Ng, BN), splits);
  hipLaunchKernelGGL((wgrad_fast_kernel<BM, BN, NWM, NWN, ROW32, PRE>), grid, dim3(64 * NWM * NWN), lds, st, a);
}

// Which kernel of the fast family a call runs: the LDS-DMA ring where it applies (wgrad_ring_ok), else
// the register-staged 64x256 (<= 64 output channels) or 128x128 tile, each with or without ROW32.
// ROW32: every K step is one 32-pixel run of an output row, and the per-lane pixel deltas and
// scalar bases fit 32-bit offsets (the caller bounds both tensors below 2^31 bytes)
int wgrad_fast_kind(const FastWgradArgs& a) {
  const bool small = a.Cout <= 64;
  if (wgrad_ring_ok(a)) return small ? kWgRing64x256 : kWgRing128;
  const bool row32 = a.Q % kWgBK == 0;
  return small ? (row32 ? kWgFastRow64x256 : kWgFast64x256) : (row32 ? kWgFastRow128 : kWgFast128);
}

template <bool PRE>
static void launch_wgrad_kind(int kind, const FastWgradArgs& a, int splits, hipStream_t st) {
  switch (kind) {
    case kWgFastRow64x256: return launch_wgrad_cfg<64, 256, 1, 4, true, PRE>(a, splits, st);
    case kWgFast64x256: return launch_wgrad_cfg<64, 256, 1, 4, false, PRE>(a, splits, st);
    case kWgFastRow128: return launch_wgrad_cfg<128, 128, 2, 2, true, PRE>(a, splits, st);
    default: return launch_wgrad_cfg<128, 128, 2, 2, false, PRE>(a, splits, st);
  }
}

int launch_wgrad_fast(FastWgradArgs a, int splits, hipStream_t st) {
  const long nkt = (a.Kpix + kWgBK - 1) / kWgBK;
  a.kt_per_split = (int)((nkt + splits - 1) / splits);
  const int kind = wgrad_fast_kind(a);
  if (kind == kWgRing64x256 || kind == kWgRing128) return launch_wgrad_ring(a, splits, st);
  if (a.in_sc) launch_wgrad_kind<true>(kind, a, splits, st);
  else launch_wgrad_kind<false>(kind, a, splits, st);
  return 0;
}
