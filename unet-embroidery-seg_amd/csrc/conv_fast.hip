// Fast bf16 implicit-GEMM conv kernels for gfx950 (the hot configurations of the U-Net:
// every conv whose input channels are a multiple of 64).  See conv_generic.hip for the GEMM views.
//
// What makes them fast relative to the generic kernels in conv_generic.hip:
//  * operands are fetched with raw buffer loads (SRD + 32-bit voffset); a padding tap or an
//    out-of-range row gets an offset past num_records, so the hardware returns zeros: no
//    branches, no 64-bit address arithmetic in the K loop;
//  * the K loop walks (tap, 64-channel chunk) as wave-uniform scalar state: the tap offset, the
//    concat source (x1 | x2) and the weight offset are SGPR values; per row only a precomputed
//    tap-validity bitmask and a pixel index remain in VGPRs;
//  * TN: MFMA operand roles are swapped (weights = A, pixels = B) so each lane's accumulator
//    holds 4 consecutive output channels of one pixel -> 8-byte stores; 256x128 / 256x64 tiles.
// The persistent halo-A ring is conv_tn_persist.hip; the weight gradients are conv_wgrad_fast.hip and
// conv_wgrad_ring.hip.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "conv_fast.h"
#include "fast_util.h"


namespace {


// ------------------------------------------------------------------------------------------
// TN (fwd / dgrad).  Tile: BM pixels x BN output channels, K step 64 channels of one tap.
// ------------------------------------------------------------------------------------------
// How a tile moves its operands to LDS.  The register-staged kinds load into registers and store to
// LDS (so the input prologue can transform the values on the way); the ring DMAs straight into LDS.
enum class Pipe {
  OneStep,    // a single K step, one LDS stage
  Prefetch2,  // global loads two K steps ahead (two register sets; only where the registers fit at two
              // waves per SIMD), two LDS stages
  ShortK,     // short K (<= 4 steps) on one LDS stage, the next step's loads in registers
  Ring        // LDS-DMA ring of NS stages, NS - 1 K steps in flight
};

// One TN configuration: its code (conv_fast.h), tile BM x BN on NWM x NWN waves, pipeline and LDS
// stage count NS (Ring: ring depth; the weights' on a halo-A ring), the pieces HA the halo-A ring issues
// the next chunk's halo DMA in (0: not a halo-A ring; those are 3x3 only, TAPS == 9), and whether the
// tile has a post-3 (residual-BN backward) instantiation -- the tiles the bottleneck conv1 data gradients
// take (1x1, 1-8 K steps; on a ring only with one compile-time tap).
template <int CODE, int BM_, int BN_, int NWM_, int NWN_, Pipe PIPE_, int NS_, int HA_ = 0, bool POST3_ = false>
struct TnCfg {
  static constexpr int code = CODE, BM = BM_, BN = BN_, NWM = NWM_, NWN = NWN_, NS = NS_, HA = HA_;
  static constexpr Pipe PIPE = PIPE_;
  static constexpr bool POST3 = POST3_;
};
template <typename... Cs>
struct TnTable {};
// Measured: the 256x128 ring (3 stages) beats the register-staged 256x128 by 3-8 % on every
// large layer; the 64x128 ring (4 stages) is 15 % faster on deep-K small-M layers (3x3 at 16x16, 72 K
// steps) but slower on short K.  A halo-A ring serves a 3x3 stride-1 "same" conv whose output grid tiles
// into BM / 32 x 32 spatial blocks, in place of the gather ring of the same tile: 256x128 with the weights
// on 3 stages (144 KiB of LDS with the two halo stages) and the halo in three pieces at taps 0, 3, 6;
// 256x64 (<= 64 output channels: eight waves of 64x32, one weight row per wave and step); 128x128 (one or
// two tiles per CU: 4 x 32 spatial tiles, four waves, the weights on a 5-stage ring).
using Tn128x128 = TnCfg<kCfgTn128x128, 128, 128, 2, 2, Pipe::Prefetch2, 2>;  // these two also carry launch_tn_multi
using Tn64x128 = TnCfg<kCfgTn64x128, 64, 128, 1, 4, Pipe::Prefetch2, 2>;
using kTnTable = TnTable<TnCfg<kCfgTn256x128, 256, 128, 4, 2, Pipe::Prefetch2, 2>,
                         Tn128x128,
                         TnCfg<kCfgTn128x128Step1, 128, 128, 2, 2, Pipe::OneStep, 1, 0, true>,
                         Tn64x128,
                         TnCfg<kCfgTn128x64, 128, 64, 2, 2, Pipe::Prefetch2, 2>,
                         TnCfg<kCfgRing256x128, 256, 128, 4, 2, Pipe::Ring, 3, 0, true>,
                         TnCfg<kCfgRing64x128, 64, 128, 1, 4, Pipe::Ring, 4>,
                         TnCfg<kCfgRing128x128S5, 128, 128, 2, 2, Pipe::Ring, 5, 0, true>,
                         TnCfg<kCfgRing128x64, 128, 64, 2, 2, Pipe::Ring, 3>,
                         TnCfg<kCfgShort128x128, 128, 128, 2, 2, Pipe::ShortK, 1, 0, true>,
                         TnCfg<kCfgShort128x64, 128, 64, 2, 2, Pipe::ShortK, 1, 0, true>,
                         TnCfg<kCfgHaloA256x128, 256, 128, 4, 2, Pipe::Ring, 3, 3>,
                         TnCfg<kCfgHaloA256x64, 256, 64, 4, 2, Pipe::Ring, 3, 1>,
                         TnCfg<kCfgHaloA128x128, 128, 128, 2, 2, Pipe::Ring, 5, 1>>;

// f(record) for the record of kTnTable whose code equals the run-time `code`; false (and no call) when
// none does (as with_const in elem_util.h)
template <typename F, typename... Cs>
inline bool with_tn_cfg(int code, F&& f, TnTable<Cs...>) {
  return ((code == Cs::code ? (f(Cs{}), true) : false) || ...);
}
template <typename F>
inline bool with_tn_cfg(int code, F&& f) {
  return with_tn_cfg(code, f, kTnTable{});
}

// waves per SIMD each configuration is sized for (LDS allows that many blocks per CU); caps the
// register allocation so the two-step register prefetch cannot cost occupancy
// short K on one LDS stage: 128x128 at three waves per SIMD, 128x64 at four
template <int BM, int BN, int NWM, int NWN, Pipe PIPE = Pipe::Prefetch2>
constexpr int tn_waves_per_simd() {
  return PIPE == Pipe::ShortK ? (BN == 64 ? 4 : 3) : (BM == 64 || (BM == 128 && BN == 64)) ? 3 : 2;
}

// byte offset of the input-prologue coefficients in the TN kernel's dynamic LDS: after the operand
// stages (halo-A ring: two halo stages and NS weight stages) or the epilogue's transpose tiles + stats
// scratch, whichever is larger
template <int BM, int BN, int NWM, int NWN, int NS, int HA = 0>
constexpr size_t kPreOff() {
  constexpr size_t stages = HA ? ((size_t)2 * kHaloChunks<BM, NWM, NWN>() + (size_t)NS * BN * 8) * 16
                               : (size_t)NS * (BM + BN) * 8 * 16;
  constexpr size_t epi = (size_t)NWM * NWN * 64 * ((BN / NWN) * 2 + 16) + 3 * NWM * BN * 4;
  return ((stages > epi ? stages : epi) + 15) / 16 * 16;
}

// TAPS (LDS-DMA ring only): the filter has exactly TAPS = nr x ns taps, known at compile time.  The
// K loop is then unrolled over the taps and every (row, tap) gather offset is precomputed, so a K
// step issues its loads with one multiply-add per row and a scalar channel offset (the generic
// ring re-derives tap deltas, validity masks and offsets every step: ~70 VALU + ~90 SALU per step
// on the 256x128 tile, which is what held its MFMA pipe at ~45 % busy).
// PRE: the input prologue of FastTNArgs (x1 = BN input z, staged as relu(z*in_sc + in_sh) between the
// global load and the LDS store); the per-channel coefficients sit in LDS after the tile stages.
// The tile body: did = this block's linear id among gx * gy tiles (gy column tiles per row tile).
// HA (halo A operand, TAPS == 9 on the LDS-DMA ring; the value = pieces the next chunk's halo DMA is
// issued in, at taps 0, 9/HA, ..): see the K loop below.
template <int BM, int BN, int NWM, int NWN, Pipe PIPE, int NS, int POST, int TAPS, bool PRE, int HA = 0>
__device__ __forceinline__ void tn_fast_body(const FastTNArgs& a, const int did, const int gx, const int gy) {
  constexpr int NT = 64 * NWM * NWN;
  constexpr int WTM = BM / NWM, WTN = BN / NWN;
  constexpr int FP = WTM / 16, FC = WTN / 16;
  constexpr int RSTEP = NT / 8;
  constexpr int A_PER = BM / RSTEP, B_PER = BN / RSTEP;
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];  // [2 or NS][(BM+BN)*8]
  constexpr int STAGE = (BM + BN) * 8;
  constexpr bool kDMA = PIPE == Pipe::Ring;
  static_assert(!(PRE && kDMA), "the input prologue needs register staging");
  static_assert(NS == (PIPE == Pipe::Prefetch2 ? 2 : 1) || (kDMA && NS >= 3), "LDS stages of the pipeline");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / NWN, wn = wid % NWN;
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (dispatch id d -> XCD
  // d % 8), each with its own L2.  Give every XCD a contiguous range of tiles, N tiles fastest, so
  // the N tiles of one row tile and the neighbouring row tiles (the 3x3 taps re-read them) share
  // one L2.  Bijective for any tile count.
  const int ntiles = gx * gy;
  const int xq = ntiles >> 3, xr = ntiles & 7, xcd = did & 7;
  const int lin = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (did >> 3);
  const int tile_m = lin / gy, tile_n = lin - tile_m * gy;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kv = tid & 7, rb = tid >> 3;
  const int hw = a.hc * a.wc;
  // GEMM row -> linear pixel of the (hc, wc) grid.  On the halo-A ring (HA) a BM-row tile is a TR x 32
  // spatial block (TR = BM / 32) instead of BM consecutive pixels of one image row: the nine taps read
  // one (TR+2) x 34 halo.
  auto row_pix = [&](int m) -> int {
    if constexpr (!HA) {
      return m;
    } else {
      constexpr int TR = BM / 32;
      const int tpr = a.wc >> 5;
      const int t = m / BM, i = m - t * BM;
      const int rest = t / tpr, tw = t - rest * tpr;
      return (rest * TR + (i >> 5)) * a.wc + (tw << 5) + (i & 31);
    }
  };

  const __amdgpu_buffer_rsrc_t r1 = srd(a.x1, a.x1_bytes);
  const __amdgpu_buffer_rsrc_t r2 = srd(a.x2 ? a.x2 : a.x1, a.x2 ? a.x2_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rw = srd(a.wt, a.w_bytes);

  int pix[A_PER];
  unsigned vmask[A_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    const int m = m0 + rb + RSTEP * i;
    pix[i] = 0;
    vmask[i] = 0u;
    if (m < a.M) {
      const int pm = row_pix(m);
      const int nb = pm / hw, rem = pm - nb * hw;
      const int hh = rem / a.wc, ww = rem - hh * a.wc;
      const int ih0 = hh * a.istride, iw0 = ww * a.istride;
      pix[i] = (nb * a.H + ih0) * a.W + iw0;
      unsigned msk = 0u;
      for (int jr = 0; jr < a.nr; ++jr) {
        const int ih = ih0 + a.dh0 + a.dhs * jr;
        if (ih < 0 || ih >= a.H) continue;
        for (int js = 0; js < a.ns; ++js) {
          const int iw = iw0 + a.dw0 + a.dws * js;
          if (iw >= 0 && iw < a.W) msk |= 1u << (jr * a.ns + js);
        }
      }
      vmask[i] = msk;
    }
  }
  unsigned boff[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) {
    const int n = n0 + rb + RSTEP * i;
    // the LDS-DMA variant writes lane-linearly (slot = kv), so it fetches the chunk that slot holds
    // under the XOR swizzle instead: kv ^ ((row >> 1) & 7) (row parity is the same for every i)
    const int kvs = kDMA ? (kv ^ ((rb >> 1) & 7)) : kv;
    boff[i] = n < a.Ng ? (unsigned)n * (unsigned)a.ldwb + kvs * 16 : kOOB;
  }

  const int nch = a.cin >> 6;
  const int nsteps = a.nr * a.ns * nch;
  // two register sets: the loads of K step kt+2 are issued while step kt is computed and
  // step kt+1's registers are written to LDS, so each load has two steps of MFMA to land
  uint4 ra0[A_PER], rb0[B_PER], ra1[A_PER], rb1[B_PER];
  // scalar K-step state
  int s_jr = 0, s_js = 0, s_c = 0;
  // ---- LDS-DMA ring (Pipe::Ring, NS stages): buffer_load ... lds straight into the stage,
  // NS - 1 K steps in flight, counted vmcnt + raw barrier (no register staging) ----
  auto gload_dma = [&](int stage, bool live) {
    const int dh = a.dh0 + a.dhs * s_jr, dw = a.dw0 + a.dws * s_js;
    const int tapbit = (s_jr * a.ns + s_js) & 31;
    const int tapdelta = dh * a.W + dw;
    const unsigned wofs = (unsigned)(((a.r0 + a.rs * s_jr) * a.S + (a.s0 + a.ss * s_js)) * a.cin + s_c) * 2u;
    const unsigned sbase = lds_addr(lds) + (unsigned)(stage * STAGE * 16) + (unsigned)(wid * 8 * 128);
    const int kvs = kv ^ ((rb >> 1) & 7);
    const bool first = s_c < a.c1;
    const unsigned cb = (unsigned)(first ? s_c : s_c - a.c1) * 2u + kvs * 16;
    const unsigned ldcb = first ? (unsigned)a.ldc1b : (unsigned)a.ldc2b;
    const __amdgpu_buffer_rsrc_t rx = first ? r1 : r2;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const bool ok = live && ((vmask[i] >> tapbit) & 1u);
      const unsigned off = ok ? (unsigned)(pix[i] + tapdelta) * ldcb + cb : kOOB;
      dma16(rx, sbase + (unsigned)(RSTEP * i * 128), off);
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i)
      dma16(rw, sbase + (unsigned)((BM + RSTEP * i) * 128), (!live || boff[i] == kOOB) ? kOOB : boff[i] + wofs);
    if (++s_js == a.ns) {
      s_js = 0;
      if (++s_jr == a.nr) {
        s_jr = 0;
        s_c += 64;
      }
    }
  };
  // live == false (a K step past the end): every offset is out of range, so the loads return
  // zeros without touching memory.  Issuing them anyway keeps the loop free of conditional loads,
  // which lets hipcc count vmcnt exactly (with conditional loads it waits for the loads of the
  // step in flight too, exposing their latency every K step).
  auto gload = [&](uint4 (&ra)[A_PER], uint4 (&rbv)[B_PER], int& kc, bool live = true) {
    kc = s_c;  // channel base of this K step (input prologue)
    const int dh = a.dh0 + a.dhs * s_jr, dw = a.dw0 + a.dws * s_js;
    const int tapbit = (s_jr * a.ns + s_js) & 31;
    const int tapdelta = dh * a.W + dw;
    const unsigned wofs = (unsigned)(((a.r0 + a.rs * s_jr) * a.S + (a.s0 + a.ss * s_js)) * a.cin + s_c) * 2u;
    if (s_c < a.c1) {
      const unsigned cb = (unsigned)s_c * 2u + kv * 16;
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const bool ok = live && ((vmask[i] >> tapbit) & 1u);
        const unsigned off = (unsigned)(pix[i] + tapdelta) * (unsigned)a.ldc1b + cb;
        ra[i] = bload(r1, ok ? off : kOOB);
      }
    } else {
      const unsigned cb = (unsigned)(s_c - a.c1) * 2u + kv * 16;
#pragma unroll
      for (int i = 0; i < A_PER; ++i) {
        const bool ok = live && ((vmask[i] >> tapbit) & 1u);
        const unsigned off = (unsigned)(pix[i] + tapdelta) * (unsigned)a.ldc2b + cb;
        ra[i] = bload(r2, ok ? off : kOOB);
      }
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) rbv[i] = bload(rw, (!live || boff[i] == kOOB) ? kOOB : boff[i] + wofs);
    // K order: taps fastest, 64-channel chunks outer -- the nine taps of one chunk run back to
    // back over the same input footprint (L2-resident), instead of cycling through every chunk
    if (++s_js == a.ns) {
      s_js = 0;
      if (++s_jr == a.nr) {
        s_jr = 0;
        s_c += 64;
      }
    }
  };
  // input prologue coefficients: [2][cin] floats after the operand stages / epilogue scratch
  const float* pre_l = reinterpret_cast<const float*>(lds + kPreOff<BM, BN, NWM, NWN, NS>() / 16);
  if constexpr (PRE) {
    float* w = reinterpret_cast<float*>(lds + kPreOff<BM, BN, NWM, NWN, NS>() / 16);
    for (int c = tid; c < a.c1; c += NT) {
      w[c] = a.in_sc[c];
      w[a.c1 + c] = a.in_sh[c];
    }
    __syncthreads();
  }
  auto sstore = [&](int buf, const uint4 (&ra)[A_PER], const uint4 (&rbv)[B_PER], int kc) {
    uint4* L = lds + buf * STAGE;
    float psc[8], psh[8];
    if constexpr (PRE) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        psc[e] = pre_l[kc + kv * 8 + e];
        psh[e] = pre_l[a.c1 + kc + kv * 8 + e];
      }
    }
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int row = rb + RSTEP * i;
      uint4 v = ra[i];
      if constexpr (PRE) {  // == bn_apply: (bf16) relu(fmaf(z, sc, sh))
        v.x = bnrelu_pair(v.x, (f32x2){psc[0], psc[1]}, (f32x2){psh[0], psh[1]});
        v.y = bnrelu_pair(v.y, (f32x2){psc[2], psc[3]}, (f32x2){psh[2], psh[3]});
        v.z = bnrelu_pair(v.z, (f32x2){psc[4], psc[5]}, (f32x2){psh[4], psh[5]});
        v.w = bnrelu_pair(v.w, (f32x2){psc[6], psc[7]}, (f32x2){psh[6], psh[7]});
      }
      L[row * 8 + swz8(row, kv)] = v;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int row = rb + RSTEP * i;
      L[(BM + row) * 8 + swz8(row, kv)] = rbv[i];
    }
  };

  f32x4 acc[FC][FP];
#pragma unroll
  for (int c = 0; c < FC; ++c)
#pragma unroll
    for (int p = 0; p < FP; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Fragment reads: row = base + p*16 + (lane & 15) and the swizzle depends on (row >> 1) & 7, i.e.
  // on the lane alone, so each (operand, K half) has one per-lane byte offset and the p / c steps are
  // immediates (p * 16 rows * 128 B); per step only the stage base is added.
  unsigned foffA[2], foffB[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int r = lane & 15, sw = ((kk * 4 + (lane >> 4)) ^ ((r >> 1) & 7)) * 16;
    foffA[kk] = (unsigned)((wm * WTM + r) * 128 + sw);
    foffB[kk] = (unsigned)((BM + wn * WTN + r) * 128 + sw);
  }
  auto frags = [&](int buf, int kk, bf16x8 (&pf)[FP], bf16x8 (&wf)[FC]) {
    const char* sb = reinterpret_cast<const char*>(lds + buf * STAGE);
    const char* pa = sb + foffA[kk];
    const char* pb = sb + foffB[kk];
#pragma unroll
    for (int p = 0; p < FP; ++p) pf[p] = *reinterpret_cast<const bf16x8*>(pa + p * 2048);
#pragma unroll
    for (int c = 0; c < FC; ++c) wf[c] = *reinterpret_cast<const bf16x8*>(pb + c * 2048);
  };
  auto mfmas = [&](const bf16x8 (&pf)[FP], const bf16x8 (&wf)[FC]) {
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int p = 0; p < FP; ++p)
        acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], pf[p], acc[c][p], 0, 0, 0);
  };
  auto compute = [&](int buf) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 pf[FP], wf[FC];
      frags(buf, kk, pf, wf);
      mfmas(pf, wf);
    }
  };

  if constexpr (HA) {
    // ---- halo-A ring: 3x3 stride-1 "same" convolutions whose BM-row tile is a TRH x 32 spatial
    // block (row_pix).  Per 64-channel chunk the (TRH+2) x 34 halo of the tile is LDS-DMA'd
    // ONCE (double buffered, the next chunk's halo in flight during this chunk's nine taps) and the
    // nine taps read their A fragments from it at a uniform pixel shift; only the weights stream
    // through the NS-stage ring, one tap per K step.  Per chunk that is ~43 KiB of A DMA instead of
    // 9 x 32 KiB of re-gathered tap rows: 2.3x fewer DMA instructions per MFMA than the gather ring.
    static_assert(TAPS == 9 && kDMA && !PRE && (B_PER % 2 == 0 || B_PER == 1), "halo-A ring: 3x3 taps");
    constexpr int TRH = BM / 32;
    constexpr int HPIX = (TRH + 2) * 34;
    constexpr int HST = kHaloChunks<BM, NWM, NWN>();  // 16-B chunks per halo stage (padded)
    constexpr int HI = HST / NT;                       // halo DMA instructions per wave (every wave)
    constexpr int WST = BN * 8;                        // 16-B chunks per weight stage
    constexpr int WP = B_PER;                          // weight DMA instructions per wave per K step
    static_assert(HI % 2 == 0, "halo rows are issued in pairs");
    static_assert(WP * (NS - 2) + HI <= 63, "vmcnt range");
    // the next chunk's halo goes out in HA pieces (HI / HA DMA instructions each) at taps 0, 9 / HA, ..
    constexpr int HPC = HI / HA, TPER = 9 / HA;
    static_assert(HI % (2 * HA) == 0 && 9 % HA == 0, "halo pieces of whole instruction pairs");
    // this block's spatial tile (row_pix: tiles of TRH image rows x 32 columns,
    // stacked over the images; hc % TRH == 0, so a tile never straddles two images)
    const int tpr = a.wc >> 5;
    const int tt = m0 / BM;
    const int rest = tt / tpr, twi = tt - rest * tpr;
    const int hg = rest * TRH;  // first row of the tile in the stacked (N * hc) row space
    const int nb = hg / a.hc, h0 = hg - nb * a.hc, w0 = twi * 32;
    const unsigned pb1 = a.x1_bytes / (unsigned)a.ldc1b;
    const unsigned pb2 = a.x2 ? a.x2_bytes / (unsigned)a.ldc2b : 0u;
    const unsigned pbad = (pb1 > pb2 ? pb1 : pb2) + 1u;
    // this lane's halo DMA slots: source pixel (or pbad: outside the image / past the halo) and the
    // swizzled source chunk; LDS slot (hp, lane & 7) holds chunk (lane & 7) ^ (hp & 7)
    unsigned hvp[HI], hsw[HI];
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      const int idx = (i * (NWM * NWN) + wid) * 64 + lane;
      const int hp = idx >> 3;
      const int hr = hp / 34, hcol = hp - hr * 34;
      const int h = h0 - 1 + hr, w = w0 - 1 + hcol;
      const bool ok = hp < HPIX && h >= 0 && h < a.H && w >= 0 && w < a.W;
      hvp[i] = ok ? (unsigned)((nb * a.H + h) * a.W + w) : pbad;
      hsw[i] = (unsigned)(((lane & 7) ^ (hp & 7)) * 16);
    }
    unsigned tw[9];  // weight byte offset of each tap
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int jr = t / 3, js = t - jr * 3;
      tw[t] = (unsigned)(((a.r0 + a.rs * jr) * a.S + (a.s0 + a.ss * js)) * a.cin) * 2u;
    }
    // A fragment p of this lane: tile pixel (row wm * WTM / 32 + p / 2, column (p & 1) * 16 + lane % 16)
    // -> halo pixel at the centre tap; a tap adds the uniform shift dh * 34 + dw
    static_assert(WTM == 64 && FP == 4, "64-row wave tiles: two image rows of 32 pixels");
    int hq[FP];
#pragma unroll
    for (int p = 0; p < FP; ++p) hq[p] = (wm * 2 + (p >> 1) + 1) * 34 + (p & 1) * 16 + (lane & 15) + 1;
    const int chA = lane >> 4;  // 16-B chunk of the first K half (the second is chA ^ 4)
    unsigned foffW[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int r = lane & 15;
      foffW[kk] = (unsigned)((wn * WTN + r) * 128 + ((kk * 4 + (lane >> 4)) ^ ((r >> 1) & 7)) * 16);
    }
    const unsigned hbase = lds_addr(lds);
    const unsigned wbase = hbase + 2u * HST * 16u;
    const int nch = a.cin >> 6;
    auto issue_halo = [&](int c, int hs, int i0, int i1) {
      const bool live = c < nch;
      const int c64 = c * 64;
      const bool first = c64 < a.c1;
      const __amdgpu_buffer_rsrc_t rx = srd_u(first ? a.x1 : a.x2, !live ? 0u : first ? a.x1_bytes : a.x2_bytes);
      const unsigned ldcb = first ? (unsigned)a.ldc1b : (unsigned)a.ldc2b;
      const unsigned soff = __builtin_amdgcn_readfirstlane(live ? (unsigned)(first ? c64 : c64 - a.c1) * 2u : 0u);
      const unsigned sb = __builtin_amdgcn_readfirstlane(hbase + (unsigned)(hs * HST * 16) + (unsigned)(wid * 1024));
#pragma unroll
      for (int i = i0; i < i1; i += 2)
        dma16x2<NT * 16>(rx, sb + (unsigned)(i * NT * 16), __umul24(hvp[i], ldcb) + hsw[i],
                         __umul24(hvp[i + 1], ldcb) + hsw[i + 1], soff);
    };
    auto issue_w = [&](int c, int t, int stage) {
      const bool live = c < nch;
      const __amdgpu_buffer_rsrc_t rwx = srd_u(a.wt, live ? a.w_bytes : 0u);
      const unsigned wsoff = __builtin_amdgcn_readfirstlane(live ? tw[t] + (unsigned)(c * 64) * 2u : 0u);
      const unsigned sb = __builtin_amdgcn_readfirstlane(wbase + (unsigned)(stage * WST * 16) + (unsigned)(wid * 8 * 128));
      if constexpr (B_PER == 1) {
        dma16s(rwx, sb, boff[0], wsoff);
      } else {
#pragma unroll
        for (int i = 0; i < B_PER; i += 2)
          dma16x2<RSTEP * 128>(rwx, sb + (unsigned)(RSTEP * i * 128), boff[i], boff[i + 1], wsoff);
      }
    };
    // wait for this step's weight stage (and, at a chunk's first tap, its halo): the younger DMAs
    // still in flight are the NS-2 later weight steps plus the next chunk's halo when it was issued
    // after this step's weights (taps 1 .. NS-1 of a chunk)
    auto wait_step = [&](auto tc) {
      constexpr int t = decltype(tc)::value;
      // halo pieces issued in the NS-1 iterations since this step's weights went out (those
      // iterations' taps t-1 .. t-NS+1, mod 9)
      constexpr int n = WP * (NS - 2) + HPC * (((((t - 1) % 9 + 9) % 9) % TPER == 0 ? 1 : 0) +
                                               (NS >= 3 && ((((t - 2) % 9 + 9) % 9) % TPER == 0) ? 1 : 0) +
                                               (NS >= 4 && ((((t - 3) % 9 + 9) % 9) % TPER == 0) ? 1 : 0) +
                                               (NS >= 5 && ((((t - 4) % 9 + 9) % 9) % TPER == 0) ? 1 : 0));
      static_assert(NS <= 5, "wait count");
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(n) : "memory");
    };
    issue_halo(0, 0, 0, HI);
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0) issue_w(s0 / 9, s0 % 9, s0);
    int stage = 0;
    for (int c = 0; c < nch; ++c) {
      const char* hs = reinterpret_cast<const char*>(lds) + (c & 1) * HST * 16;
      auto step = [&](auto tc) {
        constexpr int t = decltype(tc)::value;
        wait_step(tc);
        const int jr = t / 3, js = t - jr * 3;
        const int shift = (a.dh0 + a.dhs * jr) * 34 + (a.dw0 + a.dws * js);
        unsigned ab[FP];
#pragma unroll
        for (int p = 0; p < FP; ++p) {
          const int hp = hq[p] + shift;
          ab[p] = (unsigned)(hp * 128 + ((chA ^ (hp & 7)) * 16));
        }
        const char* ws = reinterpret_cast<const char*>(lds) + 2 * HST * 16 + stage * WST * 16;
        bf16x8 pf[FP], wf[FC];
#pragma unroll
        for (int p = 0; p < FP; ++p) pf[p] = *reinterpret_cast<const bf16x8*>(hs + ab[p]);
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) wf[cc] = *reinterpret_cast<const bf16x8*>(ws + foffW[0] + cc * 2048);
        const int st2 = stage == 0 ? NS - 1 : stage - 1;  // (stage + NS - 1) % NS
        issue_w(c + (t + NS - 1) / 9, (t + NS - 1) % 9, st2);
        if constexpr (t % TPER == 0) issue_halo(c + 1, (c + 1) & 1, (t / TPER) * HPC, (t / TPER + 1) * HPC);
        mfmas(pf, wf);
#pragma unroll
        for (int p = 0; p < FP; ++p) pf[p] = *reinterpret_cast<const bf16x8*>(hs + (ab[p] ^ 64u));
#pragma unroll
        for (int cc = 0; cc < FC; ++cc) wf[cc] = *reinterpret_cast<const bf16x8*>(ws + foffW[1] + cc * 2048);
        mfmas(pf, wf);
        stage = stage == NS - 1 ? 0 : stage + 1;
      };
      step(std::integral_constant<int, 0>{});
      step(std::integral_constant<int, 1>{});
      step(std::integral_constant<int, 2>{});
      step(std::integral_constant<int, 3>{});
      step(std::integral_constant<int, 4>{});
      step(std::integral_constant<int, 5>{});
      step(std::integral_constant<int, 6>{});
      step(std::integral_constant<int, 7>{});
      step(std::integral_constant<int, 8>{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  } else if constexpr (kDMA && TAPS > 0) {
    constexpr int PER = A_PER + B_PER;
    static_assert(NS >= 3 && PER * (NS - 2) <= 63, "vmcnt range");
    static_assert(A_PER % 2 == 0 && (B_PER % 2 == 0 || B_PER == 1), "rows are issued in pairs");
    // (row, tap) -> gather pixel, or pbad: one past every source's last pixel, so pbad * ldcb is
    // out of range for either source (the launcher checks it cannot wrap 32 bits)
    const unsigned pb1 = a.x1_bytes / (unsigned)a.ldc1b;
    const unsigned pb2 = a.x2 ? a.x2_bytes / (unsigned)a.ldc2b : 0u;
    const unsigned pbad = (pb1 > pb2 ? pb1 : pb2) + 1u;
    unsigned vpix[A_PER][TAPS];
    unsigned tw[TAPS];  // weight byte offset of each tap
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int jr = t / a.ns, js = t - jr * a.ns;
      const int tapdelta = (a.dh0 + a.dhs * jr) * a.W + a.dw0 + a.dws * js;
      tw[t] = (unsigned)(((a.r0 + a.rs * jr) * a.S + (a.s0 + a.ss * js)) * a.cin) * 2u;
#pragma unroll
      for (int i = 0; i < A_PER; ++i) vpix[i][t] = ((vmask[i] >> t) & 1u) ? (unsigned)(pix[i] + tapdelta) : pbad;
    }
    const unsigned kv16 = (unsigned)(kv ^ ((rb >> 1) & 7)) * 16u;
    const unsigned lbase = lds_addr(lds) + (unsigned)(wid * 8 * 128);
    const int nch = a.cin >> 6;
    // issue K step (chunk c, tap t) into stage `stage`; a chunk past the end loads through
    // zero-extent descriptors (zeros, no memory traffic) so every step issues PER loads
    auto issue = [&](int c, int t, int stage) {
      const bool live = c < nch;
      const int c64 = c * 64;
      const bool first = c64 < a.c1;
      // wave-uniform by construction; readfirstlane keeps them in SGPRs for the asm operands
      const __amdgpu_buffer_rsrc_t rx = srd_u(first ? a.x1 : a.x2, !live ? 0u : first ? a.x1_bytes : a.x2_bytes);
      const __amdgpu_buffer_rsrc_t rwx = srd_u(a.wt, live ? a.w_bytes : 0u);
      const unsigned ldcb = first ? (unsigned)a.ldc1b : (unsigned)a.ldc2b;
      const unsigned soff = __builtin_amdgcn_readfirstlane(live ? (unsigned)(first ? c64 : c64 - a.c1) * 2u : 0u);
      const unsigned wsoff = __builtin_amdgcn_readfirstlane(live ? tw[t] + (unsigned)c64 * 2u : 0u);
      const unsigned sb = __builtin_amdgcn_readfirstlane(lbase + (unsigned)(stage * STAGE * 16));
#pragma unroll
      for (int i = 0; i < A_PER; i += 2)
        dma16x2<RSTEP * 128>(rx, sb + (unsigned)(RSTEP * i * 128), __umul24(vpix[i][t], ldcb) + kv16,
                             __umul24(vpix[i + 1][t], ldcb) + kv16, soff);
      if constexpr (B_PER == 1) {
        dma16s(rwx, sb + (unsigned)(BM * 128), boff[0], wsoff);
      } else {
#pragma unroll
        for (int i = 0; i < B_PER; i += 2)
          dma16x2<RSTEP * 128>(rwx, sb + (unsigned)((BM + RSTEP * i) * 128), boff[i], boff[i + 1], wsoff);
      }
    };
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0) issue(s0 / TAPS, s0 % TAPS, s0);
    int stage = 0;
    // DMA issue costs the issuing wave tens of cycles per instruction; right after the barrier every
    // wave would issue at once and leave the MFMA pipes idle.  The waves sharing a SIMD (w and w + 4
    // of 8) split: one issues before its first K half, the other after it.
    const bool late = NWM * NWN == 8 && ((wid >> 2) & 1);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(PER * (NS - 2)) : "memory");
        bf16x8 pf[FP], wf[FC];
        frags(stage, 0, pf, wf);  // first fragments in flight while this step's loads issue
        const int st2 = stage == 0 ? NS - 1 : stage - 1;  // (stage + NS - 1) % NS
        if (!late) issue(c + (t + NS - 1) / TAPS, (t + NS - 1) % TAPS, st2);
        mfmas(pf, wf);
        frags(stage, 1, pf, wf);
        if (late) issue(c + (t + NS - 1) / TAPS, (t + NS - 1) % TAPS, st2);
        mfmas(pf, wf);
        stage = stage == NS - 1 ? 0 : stage + 1;
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  } else if constexpr (kDMA) {
    constexpr int PER = A_PER + B_PER;
    static_assert(NS >= 3 && PER * (NS - 2) <= 63, "vmcnt range");
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0) gload_dma(s0, s0 < nsteps);
    for (int kt = 0; kt < nsteps; ++kt) {
      // this wave's DMAs of step kt have landed (the NS-2 younger steps stay in flight), this
      // wave's LDS reads of step kt-1 are done; the barrier makes both true for every wave
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(PER * (NS - 2)) : "memory");
      gload_dma((kt + NS - 1) % NS, kt + NS - 1 < nsteps);  // refills the stage read at kt-1
      compute(kt % NS);
    }
    // every DMA (past-the-end ones write zeros) has landed before the epilogue reuses the LDS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  } else if (PIPE == Pipe::OneStep) {  // one K step
    int kc0 = 0;
    if (nsteps > 0) {
      gload(ra0, rb0, kc0);
      sstore(0, ra0, rb0, kc0);
      __syncthreads();
      compute(0);
    }
    __syncthreads();
  } else if (PIPE == Pipe::ShortK) {
    // short K (<= 4 steps) on ONE LDS stage: the next step's loads are in registers while this step
    // computes; two barriers per step.  The single stage (32 / 24 KiB) and the one register set let
    // 3-4 blocks share a CU, which is what hides the HBM latency of these memory-bound layers.
    int kc0 = 0;
    if (nsteps > 0) {
      gload(ra0, rb0, kc0);
      sstore(0, ra0, rb0, kc0);
      __syncthreads();
    }
    for (int kt = 0; kt < nsteps; ++kt) {
      const bool more = kt + 1 < nsteps;
      if (more) gload(ra0, rb0, kc0);
      compute(0);
      __syncthreads();
      if (more) {
        sstore(0, ra0, rb0, kc0);
        __syncthreads();
      }
    }
  } else {  // Pipe::Prefetch2: loads two steps ahead (two register sets)
    // Loads and LDS stores are unconditional inside the loop (past-the-end steps load zeros), so
    // the in-order vmcnt bookkeeping is the same on every path: each sstore waits only for the
    // register set it writes, while the set issued in the same half stays in flight.
    int kc0 = 0, kc1 = 0;
    if (nsteps > 0) {
      gload(ra0, rb0, kc0);
      sstore(0, ra0, rb0, kc0);
      gload(ra1, rb1, kc1, nsteps > 1);
      __syncthreads();
    }
    for (int kt = 0; kt < nsteps; kt += 2) {
      // even step: stage 0 holds kt, registers 1 hold kt+1 (in flight)
      gload(ra0, rb0, kc0, kt + 2 < nsteps);
      compute(0);
      sstore(1, ra1, rb1, kc1);
      __syncthreads();
      if (kt + 1 >= nsteps) break;
      // odd step: stage 1 holds kt+1, registers 0 hold kt+2 (in flight)
      gload(ra1, rb1, kc1, kt + 3 < nsteps);
      compute(1);
      sstore(0, ra0, rb0, kc0);
      __syncthreads();
    }
  }

  // ---- epilogue: lane holds D[cout = (lane>>4)*4 + e][pixel = lane&15] per (c, p) subtile ----
  // bias + ReLU + bf16 rounding in registers; per-wave BN partials (sum, M2 about the wave's
  // mean) by shuffles; each wave transposes its WTM x WTN tile through LDS (the operand stages are
  // free after the K loop's last barrier) and writes whole 16-B chunks of each pixel's channel
  // run; finally one barrier and a Chan merge of the row-waves' partials per output channel.
  static_assert(WTM == 64, "64 rows per wave");
  const int kg = lane >> 4, j16 = lane & 15;
  const int row0 = m0 + wm * WTM;
  const int cnt = min(WTM, a.M - row0);
  constexpr int LROW = WTN * 2 + 16;  // bytes per LDS row (padded: conflict-free 8-B writes)
  char* tl = reinterpret_cast<char*>(lds) + wid * (WTM * LROW);
  // per-wave (sum, M2) of the stats / post-op partials, after every wave's transpose tile: [2 or 3][NWM][BN]
  float* red = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + NWM * NWN * WTM * LROW);

  float csum[FC][4];
#pragma unroll
  for (int c = 0; c < FC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[c][e] = 0.f;
  float bias[FC][4];
#pragma unroll
  for (int c = 0; c < FC; ++c) {
    const int nb = n0 + wn * WTN + c * 16 + kg * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[c][e] = (a.bias && nb + e < a.Ng) ? a.bias[nb + e] : 0.f;
  }
  auto out_pix = [&](int m0_) -> long {
    const int m = row_pix(m0_);
    if (a.ostride == 1 && a.ph == 0 && a.pw == 0 && a.OW == a.wc && a.OH == a.hc) return m;
    const int nb = m / hw, rem = m - nb * hw;
    const int hh = rem / a.wc, ww = rem - hh * a.wc;
    return ((long)nb * a.OH + hh * a.ostride + a.ph) * a.OW + ww * a.ostride + a.pw;
  };
  // post-op aux values, loaded first so their latency overlaps the rounding pass
  uint2 zr[FC][FP];
  if (POST == 1) {
#pragma unroll
    for (int c = 0; c < FC; ++c) {
      const int nb = n0 + wn * WTN + c * 16 + kg * 4;
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        const bool ok = nb < a.Ng && p * 16 + j16 < cnt;
        zr[c][p] = ok ? *reinterpret_cast<const uint2*>((const bf16*)a.aux + out_pix(row0 + p * 16 + j16) * a.ld_aux + nb)
                      : uint2{0u, 0u};
      }
    }
  }
#pragma unroll
  for (int p = 0; p < FP; ++p) {
    const bool mok = p * 16 + j16 < cnt;
#pragma unroll
    for (int c = 0; c < FC; ++c) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[c][p][e] + bias[c][e];
        if (a.relu) v = fmaxf(v, 0.f);
        acc[c][p][e] = mok ? (float)(bf16)v : 0.f;  // BN statistics are of the stored (rounded) values
        csum[c][e] += acc[c][p][e];
      }
    }
  }
  if (POST == 1) {
    // mask the rounded gradient with the producer's ReLU (recomputed from aux) and reduce its
    // backward partials over the wave's rows: q0 = sum d, q1 = sum d * xhat (BN) (one reduction chain
    // pair at a time: row16_sum_n over a channel group's 8 spills in the 5-stage 128x128 tile)
#pragma unroll
    for (int c = 0; c < FC; ++c) {
      const int nb = n0 + wn * WTN + c * 16 + kg * 4;
      const bool nok = nb < a.Ng;
      float sc4[4], sh4[4], mu4[4], iv4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool bn = a.post == 2 && nok;
        sc4[e] = bn ? a.psc[nb + e] : 0.f;
        sh4[e] = bn ? a.psh[nb + e] : 0.f;
        mu4[e] = bn ? a.pmean[nb + e] : 0.f;
        iv4[e] = bn ? a.pinv[nb + e] : 0.f;
      }
      float q0[4] = {0.f, 0.f, 0.f, 0.f}, q1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        const bf16* z = reinterpret_cast<const bf16*>(&zr[c][p]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float zf = (float)z[e];
          const bool on = a.post == 2 ? fmaf(zf, sc4[e], sh4[e]) > 0.f : zf > 0.f;
          const float d = on ? acc[c][p][e] : 0.f;
          acc[c][p][e] = d;
          q0[e] += d;
          q1[e] += d * ((zf - mu4[e]) * iv4[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t0 = row16_sum(q0[e]), t1 = row16_sum(q1[e]);
        if (j16 == 0) {
          const int col = wn * WTN + c * 16 + kg * 4 + e;
          red[wm * BN + col] = t0;
          red[(NWM + wm) * BN + col] = t1;
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < FP; ++p)
#pragma unroll
    for (int c = 0; c < FC; ++c) {
      bf16 ob[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ob[e] = (bf16)acc[c][p][e];  // exact: acc holds rounded values
      *reinterpret_cast<uint2*>(tl + (p * 16 + j16) * LROW + (c * 16 + kg * 4) * 2) = *reinterpret_cast<uint2*>(ob);
    }
  if (a.stats) {
    // (sum, M2 about the wave mean) of each of the lane's FC * 4 channels over the wave's rows; the
    // row reductions run together (row16_sum_n)
    float sv[FC * 4], qv[FC * 4];
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) sv[c * 4 + e] = csum[c][e];
    row16_sum_n(sv);
    const float inv_cnt = 1.0f / (float)max(cnt, 1);
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mean = sv[c * 4 + e] * inv_cnt;
        float q = 0.f;
#pragma unroll
        for (int p = 0; p < FP; ++p)
          if (p * 16 + j16 < cnt) {
            const float d = acc[c][p][e] - mean;
            q += d * d;
          }
        qv[c * 4 + e] = q;
      }
    row16_sum_n(qv);
    if (j16 == 0)
#pragma unroll
      for (int c = 0; c < FC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = wn * WTN + c * 16 + kg * 4 + e;
          red[wm * BN + col] = sv[c * 4 + e];
          red[(NWM + wm) * BN + col] = qv[c * 4 + e];
        }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS tile is written
  __builtin_amdgcn_wave_barrier();
  // coalesced write-out: lane -> (pixel row r = i*(64/CPR) + lane/CPR, 16-B chunk lane%CPR)
  constexpr int CPR = WTN / 8;          // 16-B chunks per pixel row of the wave tile
  constexpr int RPI = 64 / CPR;         // rows per store instruction
  const int ck = lane % CPR, rsub = lane / CPR;
  const int nc = n0 + wn * WTN + ck * 8;
  // post 3 (residual-BN backward) on the transposed tile, 8 channels x this lane's rows: d = mask *
  // bf16(dgrad + the residual gradient already in y); q0 = sum d, q1 = sum d * xhat1 [, q2 = .. xhat2]
  constexpr int NQ3 = POST == 3 ? 8 : 1;
  float q3[3][NQ3], mu3[2][NQ3], iv3[2][NQ3];
  const bool two = POST == 3 && a.aux2 != nullptr;
  if constexpr (POST == 3) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = nc + e < a.Ng;
      q3[0][e] = q3[1][e] = q3[2][e] = 0.f;
      mu3[0][e] = ok ? a.pmean[nc + e] : 0.f;
      iv3[0][e] = ok ? a.pinv[nc + e] : 0.f;
      mu3[1][e] = (ok && two) ? a.pmean2[nc + e] : 0.f;
      iv3[1][e] = (ok && two) ? a.pinv2[nc + e] : 0.f;
    }
  }
  // the write-out's global reads (the old gradient; post 3: y3 / y_ds and the mask byte) of GRP rows
  // are issued together before their stores: the stores may alias them as far as the compiler knows,
  // so loads left inside the row loop would each wait out a full memory round trip (vmcnt also counts
  // the preceding stores) -- eight serial HBM latencies per tile in these short-K layers.  Post 3 in
  // groups of four rows (its 13 registers per row beside the partials and coefficients would spill).
  constexpr int NIT = WTM / RPI;
  constexpr int GRP = (POST == 3 && NIT > 4) ? 4 : NIT;
  static_assert(NIT % GRP == 0, "row groups");
#pragma unroll
  for (int g0 = 0; g0 < NIT; g0 += GRP) {
    uint4 oldv[GRP], zv[POST == 3 ? GRP : 1], z2v[POST == 3 ? GRP : 1];
    unsigned mkv[POST == 3 ? GRP : 1];
    if (POST == 3 || a.accumulate) {
      // every load unconditional, at a valid address for the lanes whose row / chunk is absent (this
      // wave's first row, or the last row M - 1 when the wave has none -- the last tile's second
      // row-wave can start past M; the last chunk; their values are never used): a load under the lane
      // condition had its value moved across the branch and was waited on by itself -- GRP serial
      // round trips
      const bf16* aux2p = two ? (const bf16*)a.aux2 : (const bf16*)a.aux;
      const long ld2 = two ? a.ld_aux2 : a.ld_aux;
      const int ncl = nc < a.Ng ? nc : a.Ng - 8;
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        const int r = (g0 + j) * RPI + rsub;
        const long opx = out_pix(r < cnt ? row0 + r : min(row0, a.M - 1));
        oldv[j] = *reinterpret_cast<const uint4*>((const bf16*)a.y + opx * a.ldy + ncl);
        if constexpr (POST == 3) {
          zv[j] = *reinterpret_cast<const uint4*>((const bf16*)a.aux + opx * a.ld_aux + ncl);
          z2v[j] = *reinterpret_cast<const uint4*>(aux2p + opx * ld2 + ncl);
          mkv[j] = (unsigned)a.mbits[opx * (a.Ng >> 3) + (ncl >> 3)];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GRP; ++j) {
      const int r = (g0 + j) * RPI + rsub;
      if (r >= cnt || nc >= a.Ng) continue;
      const long opx = out_pix(row0 + r);
      bf16* ptr = (bf16*)a.y + opx * a.ldy + nc;
      uint4 v = *reinterpret_cast<const uint4*>(tl + r * LROW + ck * 16);
      if constexpr (POST == 3) {
        const uint4 old = oldv[j], z = zv[j], z2 = z2v[j];
        const unsigned mk = mkv[j];
        const bf16* ob = reinterpret_cast<const bf16*>(&old);
        const bf16* zb = reinterpret_cast<const bf16*>(&z);
        const bf16* z2b = reinterpret_cast<const bf16*>(&z2);
        bf16* nv = reinterpret_cast<bf16*>(&v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bf16 sm = (bf16)((float)nv[e] + (float)ob[e]);  // == the accumulating store
          const float d = ((mk >> e) & 1u) ? (float)sm : 0.f;
          nv[e] = (bf16)d;
          q3[0][e] += d;
          q3[1][e] = fmaf(d, ((float)zb[e] - mu3[0][e]) * iv3[0][e], q3[1][e]);
          if (two) q3[2][e] = fmaf(d, ((float)z2b[e] - mu3[1][e]) * iv3[1][e], q3[2][e]);
        }
      } else if (a.accumulate) {  // dx += dgrad (two bf16 tensors summed in fp32, like autograd's accumulation)
        const uint4 old = oldv[j];
        const bf16* ob = reinterpret_cast<const bf16*>(&old);
        bf16* nv = reinterpret_cast<bf16*>(&v);
#pragma unroll
        for (int e = 0; e < 8; ++e) nv[e] = (bf16)((float)nv[e] + (float)ob[e]);
      }
      *reinterpret_cast<uint4*>(ptr) = v;
    }
  }
  if constexpr (POST == 3) {
    // sum over the lanes of this chunk column (same ck), then one lane per chunk writes the wave's
    // partials of its 8 channels to red[q][NWM][BN]
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        for (int o = CPR; o < 64; o <<= 1) q3[q][e] += __shfl_xor(q3[q][e], o, 64);
    if (rsub == 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = wn * WTN + ck * 8 + e;
        red[wm * BN + col] = q3[0][e];
        red[(NWM + wm) * BN + col] = q3[1][e];
        red[(2 * NWM + wm) * BN + col] = q3[2][e];
      }
    }
  }
  if (POST) {
    // plain sums of the NWM row-waves' partials -> ppart[tile_m][nq][Ng] (nq = 3 with a second
    // residual branch, else 2)
    const int nq = (POST == 3 && a.aux2) ? 3 : 2;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int col = tid; col < BN; col += NT) {
      const int n = n0 + col;
      if (n >= a.Ng) continue;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int w = 0; w < NWM; ++w) {
        t0 += red[w * BN + col];
        t1 += red[(NWM + w) * BN + col];
        if (POST == 3) t2 += red[(2 * NWM + w) * BN + col];
      }
      a.ppart[(long)tile_m * nq * a.Ng + n] = t0;
      a.ppart[(long)tile_m * nq * a.Ng + a.Ng + n] = t1;
      if (nq == 3) a.ppart[(long)tile_m * nq * a.Ng + 2 * a.Ng + n] = t2;
    }
  }
  if (a.stats) {
    // Chan merge of the NWM row-wave partials -> one (sum, M2) per block row tile (BM rows),
    // written contiguously: stats[tile_m][2][Ng].  Raw barrier: LDS visibility only -- a
    // __syncthreads() would also wait for this block's output stores to retire.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int col = tid; col < BN; col += NT) {
      const int n = n0 + col;
      if (n >= a.Ng) continue;
      float st = 0.f, nt = 0.f;
#pragma unroll
      for (int w = 0; w < NWM; ++w) {
        st += red[w * BN + col];
        nt += (float)max(0, min(WTM, a.M - (m0 + w * WTM)));
      }
      const float mean = st / fmaxf(nt, 1.f);
      float q = 0.f;
#pragma unroll
      for (int w = 0; w < NWM; ++w) {
        const float nw = (float)max(0, min(WTM, a.M - (m0 + w * WTM)));
        if (nw > 0.f) {
          const float d = red[w * BN + col] / nw - mean;
          q += red[(NWM + w) * BN + col] + nw * d * d;
        }
      }
      a.stats[(long)tile_m * 2 * a.Ng + n] = st;
      a.stats[(long)tile_m * 2 * a.Ng + a.Ng + n] = q;
    }
  }
}

template <int BM, int BN, int NWM, int NWN, Pipe PIPE, int NS, int POST, int TAPS = 0, bool PRE = false, int HA = 0>
__global__ __launch_bounds__(64 * NWM * NWN, (tn_waves_per_simd<BM, BN, NWM, NWN, PIPE>())) void tn_fast_kernel(FastTNArgs a) {
  tn_fast_body<BM, BN, NWM, NWN, PIPE, NS, POST, TAPS, PRE, HA>(a, blockIdx.x + gridDim.x * blockIdx.y, gridDim.x, gridDim.y);
}

// Several independent GEMMs of one configuration in one launch: the output-parity classes of a
// stride-2 data gradient (conv.hip plan_dgrad; 4 / 2 / 2 / 1 taps, a few hundred tiles each),
// which launched one after another left the chip mostly idle.  Blocks [start[k], start[k+1]) run
// GEMM k as its own gx[k] x gy[k] grid.
struct TNMulti {
  FastTNArgs c[4];
  int start[5];
  int gx[4], gy[4];
  int n;
};

template <int BM, int BN, int NWM, int NWN, Pipe PIPE, int NS, int POST>
__global__ __launch_bounds__(64 * NWM * NWN, (tn_waves_per_simd<BM, BN, NWM, NWN>())) void tn_multi_kernel(TNMulti m) {
  const int b = blockIdx.x;
  int k = 0;
  while (k + 1 < m.n && b >= m.start[k + 1]) ++k;
  tn_fast_body<BM, BN, NWM, NWN, PIPE, NS, POST, 0, false>(m.c[k], b - m.start[k], m.gx[k], m.gy[k]);
}

// One instantiation of record C: POST 0 / 1 (post 1 and 2, told apart at run time) / 3, TAPS compile-time
// taps of a gather ring (0: the generic ring; a halo-A ring has 9), PRE the input prologue.
template <typename C, int POST, int TAPS = 0, bool PRE = false>
int launch_tn_cfg(const FastTNArgs& a, hipStream_t st) {
  constexpr int BM = C::BM, BN = C::BN, NWM = C::NWM, NWN = C::NWN, NS = C::NS, HA = C::HA;
  constexpr Pipe PIPE = C::PIPE;
  constexpr int NT = 64 * NWM * NWN;
  // operand stages, or the epilogue's per-wave transpose tiles + stats scratch if larger; then the
  // input-prologue coefficients (PRE)
  constexpr size_t kMaxPre = 2 * 2048 * 4;
  constexpr size_t off = kPreOff<BM, BN, NWM, NWN, NS, HA>();
  const size_t lds = off + (PRE ? (size_t)2 * a.c1 * 4 : 0);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tn_fast_kernel<BM, BN, NWM, NWN, PIPE, NS, POST, TAPS, PRE, HA>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(off + (PRE ? kMaxPre : 0)));
    attr = true;
  }
  dim3 grid(ceil_div(a.M, BM), ceil_div(a.Ng, BN), 1);
  hipLaunchKernelGGL((tn_fast_kernel<BM, BN, NWM, NWN, PIPE, NS, POST, TAPS, PRE, HA>), grid, dim3(NT), lds, st, a);
  return 0;
}

// the plain / post-op arm of one tile
template <typename C, int TAPS>
int launch_tn_post(const FastTNArgs& a, hipStream_t st) {
  return a.post ? launch_tn_cfg<C, 1, TAPS>(a, st) : launch_tn_cfg<C, 0, TAPS>(a, st);
}

template <typename C, int POST>
int launch_tn_multi_cfg(const FastTNArgs* fs, int n, hipStream_t st) {
  constexpr int BM = C::BM, BN = C::BN, NWM = C::NWM, NWN = C::NWN, NS = C::NS;
  constexpr Pipe PIPE = C::PIPE;
  constexpr int NT = 64 * NWM * NWN;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tn_multi_kernel<BM, BN, NWM, NWN, PIPE, NS, POST>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPreOff<BM, BN, NWM, NWN, NS>());
    attr = true;
  }
  TNMulti m{};
  m.n = n;
  int total = 0;
  for (int k = 0; k < n; ++k) {
    m.c[k] = fs[k];
    m.gx[k] = ceil_div(fs[k].M, BM);
    m.gy[k] = ceil_div(fs[k].Ng, BN);
    m.start[k] = total;
    total += m.gx[k] * m.gy[k];
  }
  m.start[n] = total;
  constexpr size_t lds = kPreOff<BM, BN, NWM, NWN, NS>();
  hipLaunchKernelGGL((tn_multi_kernel<BM, BN, NWM, NWN, PIPE, NS, POST>), dim3(total), dim3(NT), lds, st, m);
  return 0;
}

// Compile-time tap count for the LDS-DMA ring (0 = generic ring): 3x3 and 1x1 filters, when the
// precomputed gather offsets (pixel index < 2^24, pbad * ldcb) fit the 24-bit multiply and 32 bits.
static int tn_taps(const FastTNArgs& a) {
  const int taps = a.nr * a.ns;
  if (taps != 9 && taps != 1) return 0;
  const unsigned long long p1 = a.x1_bytes / (unsigned)a.ldc1b;
  const unsigned long long p2 = a.x2 ? a.x2_bytes / (unsigned)a.ldc2b : 0ull;
  const unsigned long long pbad = (p1 > p2 ? p1 : p2) + 1ull;
  const unsigned long long ld = (unsigned)(a.ldc1b > a.ldc2b ? a.ldc1b : a.ldc2b);
  if (pbad >= (1ull << 24) || ld >= (1ull << 24) || pbad * ld + 256ull >= (1ull << 32)) return 0;
  return taps;
}

// The halo-A ring serves a 3x3 stride-1 "same" conv whose output grid tiles into 8 x 32 spatial blocks.
static bool halo_a_ok(const FastTNArgs& a) {
  // default since the round-3 A/B (+1.8 % end to end); UNETSEG_TN_NO_HALO_RING=1 keeps the gather
  // ring -- read per call so a test can run both rings in one process
  if (getenv("UNETSEG_TN_NO_HALO_RING") != nullptr || a.in_sc || a.nr != 3 || a.ns != 3 || a.istride != 1) return false;
  if (a.dhs * a.dhs != 1 || a.dws * a.dws != 1) return false;
  const int dh_lo = a.dhs > 0 ? a.dh0 : a.dh0 - 2, dw_lo = a.dws > 0 ? a.dw0 : a.dw0 - 2;
  if (dh_lo != -1 || dw_lo != -1) return false;  // one halo pixel on every side
  if (a.H != a.hc || a.W != a.wc || a.hc % 8 || a.wc % 32) return false;
  return tn_taps(a) == 9;
}

// The tile a call takes before the halo-A rings are considered (tn_config).
static int tn_config_base(const FastTNArgs& a) {
  if (const char* e = getenv("UNETSEG_TN_CFG")) {  // tools/conv_bench.py: force a register-staged or gather-ring tile
    const int c = atoi(e);
    if (c == kCfgHaloA256x128) return kCfgRing256x128;  // the halo-A ring where it applies (tn_config), else the gather ring
    bool ok = false;
    with_tn_cfg(c, [&](auto r) {
      using C = decltype(r);
      ok = !C::HA && !(a.in_sc && C::PIPE == Pipe::Ring);
    });
    if (ok) return c;
  }
  // the input prologue transforms registers between load and LDS store: register-staged tiles only
  const bool no_dma = a.in_sc != nullptr;
  if (!a.in_sc && halo3_ok(a)) return kCfgHalo;
  const int nsteps = a.nr * a.ns * (a.cin >> 6);
  // short K (<= 4 steps: the bottleneck 1x1 layers, HBM-bound) on one LDS stage, 3-4 blocks per CU
  // (128x128 with one step keeps its own single-step tile: as fast, fewer barriers)
  if (nsteps <= 4 && (nsteps >= 2 || a.Ng <= 64)) return a.Ng <= 64 ? kCfgShort128x64 : kCfgShort128x128;
  if (nsteps == 1 && a.Ng > 64) return kCfgTn128x128Step1;  // the prefetch stage would only cost occupancy
  // 128x64 (two-step prefetch, 3 blocks/CU): 5-10 % over 256x64; deep 3x3 K on the 3-stage ring
  // with compile-time taps: ~8 % more (192->64 at 256x256: 390 -> 357 us)
  if (a.Ng <= 64) return (!no_dma && nsteps >= 18 && tn_taps(a) == 9) ? kCfgRing128x64 : kCfgTn128x64;
  if (nsteps <= 4) return kCfgTn128x128;
  const long tiles_big = (long)ceil_div(a.M, 256) * ceil_div(a.Ng, 128);
  if (tiles_big >= 256) return no_dma ? kCfgTn256x128 : kCfgRing256x128;
  const long tiles_mid = (long)ceil_div(a.M, 128) * ceil_div(a.Ng, 128);
  // one or two 128x128 tiles per CU and a deep K: the 5-stage ring with compile-time taps (one
  // block per CU) beats the register-staged tile by ~25 % (3x3 256->256 at 32x32: 43 -> 34 us)
  if (tiles_mid >= 256) return (!no_dma && nsteps >= 16 && tn_taps(a)) ? kCfgRing128x128S5 : kCfgTn128x128;
  // 64-row tiles so that small-M layers still fill the chip
  return (!no_dma && nsteps >= 32) ? kCfgRing64x128 : kCfgTn64x128;
}

// kCfgHalo or the code of a kTnTable record: a gather ring gives way to the halo-A ring on its tile
static int tn_config(const FastTNArgs& a) {
  const int c = tn_config_base(a);
  if ((c == kCfgRing256x128 || c == kCfgRing128x64 || c == kCfgRing128x128S5) && halo_a_ok(a))
    return c == kCfgRing256x128 ? kCfgHaloA256x128 : c == kCfgRing128x64 ? kCfgHaloA256x64 : kCfgHaloA128x128;
  return c;
}

// row tile (BM) of a TN configuration
static int tn_cfg_bm(int cfg) {
  int bm = 128;
  with_tn_cfg(cfg, [&](auto r) { bm = decltype(r)::BM; });
  return bm;
}

}  // namespace

bool tn_fast_ok(const FastTNArgs& a) {
  return a.cin % 64 == 0 && a.c1 % 64 == 0 && a.nr * a.ns <= 32 && a.Ng % 8 == 0;
}

// Row tile of the BN partial statistics = the block's rows (BM) on the TN kernels, one 8x32
// spatial tile on the halo kernel.
int tn_fast_tile_m(const FastTNArgs& a) {
  const int cfg = tn_config(a);
  return cfg == kCfgHalo ? halo_tile_m() : tn_cfg_bm(cfg);
}

int tn_fast_post_rows(const FastTNArgs& a) {
  if (a.M <= 0 || a.Ng <= 0) return 0;
  const int cfg = tn_config(a);
  return cfg == kCfgHalo ? halo3_blocks(a) : ceil_div(a.M, tn_cfg_bm(cfg));
}

// the 256-row halo-A rings run persistent (conv_tn_persist.hip) when tn_persist_tiles says so
template <typename C>
static bool tn_persist(const FastTNArgs& a) {
  return C::HA && C::BM == 256 && !a.in_sc && a.post != 3 && a.post != 4 && tn_persist_tiles(a, C::BN) > 0;
}

int tn_fast_config(const FastTNArgs& a, int* taps_out) {
  int cfg = tn_config(a), taps = 0;
  with_tn_cfg(cfg, [&](auto r) {
    using C = decltype(r);
    if (tn_persist<C>(a)) cfg = C::BN == 128 ? kCfgPersist256x128 : kCfgPersist256x64;
    else if (C::PIPE == Pipe::Ring && !C::HA) taps = tn_taps(a);
  });
  if (taps_out) *taps_out = taps;
  return cfg;
}

// The configuration has a post-3 (residual-BN backward) instantiation for this call.
bool tn_fast_post_res_ok(const FastTNArgs& a) {
  bool ok = false;
  with_tn_cfg(tn_config(a), [&](auto r) {
    using C = decltype(r);
    ok = C::POST3 && (C::PIPE != Pipe::Ring || tn_taps(a) == 1);
  });
  return ok;
}

static int launch_tn_post_res(const FastTNArgs& a, hipStream_t st) {
  if (!tn_fast_post_res_ok(a)) return -1;
  int rc = -1;
  with_tn_cfg(tn_config(a), [&](auto r) {
    using C = decltype(r);
    if constexpr (C::POST3) rc = launch_tn_cfg<C, 3, C::PIPE == Pipe::Ring ? 1 : 0>(a, st);
  });
  return rc;
}

int launch_tn_fast(const FastTNArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.Ng <= 0) return 0;
  if (a.post == 3) return a.in_sc ? -1 : launch_tn_post_res(a, st);
  const int cfg = tn_config(a);
  if (a.post == 4) return cfg == kCfgHalo ? launch_halo3(a, st) : -1;  // mask bits: halo path only
  if (cfg == kCfgHalo) return a.in_sc ? -1 : launch_halo3(a, st);
  int rc = -1;
  with_tn_cfg(cfg, [&](auto r) {
    using C = decltype(r);
    if constexpr (C::PIPE != Pipe::Ring) {
      // input prologue (fwd only: no post-op) on the register-staged tiles
      rc = a.in_sc ? launch_tn_cfg<C, 0, 0, true>(a, st) : launch_tn_post<C, 0>(a, st);
    } else if (a.in_sc) {
      rc = -1;
    } else if constexpr (C::HA != 0) {
      rc = tn_persist<C>(a) ? launch_tn_persist(a, C::BN, C::HA, st) : launch_tn_post<C, 9>(a, st);
    } else {
      switch (tn_taps(a)) {
        case 9: rc = launch_tn_post<C, 9>(a, st); break;
        case 1: rc = launch_tn_post<C, 1>(a, st); break;
        default: rc = launch_tn_post<C, 0>(a, st);
      }
    }
  });
  return rc;
}

// Merged launch of 2-4 GEMMs (stride-2 data-gradient parity classes) on one register-staged tile:
// 128x128 (or 64x128 when any class would take a 64-row tile).  Returns -1 (nothing launched) when
// the classes cannot share one (input prologue, a halo class, more than 4).
int tn_multi_tile_m(const FastTNArgs* fs, int n) {
  if (n < 2 || n > 4) return -1;
  bool bm64 = false;
  for (int k = 0; k < n; ++k) {
    if (fs[k].in_sc || fs[k].M <= 0) return -1;
    const int cfg = tn_config(fs[k]);
    if (cfg == kCfgHalo) return -1;
    if (tn_cfg_bm(cfg) == 64) bm64 = true;
  }
  return bm64 ? 64 : 128;
}

int launch_tn_multi(const FastTNArgs* fs, int n, hipStream_t st) {
  const int bm = tn_multi_tile_m(fs, n);
  if (bm < 0) return -1;
  const bool post = fs[0].post != 0;
  if (bm == 64) return post ? launch_tn_multi_cfg<Tn64x128, 1>(fs, n, st) : launch_tn_multi_cfg<Tn64x128, 0>(fs, n, st);
  return post ? launch_tn_multi_cfg<Tn128x128, 1>(fs, n, st) : launch_tn_multi_cfg<Tn128x128, 0>(fs, n, st);
}
