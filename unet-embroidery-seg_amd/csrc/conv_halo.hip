// 3x3 stride-1 "same" convolutions with 64 input channels (fwd and stride-1 dgrad), bf16, gfx950.
//
// These are the high-resolution, narrow layers of the U-Net decoder (up_conv at 512^2, up_concat1 at
// 256^2) and of ResNet layer1 at 128^2.  The generic implicit GEMM re-reads every input pixel once
// per tap (9x) through L2 and restages the weights per 256-pixel tile; here:
//  * weights stay resident: one block owns one 64-channel output tile for its whole life and keeps
//    all 9 taps x 64 x 64 bf16 (72 KiB) in LDS;
//  * the input arrives as a 2D halo tile: (TH+2) x 34 pixels x 64 channels (42.5 KiB) serve a
//    TH x 32 output tile for all 9 taps (1.33 reads per pixel instead of 9);
//  * persistent blocks (one per CU) walk spatial tiles; the next tile's halo streams in by
//    LDS-DMA (buffer_load ... lds) while the current one is computed -- two halo stages;
//  * within a tile there is no barrier: 9 taps x 2 K-halves of MFMA straight from LDS;
//  * output stores are explicit buffer stores so the per-wave count of memory operations after the
//    next tile's DMA is a compile-time constant: the wait for that DMA is `vmcnt(FP*FC)` and never
//    waits on this tile's stores.
// Operand roles as in the TN kernels: weights = A (16 output channels per MFMA row block),
// pixels = B, so each lane's accumulator holds 4 consecutive output channels of one pixel.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "conv_fast.h"
#include "fast_util.h"

namespace {

constexpr int HW_TW = 32;  // output tile width (pixels)

// Halo pixel rows are read 16 at a time from an arbitrary start (the tap shift); XOR the chunk
// with hp & 7 (not (hp>>1) & 7 as for aligned rows): conflict-free ds_read_b128 for every start.
__device__ __forceinline__ int swzh(int hp, int ch) { return ch ^ (hp & 7); }

// ---- tile geometry shared by the kernels of this file ----
// spatial tile sp of a launch (tiles dealt row-major within an image, images in order)
struct Tile {
  int nb, th, tw;  // image, tile row, tile column
};
__device__ __forceinline__ Tile tile_of(int sp, int tiles_w, int tiles_h) {
  const int tw = sp % tiles_w, rest = sp / tiles_w;
  const int th = rest % tiles_h, nb = rest / tiles_h;
  return {nb, th, tw};
}

// A (TH + 2) x (HW_TW + 2) halo around the TH x HW_TW tile at (h0, w0).  With H % TH == 0 and
// W % HW_TW == 0 only the halo's border pixels can leave the image, so each DMA lane keeps the
// borders its pixel (hr, hc) lies on -- 1 top, 2 bottom, 4 left, 8 right, 16 a slot past the halo --
// and a tile's load is one mask test against the borders that tile has outside the image.
template <int TH>
__device__ __forceinline__ unsigned halo_flag(int hr, int hc, bool past) {
  return past ? 16u : (hr == 0 ? 1u : 0u) | (hr == TH + 1 ? 2u : 0u) | (hc == 0 ? 4u : 0u) | (hc == HW_TW + 1 ? 8u : 0u);
}
template <int TH>
__device__ __forceinline__ unsigned halo_kill(int h0, int w0, int H, int W) {
  return __builtin_amdgcn_readfirstlane(16u | (h0 == 0 ? 1u : 0u) | (h0 + TH >= H ? 2u : 0u) | (w0 == 0 ? 4u : 0u) |
                                        (w0 + HW_TW >= W ? 8u : 0u));
}
// uniform byte offset of the halo's top-left pixel (h0 - 1, w0 - 1) of image nb, pixel pitch ldb bytes:
// wraps below zero on the first row / column, whose lanes halo_kill sends out of range
__device__ __forceinline__ unsigned halo_origin(int nb, int h0, int w0, int H, int W, unsigned ldb) {
  return __builtin_amdgcn_readfirstlane((unsigned)((nb * H + h0 - 1) * W + w0 - 1) * ldb);
}

// Lane j16 + 16 kg of a wave that owns RPW rows of a tile: its pixel of the wave's 16-pixel group p
// (two groups per row) -- row and column within the tile, and the pixel's index in an [N][OH][OW] image
template <int RPW>
struct LanePix {
  int r, col;
  __device__ __forceinline__ LanePix(int wid, int p, int j16)
      : r(wid * RPW + p / (HW_TW / 16)), col((p % (HW_TW / 16)) * 16 + j16) {}
  // the pixel's tap (dh, dw) in a (TH + 2) x (HW_TW + 2) halo
  __device__ __forceinline__ int halo_px(int dh, int dw) const { return (r + 1 + dh) * (HW_TW + 2) + col + 1 + dw; }
  // I = int where the caller's extents are known to fit 32 bits
  template <int TH, typename I = long>
  __device__ __forceinline__ I opix(const Tile& tl, int OH, int OW) const {
    return ((I)tl.nb * OH + tl.th * TH + r) * OW + tl.tw * HW_TW + col;
  }
};

// EPI: epilogue flags fixed at compile time (kEpiBias | kEpiRelu | kEpiStats | kEpiAcc), or kEpiDyn
// to read them from the arguments; with them fixed the tile epilogue has no uniform branches and
// the bias sits in registers.
// kEpiHead1 / kEpiHead2: the model's final 1x1 conv (64 -> 1 or 2 logits) on the rounded outputs
// (model/unet_resnet.py:99-103 `final`, model/unet_multitask.py seg_head): the 512^2 activation is
// not read back by a separate head pass.
// kEpiMask: the ReLU mask of the stored output packed to bits, mbits_out[pixel][Ng/8] (bit e of byte b =
// channel 8b + e > 0) -- the consumer's data gradient (post 4) reads 1/16 of what the activation costs.
constexpr int kEpiBias = 1, kEpiRelu = 2, kEpiStats = 4, kEpiAcc = 8, kEpiDyn = 16, kEpiHead1 = 32, kEpiHead2 = 64,
              kEpiMask = 128;

// wait for half h of the HS pipeline and join the block: the vector-memory operations issued after
// half h's DMA may stay in flight -- the next two halves (D instructions each) and the aux loads (NA)
// / output stores (NS) issued in between (exact for the first three halves, whose predecessors are
// fewer).  A count below the true one only waits longer.
template <int D, int NA, int NS>
__device__ __forceinline__ void hs_wait(int h) {
  if (h == 0)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * D) : "memory");
  else if (h == 1)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * D + NA) : "memory");
  else if (h == 2)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * D + NA + NS) : "memory");
  else if (h & 1)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * D + 2 * NA + NS) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * D + NA + 2 * NS) : "memory");
}

// HS: the input arrives as 32-channel half tiles through FOUR half stages (the same 85 KiB as two
// whole-tile stages): a half tile's DMA is issued three half-steps before it is consumed, so 64 KiB
// stay in flight per CU instead of the 0-43 KiB of the double-buffered whole tiles, whose wait at
// every tile end left the waves parked (the 512^2 layers ran at ~2.7 TB/s).  Half-stage rows are
// 64 B (4 chunks, chunk ^ (bit 2 of the pixel) << 1: conflict-free 16-pixel reads from any start).
template <int TH, int NW, int POST, int EPI, bool HS = false>
__global__ __launch_bounds__(64 * NW) void halo3_kernel(FastTNArgs a, int tiles_w, int tiles_h, int n_sp, int G_per,
                                                        unsigned y_bytes) {
  constexpr bool kDyn = (EPI & kEpiDyn) != 0;
  const bool has_bias = kDyn ? a.bias != nullptr : (EPI & kEpiBias) != 0;
  const bool do_relu = kDyn ? a.relu != 0 : (EPI & kEpiRelu) != 0;
  const bool do_stats = kDyn ? a.stats != nullptr : (EPI & kEpiStats) != 0;
  const bool do_acc = kDyn ? a.accumulate != 0 : (EPI & kEpiAcc) != 0;
  constexpr int HK = (EPI & kEpiHead2) ? 2 : (EPI & kEpiHead1) ? 1 : 0;  // fused head logits
  static_assert(HK == 0 || (!kDyn && POST == 0), "the fused head rides on a fixed bias + ReLU epilogue");
  constexpr bool kMask = (EPI & kEpiMask) != 0;
  static_assert(!kMask || (!kDyn && POST == 0 && HK == 0 && (EPI & kEpiRelu)), "mask bits of a ReLU output");
  // POST 4: post 1 with the ReLU mask read from packed bits (a.mbits, the kEpiMask layout)
  // wave w owns output rows [w*TH/NW, (w+1)*TH/NW)
  constexpr int RPW = TH / NW;               // rows per wave
  constexpr int FP = RPW * (HW_TW / 16);     // 16-pixel groups per wave
  constexpr int FC = 4;                      // 16-channel output groups (64 output channels)
  constexpr int HP = (TH + 2) * (HW_TW + 2); // halo pixels
  constexpr int HCH = HP * 8;                // 16-B chunks per halo stage
  constexpr int HI = (HCH + 64 * NW - 1) / (64 * NW);  // halo DMA instructions per wave
  constexpr int WCH = 9 * 64 * 8;            // 16-B chunks of resident weights
  constexpr int WI = WCH / (64 * NW);        // weight DMA instructions per wave
  static_assert(TH % NW == 0 && WCH % (64 * NW) == 0, "tile shape");
  // the spread halo DMA issues piece i at tap step i of the 18-step loop: every piece must land on a
  // step that exists, or the next tile would read a partly loaded halo
  static_assert(HI <= 18, "halo pieces exceed the tap steps");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  uint4* wl = lds;                           // [9*64 rows][8 chunks]
  uint4* hl = lds + WCH;                     // [2][HP][8]
  float* red = reinterpret_cast<float*>(hl + 2 * HCH);  // [NW][64]
  float* sbias = red + NW * 64;              // [64]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  // block -> (output-channel tile, first spatial tile); spatial tiles dealt round-robin
  const int tn = blockIdx.x / G_per, slot = blockIdx.x % G_per;
  const int n0 = tn * 64;
  const int my_tiles = slot < n_sp ? (n_sp - slot + G_per - 1) / G_per : 0;
  const __amdgpu_buffer_rsrc_t rx = srd(a.x1, a.x1_bytes);
  const __amdgpu_buffer_rsrc_t rw = srd(a.wt, a.w_bytes);
  const __amdgpu_buffer_rsrc_t ry = srd(a.y, y_bytes);
  const unsigned hw_img = (unsigned)(a.OH * a.OW);
  const __amdgpu_buffer_rsrc_t rh = srd(HK ? (const void*)a.head_y : a.y,
                                        HK ? (unsigned)(a.M / (a.OH * a.OW)) * HK * hw_img * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rmb =
      srd(kMask ? (const void*)a.mbits_out : a.y, kMask ? (unsigned)a.M * (unsigned)(a.Ng >> 3) : 0u);
  const __amdgpu_buffer_rsrc_t rst =
      srd(do_stats ? (const void*)a.stats : a.y, do_stats ? (unsigned)n_sp * 2u * (unsigned)a.Ng * 4u : 0u);
  // post-op inputs: POST 4 the mask bits [M][Ng/8], POST 1 / 2 the pre-activation aux [M][ld_aux]
  const __amdgpu_buffer_rsrc_t raux =
      POST == 4 ? srd(a.mbits, (unsigned)a.M * (unsigned)(a.Ng >> 3))
                : srd(POST ? a.aux : a.y, POST ? (unsigned)a.M * (unsigned)a.ld_aux * 2u : 0u);

  if (kDyn && a.bias && tid < 64) sbias[tid] = a.bias[n0 + tid];
  // BN post-op coefficients of this block's 64 channels live in `red` (free in dgrad: no stats)
  float* pco = red;  // [4][64]: sc, sh, mean, inv
  if (POST == 2 && tid < 64) {
    pco[tid] = a.psc[n0 + tid];
    pco[64 + tid] = a.psh[n0 + tid];
    pco[128 + tid] = a.pmean[n0 + tid];
    pco[192 + tid] = a.pinv[n0 + tid];
  }

  // ---- resident weights: LDS row (jt, k) = weights of output channel n0+k at halo tap jt ----
  {
    const unsigned base = lds_addr(wl);
#pragma unroll 2
    for (int i = 0; i < WI; ++i) {
      const int inst = i * NW + wid;
      const int idx = inst * 64 + lane;
      const int row = idx >> 3, pc = idx & 7;
      const int jt = row >> 6, k = row & 63;
      const int jr = jt / 3, js = jt - jr * 3;
      const int wtap = (a.r0 + a.rs * jr) * a.S + (a.s0 + a.ss * js);
      const unsigned off = (unsigned)(n0 + k) * (unsigned)a.ldwb + (unsigned)(wtap * 128 + swz8(row, pc) * 16);
      dma16(rw, base + (unsigned)inst * 1024u, off);
    }
  }

  // ---- halo geometry of this lane's DMA slots (identical for every tile): byte offset relative to
  // the halo's top-left pixel (swizzle included) and its border flags (halo_flag), so a tile's load is
  // one add and one mask test per row ----
  unsigned hoff[HI], hflag[HI];
#pragma unroll
  for (int i = 0; i < HI; ++i) {
    const int idx = (i * NW + wid) * 64 + lane;
    const int hp = idx >> 3, hr = hp / (HW_TW + 2), hc = hp % (HW_TW + 2);
    hoff[i] = (unsigned)(hr * a.W + hc) * (unsigned)a.ldc1b + swzh(hp, lane & 7) * 16u;
    hflag[i] = halo_flag<TH>(hr, hc, idx >= HCH);
  }
  // halo DMA instructions this wave issues per tile: HI, or HI - 1 for the waves with no slot in the
  // last one (issue_halo skips it)
  const bool full_dma = HCH % (64 * NW) == 0 || ((HI - 1) * NW + wid) * 64 < HCH;
  auto issue_halo = [&](int t, int stage) {  // a whole halo at once: the first tile's
    const Tile tl = tile_of(slot + t * G_per, tiles_w, tiles_h);
    const int h0 = tl.th * TH, w0 = tl.tw * HW_TW;
    const unsigned base = __builtin_amdgcn_readfirstlane(lds_addr(hl + stage * HCH));
    const unsigned hb = halo_origin(tl.nb, h0, w0, a.H, a.W, (unsigned)a.ldc1b);
    const unsigned kill = halo_kill<TH>(h0, w0, a.H, a.W);
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      const unsigned off = (hflag[i] & kill) ? kOOB : hb + hoff[i];
      // only the last row can hold lanes past the halo (they must not write LDS)
      if (i < HI - 1 || HCH % (64 * NW) == 0 || hflag[i] != 16u) dma16(rx, base + (unsigned)((i * NW + wid) * 1024), off);
    }
  };

  // ---- half-stage geometry (HS): 4 chunks per halo pixel, HI2 DMA instructions per wave (the last
  // one only for the waves whose slots exist: waves 0..5 issue HI2, the rest HI2 - 1) ----
  constexpr int HCH2 = HP * 4;
  constexpr int HI2 = (HCH2 + 64 * NW - 1) / (64 * NW);
  constexpr int LASTW = (HCH2 - (HI2 - 1) * 64 * NW + 63) / 64;  // waves with slots in the last instruction
  unsigned hoff2[HS ? HI2 : 1], hflag2[HS ? HI2 : 1];
  if constexpr (HS) {
#pragma unroll
    for (int i = 0; i < HI2; ++i) {
      const int idx = (i * NW + wid) * 64 + lane;
      const int hp = idx >> 2, q = idx & 3;
      const int hr = hp / (HW_TW + 2), hc = hp % (HW_TW + 2);
      hoff2[i] = (unsigned)(hr * a.W + hc) * (unsigned)a.ldc1b + (unsigned)((q ^ (((hp >> 2) & 1) << 1)) * 16);
      hflag2[i] = halo_flag<TH>(hr, hc, idx >= HCH2);
    }
  }
  const bool last_dma = wid < LASTW;  // this wave issues the last half-stage instruction
  // half h = 2 t + kk (input channels 32 kk .. 32 kk + 31 of tile t) into half stage `stage`; halves
  // past this block's tiles load nothing (out of range) but are issued, so every wave's count is fixed
  auto issue_half = [&](int h, int stage) {
    const int t = h >> 1;
    const bool live = t < my_tiles;
    const Tile tl = tile_of(live ? slot + t * G_per : slot, tiles_w, tiles_h);
    const int h0 = tl.th * TH, w0 = tl.tw * HW_TW;
    const unsigned base = __builtin_amdgcn_readfirstlane(lds_addr(hl + stage * HCH2));
    const unsigned hb = halo_origin(tl.nb, h0, w0, a.H, a.W, (unsigned)a.ldc1b) + (unsigned)(h & 1) * 64u;
    const unsigned kill = halo_kill<TH>(h0, w0, a.H, a.W);
#pragma unroll
    for (int i = 0; i < HI2; ++i) {
      const unsigned off = (!live || (hflag2[i] & kill)) ? kOOB : hb + hoff2[i];
      if (i < HI2 - 1) {
        dma16(rx, base + (unsigned)((i * NW + wid) * 1024), off);
      } else if (last_dma) {
        if (hflag2[i] != 16u) dma16(rx, base + (unsigned)((i * NW + wid) * 1024), off);
      }
    }
  };

  f32x4 acc[FC][FP];
  // data-gradient post-op (a.post): running per-lane sums of the masked gradient over all tiles of
  // this block, reduced once at the end into ppart[blockIdx.x][2][Ng]
  float pq0[FC][4], pq1[FC][4];
#pragma unroll
  for (int c = 0; c < FC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) pq0[c][e] = pq1[c][e] = 0.f;
  // per-wave vector-memory operations of one tile's epilogue, counted from the loops that issue them
  // (each issues its full count on every wave: inactive lanes go out of range, nothing is skipped):
  //   aux loads (post op): POST 4 one 8-B mask load per 16-pixel group, POST 1/2 one per (group, channel
  //   group); stores: FP x FC outputs, FP x HK head logits, FP mask words
  constexpr int NA_ = POST == 4 ? FP : POST ? FP * FC : 0;
  constexpr int NS_ = FP * FC + FP * HK + (kMask ? FP : 0);
  // (operations issued beyond these -- the accumulate epilogue's old-value loads -- only make a wait
  // wait longer; a count above the true one would not wait for the DMA)
  static_assert(!HS || 2 * HI2 + 2 * NA_ + 2 * NS_ <= 63, "hs_wait counts must fit vmcnt's 6 bits");
  auto half_wait = [&](int h) {
    if (last_dma) hs_wait<HI2, NA_, NS_>(h);
    else hs_wait<HI2 - 1, NA_, NS_>(h);
  };
  if constexpr (HS) {
    issue_half(0, 0);
    issue_half(1, 1);
    issue_half(2, 2);
  } else {
    if (my_tiles > 0) issue_halo(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }

  // halo tap offsets (uniform): jt -> (dh, dw)
  const int dh0 = a.dh0, dhs = a.dhs, dw0 = a.dw0, dws = a.dws;
  const int j16 = lane & 15, kg = lane >> 4;
  // fused head: this lane's 16 channels' head weights in registers (one block per CU: VGPRs are free)
  float hwr[HK > 0 ? HK : 1][FC][4], hbr[HK > 0 ? HK : 1];
#pragma unroll
  for (int k = 0; k < HK; ++k) {
    hbr[k] = a.head_b[k];
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) hwr[k][c][e] = a.head_w[k * 64 + c * 16 + kg * 4 + e];
  }
  float breg[FC][4];  // this lane's 16 output channels' bias (compile-time flags only)
#pragma unroll
  for (int c = 0; c < FC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) breg[c][e] = (!kDyn && has_bias) ? a.bias[n0 + c * 16 + kg * 4 + e] : 0.f;

  for (int t = 0; t < my_tiles; ++t) {
    const int stage = t & 1;
    if constexpr (HS) {
      half_wait(2 * t);
      issue_half(2 * t + 3, (2 * t + 3) & 3);
    }
    // post-op: this tile's aux values are loaded now, so their latency hides under the tap loop: NA_
    // loads per wave.  HS: plain loads after this half step's DMA (hs_wait counts them).  Double
    // buffer: they go out BEFORE the next tile's DMA, as buffer loads the compiler does not track,
    // and the epilogue waits for them with vmcnt(this wave's DMA count): waiting on loads issued
    // after the DMA (in-order counter) retired the next tile's halo inside this tile -- the prefetch
    // was gone (16 x 512^2 post 4: 397 us against 281 for the plain data gradient)
    uint2 zr[FC][FP];
    uint2 zb[FP];  // POST 4: the 8 mask bytes (64 channels) of this lane's pixel
    if (POST) {
      const Tile tl = tile_of(slot + t * G_per, tiles_w, tiles_h);
      // 8 bytes at `off` of the mask bits [M][Ng/8] (POST 4) / the pre-activation aux [M][ld_aux];
      // the buffer loads take 32-bit offsets and their arithmetic stays 32-bit (halo3_ok bounds the extents)
      using Pix = std::conditional_t<HS, long, int>;
      using Off = std::conditional_t<HS, long, unsigned>;
      auto aux_load = [&](Off off) -> uint2 {
        if constexpr (!HS) return bload64_asm(raux, off);
        else return *reinterpret_cast<const uint2*>((POST == 4 ? (const char*)a.mbits : (const char*)a.aux) + off);
      };
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        const Off opix = (Off)LanePix<RPW>(wid, p, j16).template opix<TH, Pix>(tl, a.OH, a.OW);
        if (POST == 4) {
          zb[p] = aux_load(opix * (Off)(a.Ng >> 3) + (Off)(n0 >> 3));
        } else {
#pragma unroll
          for (int c = 0; c < FC; ++c) zr[c][p] = aux_load((opix * (Off)a.ld_aux + (Off)(n0 + c * 16 + kg * 4)) * 2);
        }
      }
    }
    // the next tile's halo DMA, one instruction per tap step at the first HI steps of the MFMA
    // loop below: issued all at once here, the eight waves spent their issue cycles together at the
    // tile start with the MFMA pipes idle (16 x 512^2 fwd 313 -> 302 us, fwd + statistics 448 -> 433 us)
    // (the pieces are issue_halo's loop body, one per step: the same per-wave count)
    const bool dma_next = t + 1 < my_tiles;
    unsigned nx_base = 0u, nx_hb = 0u, nx_kill = 0u;
    if constexpr (!HS) {
      if (dma_next) {
        const Tile tl = tile_of(slot + (t + 1) * G_per, tiles_w, tiles_h);
        const int h0 = tl.th * TH, w0 = tl.tw * HW_TW;
        nx_base = __builtin_amdgcn_readfirstlane(lds_addr(hl + (stage ^ 1) * HCH));
        nx_hb = halo_origin(tl.nb, h0, w0, a.H, a.W, (unsigned)a.ldc1b);
        nx_kill = halo_kill<TH>(h0, w0, a.H, a.W);
      }
    }
    auto issue_piece = [&](int i) {
      if (!dma_next) return;
      const unsigned off = (hflag[i] & nx_kill) ? kOOB : nx_hb + hoff[i];
      if (i < HI - 1 || HCH % (64 * NW) == 0 || hflag[i] != 16u) dma16(rx, nx_base + (unsigned)((i * NW + wid) * 1024), off);
    };
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int p = 0; p < FP; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (HS) {
      // half kk = input channels 32 kk .. 32 kk + 31: all nine taps, then the next half
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk == 1) {
          half_wait(2 * t + 1);
          issue_half(2 * t + 4, (2 * t + 4) & 3);
        }
        const uint4* hs2 = hl + ((2 * t + kk) & 3) * HCH2;
        const int ch = kk * 4 + kg;
#pragma unroll
        for (int jt = 0; jt < 9; ++jt) {
          const int jr = jt / 3, js = jt - jr * 3;
          const int dh = dh0 + dhs * jr, dw = dw0 + dws * js;
          bf16x8 wf[FC], pf[FP];
#pragma unroll
          for (int c = 0; c < FC; ++c) {
            const int row = jt * 64 + c * 16 + j16;
            uint4 v = wl[row * 8 + swz8(row, ch)];
            wf[c] = *reinterpret_cast<bf16x8*>(&v);
          }
#pragma unroll
          for (int p = 0; p < FP; ++p) {
            const int hp = LanePix<RPW>(wid, p, j16).halo_px(dh, dw);
            uint4 v = hs2[hp * 4 + (kg ^ (((hp >> 2) & 1) << 1))];
            pf[p] = *reinterpret_cast<bf16x8*>(&v);
          }
#pragma unroll
          for (int c = 0; c < FC; ++c)
#pragma unroll
            for (int p = 0; p < FP; ++p)
              acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], pf[p], acc[c][p], 0, 0, 0);
        }
      }
    } else {
      // 18 steps (tap jt, K half kk), software-pipelined: the fragments of step s+1 are read before
      // the MFMAs of step s and sched_group_barrier pins that order -- left to itself the scheduler
      // issued each read right before its MFMAs, and with 2 MFMAs per LDS round trip the waves sat on
      // lgkmcnt (MFMA busy 45 %, SQ_LDS_IDX_ACTIVE 34 % at 512^2)
      const uint4* hs = hl + stage * HCH;
      auto frag_load = [&](int st, bf16x8 (&wf)[FC], bf16x8 (&pf)[FP]) {
        const int jt = st >> 1, kk = st & 1;
        const int jr = jt / 3, js = jt - jr * 3;
        const int dh = dh0 + dhs * jr, dw = dw0 + dws * js;
        const int ch = kk * 4 + kg;
#pragma unroll
        for (int c = 0; c < FC; ++c) {
          const int row = jt * 64 + c * 16 + j16;
          uint4 v = wl[row * 8 + swz8(row, ch)];
          wf[c] = *reinterpret_cast<bf16x8*>(&v);
        }
#pragma unroll
        for (int p = 0; p < FP; ++p) {
          const int hp = LanePix<RPW>(wid, p, j16).halo_px(dh, dw);
          uint4 v = hs[hp * 8 + swzh(hp, ch)];
          pf[p] = *reinterpret_cast<bf16x8*>(&v);
        }
      };
      bf16x8 wfb[2][FC], pfb[2][FP];
      frag_load(0, wfb[0], pfb[0]);
      __builtin_amdgcn_sched_group_barrier(0x100, FC + FP, 0);
#pragma unroll
      for (int st = 0; st < 18; ++st) {
        if (st + 1 < 18) frag_load(st + 1, wfb[(st + 1) & 1], pfb[(st + 1) & 1]);
#pragma unroll
        for (int c = 0; c < FC; ++c)
#pragma unroll
          for (int p = 0; p < FP; ++p)
            acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfb[st & 1][c], pfb[st & 1][p], acc[c][p], 0, 0, 0);
        if (st + 1 < 18) __builtin_amdgcn_sched_group_barrier(0x100, FC + FP, 0);  // DS reads of step st+1
        __builtin_amdgcn_sched_group_barrier(0x008, FC * FP, 0);                    // MFMAs of step st
        if (st < HI) issue_piece(st);  // piece st of the next tile's halo
      }
    }

    // ================= epilogue =================
    if (!HS && POST) {
      // this tile's aux loads landed; the next tile's halo (this wave's DMAs, issued after them) may fly
      if (t + 1 < my_tiles) {
        if (full_dma)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HI) : "memory");
        else
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HI - 1) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        if (POST == 4) {
          asm volatile("" : "+v"(zb[p]));
        } else {
#pragma unroll
          for (int c = 0; c < FC; ++c) asm volatile("" : "+v"(zr[c][p]));
        }
      }
    }
    const Tile tl = tile_of(slot + t * G_per, tiles_w, tiles_h);
    float csum[FC][4];
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) csum[c][e] = 0.f;
    uint2 outv[FC][FP];
    unsigned outo[FP], mko[FP], mkx[FP], mky[FP];
#pragma unroll
    for (int p = 0; p < FP; ++p) {
      const long opix = LanePix<RPW>(wid, p, j16).template opix<TH>(tl, a.OH, a.OW);
      outo[p] = (unsigned)(opix * a.ldy + n0) * 2u;
      mko[p] = (unsigned)(opix * (a.Ng >> 3) + (n0 >> 3));
      mkx[p] = mky[p] = 0u;
#pragma unroll
      for (int c = 0; c < FC; ++c) {
        const int cb = c * 16 + kg * 4;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[c][p][e] + (!has_bias ? 0.f : kDyn ? sbias[cb + e] : breg[c][e]);
          if (do_relu) v[e] = fmaxf(v[e], 0.f);
        }
        if (do_acc) {
          const bf16* ob = reinterpret_cast<const bf16*>((const char*)a.y + outo[p] + cb * 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += (float)ob[e];
        }
        bf16 o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16)v[e];
          v[e] = (float)o[e];
        }
        if (POST) {  // mask with the producer's ReLU (from aux or its bits) and accumulate backward partials
          const bf16* z = reinterpret_cast<const bf16*>(&zr[c][p]);
          // POST 4: byte 2c + kg/2 of the pixel's 8, high nibble for odd kg
          const unsigned nib =
              POST == 4 ? ((c < 2 ? zb[p].x : zb[p].y) >> ((((2 * c + (kg >> 1)) & 3) * 8) + (kg & 1) * 4)) & 15u : 0u;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float zf = POST == 4 ? 0.f : (float)z[e];
            bool on = POST == 4 ? ((nib >> e) & 1u) != 0u : zf > 0.f;
            float xh = 0.f;
            if (POST == 2) {
              const int ch = cb + e;
              on = fmaf(zf, pco[ch], pco[64 + ch]) > 0.f;
              xh = (zf - pco[128 + ch]) * pco[192 + ch];
            }
            v[e] = on ? v[e] : 0.f;
            o[e] = (bf16)v[e];
            pq0[c][e] += v[e];
            if (POST == 2) pq1[c][e] += v[e] * xh;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          csum[c][e] += v[e];
          acc[c][p][e] = v[e];
        }
        outv[c][p] = *reinterpret_cast<uint2*>(o);
        if (kMask) {  // this lane's 4 channels -> its nibble of byte 2c + kg/2 (word x: c < 2, y: c >= 2)
          unsigned nb4 = 0u;
#pragma unroll
          for (int e = 0; e < 4; ++e) nb4 |= (v[e] > 0.f ? 1u : 0u) << e;
          const unsigned sh = (((2 * c + (kg >> 1)) & 3) * 8) + (kg & 1) * 4;
          if (c < 2) mkx[p] |= nb4 << sh;
          else mky[p] |= nb4 << sh;
        }
      }
    }
    if (kMask) {  // OR the four channel groups' nibbles (lanes j16 + 16 kg): disjoint bits
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        mkx[p] |= __shfl_xor(mkx[p], 16);
        mkx[p] |= __shfl_xor(mkx[p], 32);
        mky[p] |= __shfl_xor(mky[p], 16);
        mky[p] |= __shfl_xor(mky[p], 32);
      }
    }
    if (HK) {
      // head logits of this lane's pixels: 16 channels per lane, then the four channel groups
      // (lanes j16 + 16 kg) summed by cross-row shuffles; lanes kg == 0 store, the others' stores
      // go out of range (every wave issues exactly FP * HK head stores)
#pragma unroll
      for (int p = 0; p < FP; ++p) {
        const LanePix<RPW> lp(wid, p, j16);
        const unsigned pix = (unsigned)((tl.th * TH + lp.r) * a.OW + tl.tw * HW_TW + lp.col);  // within the image
#pragma unroll
        for (int k = 0; k < HK; ++k) {
          float hs = 0.f;
#pragma unroll
          for (int c = 0; c < FC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) hs = fmaf(acc[c][p][e], hwr[k][c][e], hs);
          hs += __shfl_xor(hs, 16);
          hs += __shfl_xor(hs, 32);
          hs += hbr[k];
          bstore32(rh, kg == 0 ? ((unsigned)(tl.nb * HK + k) * hw_img + pix) * 4u : kOOB, hs);
        }
      }
    }
    if (do_stats) {
      // per-tile BN partials over the TH*32 pixels (sum, M2 about the tile mean): each wave reduces its
      // own 16 * FP pixels to (sum, M2 about the wave mean) in registers -- the 16 channel values of a
      // lane reduced together over the row's 16 lanes (row16_sum_n) -- and wave 0 merges the NW waves
      // (Chan: M2 = sum M2_w + n_w (mean_w - mean)^2), the sums and then the M2s passing through `red`
      // (no room in LDS for both at once).  Until round 5 every lane fetched the tile mean of its 16
      // channels from LDS and the 32 row reductions ran one chain at a time: the statistics epilogue
      // cost almost half as much as the convolution (16 x 512^2: 475 vs 325 us)
      float sv[FC * 4], qv[FC * 4];
#pragma unroll
      for (int c = 0; c < FC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[c * 4 + e] = csum[c][e];
      row16_sum_n(sv);
#pragma unroll
      for (int c = 0; c < FC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float mw = sv[c * 4 + e] * (1.0f / (16 * FP));
          float q = 0.f;
#pragma unroll
          for (int p = 0; p < FP; ++p) {
            const float d = acc[c][p][e] - mw;
            q += d * d;
          }
          qv[c * 4 + e] = q;
        }
      row16_sum_n(qv);
      if (j16 == 0)
#pragma unroll
        for (int c = 0; c < FC; ++c)
          *reinterpret_cast<float4*>(red + wid * 64 + c * 16 + kg * 4) =
              float4{sv[c * 4], sv[c * 4 + 1], sv[c * 4 + 2], sv[c * 4 + 3]};
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      float sw[NW];
      if (tid < 64)
#pragma unroll
        for (int w = 0; w < NW; ++w) sw[w] = red[w * 64 + tid];
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // sums read: reuse red for M2
      if (j16 == 0)
#pragma unroll
        for (int c = 0; c < FC; ++c)
          *reinterpret_cast<float4*>(red + wid * 64 + c * 16 + kg * 4) =
              float4{qv[c * 4], qv[c * 4 + 1], qv[c * 4 + 2], qv[c * 4 + 3]};
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      float tot = 0.f, q = 0.f;
      if (tid < 64) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          tot += sw[w];
          q += red[w * 64 + tid];
        }
        const float mean = tot * (1.0f / (TH * HW_TW));
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const float d = sw[w] * (1.0f / (16 * FP)) - mean;
          q = fmaf((float)(16 * FP) * d, d, q);
        }
      }
      // buffer stores issued by every wave (only wave 0's land), counted in the tile's closing wait:
      // as plain stores of wave 0 alone they were retired by that wait -- a full write round trip per
      // tile with the whole block parked on the barrier behind it (16 x 512^2: +140 us)
      const unsigned so = tid < 64 ? (unsigned)((slot + t * G_per) * 2 * a.Ng + n0 + tid) * 4u : kOOB;
      bstore32(rst, so, tot);
      bstore32(rst, tid < 64 ? so + (unsigned)a.Ng * 4u : kOOB, q);
    }
    // output stores last: exactly FP*FC buffer stores per wave after the next tile's DMA
#pragma unroll
    for (int p = 0; p < FP; ++p)
#pragma unroll
      for (int c = 0; c < FC; ++c) bstore64(ry, outo[p] + (c * 16 + kg * 4) * 2, outv[c][p]);
    // mask bytes: lanes kg == 0 store the pixel's 8 bytes, the others' stores go out of range (every
    // wave issues exactly FP of them)
    if (kMask)
#pragma unroll
      for (int p = 0; p < FP; ++p) bstore64(rmb, kg == 0 ? mko[p] : kOOB, uint2{mkx[p], mky[p]});
    // next halo landed (all but this tile's stores retired) and every wave is done with both the
    // current stage (WAR for the DMA after next) and `red` (HS: the next half's wait does both)
    // (HS: the two statistics stores are not in hs_wait's counts -- it waits for them too, which is
    // only slower)
    if constexpr (!HS) {
      if (do_stats)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NS_ + 2) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NS_) : "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // HS: the past-the-end halves are still landing in the stages of other waves
  if constexpr (HS) asm volatile("s_barrier" ::: "memory");
  if (POST) {
    // lanes -> waves -> block: ppart[blockIdx.x][2][Ng] for this block's 64 output channels (the
    // halo stages are free now: every wave has passed the last tile's barrier)
    float* pr = reinterpret_cast<float*>(hl);  // [NW][2][64]
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t0 = row16_sum(pq0[c][e]), t1 = POST == 2 ? row16_sum(pq1[c][e]) : 0.f;
        if (j16 == 0) {
          pr[(wid * 2 + 0) * 64 + c * 16 + kg * 4 + e] = t0;
          pr[(wid * 2 + 1) * 64 + c * 16 + kg * 4 + e] = t1;
        }
      }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (tid < 128) {
      const int k = tid >> 6, ch = tid & 63;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += pr[(w * 2 + k) * 64 + ch];
      a.ppart[(long)blockIdx.x * 2 * a.Ng + k * a.Ng + n0 + ch] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The ResNet stem forward (model/resnet_backbone.py:126-131: 7x7 / stride 2 / pad 3, 3 -> 64) on the
// same persistent-halo plan.  The input is the width-packed xp bf16 [N][H][W+8][8] (conv.hip: image
// column w at packed column w+3, channels 3..7 and the 3+5 border columns zero), so filter row fr of
// output (p, q) is the 8 consecutive packed pixels 2q .. 2q+7 of input row 2p+fr-3: one 64-wide K
// chunk (8 taps x 8 channels, tap 7 has zero weight).  The TN stem gathered those 128 B per output
// pixel and filter row from L2 (7 x 128 B per pixel, 14x the input) and re-read its 57 KB of weights
// per 128-pixel tile; here a block keeps the weights (7 x 64 x 64 bf16) in LDS and streams one
// (2*TH+5) x 70 packed-pixel patch per TH x 32 output tile (TH = 16: 40.5 KB; each input pixel is
// fetched ~1.3 times instead of 14).  MFMA roles as in halo3_kernel: weights = A (16 output channels per MFMA row
// block), pixels = B (lane j16 + 16 kg reads packed pixel 2*col + 4*kk + kg of its patch row).
// Epilogue: the BN partial statistics of each tile (sum, M2 about the tile mean) -> stats[tile][2][64].
// ------------------------------------------------------------------------------------------
constexpr int kStemTH = 16;                  // output rows per tile (two per wave: each weight
                                             // fragment read from LDS feeds 4 pixel groups)
constexpr int kStemPR = 2 * kStemTH + 5;     // patch rows
constexpr int kStemPC = 2 * HW_TW + 6;       // patch columns (packed pixels)
// A patch row is stored even packed columns first, then odd ones: the 16 lanes of a pixel fragment
// read columns 2*col + ch (col = 16 consecutive pixels), i.e. 16 consecutive LDS units -- with the
// natural order they were 32 B apart and lanes j16 and j16 + 8 hit the same banks.
__device__ __forceinline__ int stem_pos(int hc) { return (hc & 1) ? kStemPC / 2 + (hc >> 1) : hc >> 1; }
__device__ __forceinline__ int stem_col(int pos) { return pos < kStemPC / 2 ? 2 * pos : 2 * (pos - kStemPC / 2) + 1; }

template <int NW, int NST>
__global__ __launch_bounds__(64 * NW) void stem_halo_kernel(const bf16* xp, unsigned x_bytes, const bf16* wk, int H,
                                                            int Wp, int P, int Q, int n_sp, bf16* y, int ldy,
                                                            unsigned y_bytes, float* stats) {
  constexpr int TH = kStemTH;
  constexpr int RPW = TH / NW;
  constexpr int FP = RPW * (HW_TW / 16);
  constexpr int FC = 4;
  constexpr int HP = kStemPR * kStemPC;            // 16-B units (packed pixels) per patch
  constexpr int HI = (HP + 64 * NW - 1) / (64 * NW);
  constexpr int HPP = HI * 64 * NW;                // a stage padded to whole DMA instructions: every
                                                   // wave issues exactly HI per patch (exact vmcnt)
  constexpr int ST_PER_TILE = FP * FC + 2;         // stores per wave and tile (outputs + 2 stats)
  constexpr int WCH = 7 * 64 * 8;                  // 16-B chunks of resident weights
  constexpr int WI = WCH / (64 * NW);
  static_assert(TH % NW == 0 && WCH % (64 * NW) == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  uint4* wl = lds;                  // [7*64 rows][8 chunks]
  uint4* hl = lds + WCH;            // [NST][HPP]
  float* red = reinterpret_cast<float*>(hl + NST * HPP);  // [NW][64]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = blockIdx.x, G_per = gridDim.x;
  const int my_tiles = slot < n_sp ? (n_sp - slot + G_per - 1) / G_per : 0;
  const int tiles_w = Q / HW_TW, tiles_h = P / TH;
  const __amdgpu_buffer_rsrc_t rx = srd(xp, x_bytes);
  const __amdgpu_buffer_rsrc_t rw = srd(wk, 64u * 7u * 128u);
  const __amdgpu_buffer_rsrc_t ry = srd(y, y_bytes);
  const __amdgpu_buffer_rsrc_t rs = srd(stats, (unsigned)n_sp * 128u * 4u);

  // resident weights: LDS row (fr, k) = wk[k][fr][0..63]
  {
    const unsigned base = lds_addr(wl);
#pragma unroll 2
    for (int i = 0; i < WI; ++i) {
      const int inst = i * NW + wid;
      const int idx = inst * 64 + lane;
      const int row = idx >> 3, pc = idx & 7;
      const int fr = row >> 6, k = row & 63;
      dma16(rw, base + (unsigned)inst * 1024u, (unsigned)(k * 7 + fr) * 128u + (unsigned)swz8(row, pc) * 16u);
    }
  }
  // patch geometry of this lane's DMA slots: offset from the patch origin and whether the unit lies in
  // the 3 rows above or the 2 rows below the image (only those can leave it; columns never do)
  unsigned hoff[HI], hflag[HI];
#pragma unroll
  for (int i = 0; i < HI; ++i) {
    const int idx = (i * NW + wid) * 64 + lane;
    const int hr = idx / kStemPC, hc = stem_col(idx - hr * kStemPC);  // LDS position -> packed column
    hoff[i] = (unsigned)(hr * Wp + hc) * 16u;
    hflag[i] = idx >= HP ? 16u : (hr < 3 ? 1u : 0u) | (hr >= 2 * TH + 3 ? 2u : 0u);
  }
  auto issue_patch = [&](int t, int stage) {
    const Tile tl = tile_of(slot + t * G_per, tiles_w, tiles_h);
    const int h0 = tl.th * TH, w0 = tl.tw * HW_TW;
    const unsigned base = __builtin_amdgcn_readfirstlane(lds_addr(hl + stage * HPP));
    // origin row 2*h0 - 3 wraps below zero on the first tile row; those lanes are killed
    const unsigned hb = __builtin_amdgcn_readfirstlane((unsigned)((tl.nb * H + 2 * h0 - 3) * Wp + 2 * w0) * 16u);
    const unsigned kill = __builtin_amdgcn_readfirstlane(16u | (h0 == 0 ? 1u : 0u) | (h0 + TH >= P ? 2u : 0u));
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      const unsigned off = (hflag[i] & kill) ? kOOB : hb + hoff[i];  // padding units: zeros
      dma16(rx, base + (unsigned)((i * NW + wid) * 1024), off);
    }
  };

  f32x4 acc[FC][FP];
  // NST-stage patch ring: patches 0 .. NST-2 in flight before the first tile, patch t + NST - 1 issued
  // as tile t starts (a tile's MFMA work is ~0.8 us, far below the DMA latency under load)
#pragma unroll
  for (int q = 0; q < NST - 1; ++q)
    if (q < my_tiles) issue_patch(q, q);
  if (my_tiles >= NST - 1)  // weights and patch 0 landed (patches 1 .. NST-2 may still fly)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((NST - 2) * HI) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const int j16 = lane & 15, kg = lane >> 4;

  for (int t = 0; t < my_tiles; ++t) {
    const int stage = t % NST;
    if (t + NST - 1 < my_tiles) issue_patch(t + NST - 1, (t + NST - 1) % NST);
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int p = 0; p < FP; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* hs = hl + stage * HPP;
#pragma unroll
    for (int fr = 0; fr < 7; ++fr) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int ch = kk * 4 + kg;
        bf16x8 wf[FC], pf[FP];
#pragma unroll
        for (int c = 0; c < FC; ++c) {
          const int row = fr * 64 + c * 16 + j16;
          uint4 v = wl[row * 8 + swz8(row, ch)];
          wf[c] = *reinterpret_cast<bf16x8*>(&v);
        }
#pragma unroll
        for (int p = 0; p < FP; ++p) {
          const int r = wid * RPW + p / (HW_TW / 16);
          const int col = (p % (HW_TW / 16)) * 16 + j16;
          uint4 v = hs[(2 * r + fr) * kStemPC + stem_pos(2 * col + ch)];
          pf[p] = *reinterpret_cast<bf16x8*>(&v);
        }
#pragma unroll
        for (int c = 0; c < FC; ++c)
#pragma unroll
          for (int p = 0; p < FP; ++p)
            acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[c], pf[p], acc[c][p], 0, 0, 0);
      }
    }

    // epilogue: round to bf16, BN partials of the rounded values, stores last
    const int sp = slot + t * G_per;
    const Tile tl = tile_of(sp, tiles_w, tiles_h);
    float csum[FC][4];
    uint2 outv[FC][FP];
    unsigned outo[FP];
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) csum[c][e] = 0.f;
#pragma unroll
    for (int p = 0; p < FP; ++p) {
      const int r = wid * RPW + p / (HW_TW / 16);
      const int col = (p % (HW_TW / 16)) * 16 + j16;
      const long opix = ((long)tl.nb * P + tl.th * TH + r) * Q + tl.tw * HW_TW + col;
      outo[p] = (unsigned)(opix * ldy) * 2u;
#pragma unroll
      for (int c = 0; c < FC; ++c) {
        bf16 o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (bf16)acc[c][p][e];
          const float v = (float)o[e];
          acc[c][p][e] = v;
          csum[c][e] += v;
        }
        outv[c][p] = *reinterpret_cast<uint2*>(o);
      }
    }
    // BN partials as halo3_kernel's: (sum, M2 about the wave mean) per wave in registers, merged by
    // wave 0 (Chan), the sums and then the M2s through `red`
    float sv[FC * 4], qv[FC * 4];
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) sv[c * 4 + e] = csum[c][e];
    row16_sum_n(sv);
#pragma unroll
    for (int c = 0; c < FC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mw = sv[c * 4 + e] * (1.0f / (16 * FP));
        float q = 0.f;
#pragma unroll
        for (int p = 0; p < FP; ++p) {
          const float d = acc[c][p][e] - mw;
          q += d * d;
        }
        qv[c * 4 + e] = q;
      }
    row16_sum_n(qv);
    if (j16 == 0)
#pragma unroll
      for (int c = 0; c < FC; ++c)
        *reinterpret_cast<float4*>(red + wid * 64 + c * 16 + kg * 4) =
            float4{sv[c * 4], sv[c * 4 + 1], sv[c * 4 + 2], sv[c * 4 + 3]};
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float sw[NW], stot = 0.f;
    if (tid < 64)
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        sw[w] = red[w * 64 + tid];
        stot += sw[w];
      }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (j16 == 0)
#pragma unroll
      for (int c = 0; c < FC; ++c)
        *reinterpret_cast<float4*>(red + wid * 64 + c * 16 + kg * 4) =
            float4{qv[c * 4], qv[c * 4 + 1], qv[c * 4 + 2], qv[c * 4 + 3]};
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    {
      float q = 0.f;
      if (tid < 64) {
        const float mean = stot * (1.0f / (TH * HW_TW));
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          q += red[w * 64 + tid];
          const float d = sw[w] * (1.0f / (16 * FP)) - mean;
          q = fmaf((float)(16 * FP) * d, d, q);
        }
      }
      // every wave issues both stats stores (only wave 0's lanes land): exact per-wave counts
      const unsigned so = tid < 64 ? (unsigned)(sp * 128 + tid) * 4u : kOOB;
      bstore32(rs, so, stot);
      bstore32(rs, tid < 64 ? so + 256u : kOOB, q);
    }
#pragma unroll
    for (int p = 0; p < FP; ++p)
#pragma unroll
      for (int c = 0; c < FC; ++c) bstore64(ry, outo[p] + (c * 16 + kg * 4) * 2, outv[c][p]);
    // patch t + 1 landed and every wave is done with the current stage and `red`.  In the steady
    // state (patch t + 1 issued inside the loop, patches t + 2 .. t + NST - 1 issued) exactly
    // (NST - 2) patches and (NST - 1) tiles' stores were issued after it; near either end, wait for
    // all but this tile's stores (conservative)
    if (t >= NST - 2 && t + NST - 1 < my_tiles)
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((NST - 2) * HI + (NST - 1) * ST_PER_TILE)
                   : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(ST_PER_TILE) : "memory");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------
// wgrad of the same convolutions: dW[k][tap][c] = sum_pix dY[pix][k] * X[pix + off(tap)][c].
// Block group = (64 output channels, 64 input channels); persistent over TH x 32 spatial tiles,
// each tile = dY tile (256 px x 64 ch) + X halo (340 px x 64 ch) by LDS-DMA, double buffered.
// Wave w owns input channels 16w .. 16w+15 of the 9 taps: 4 x 9 accumulators of 16x16.
// Fragments come from pixel-major LDS with ds_read_b64_tr_b16 (K = 32 pixels of one output row);
// the halo rows of a tap are the output row's pixels shifted by (dh, dw), so the same transposed
// read serves all 9 taps.  Partials go to slab[slot] in the natural [cout][tap*cin + c] layout of
// the split-K reduce.
// ------------------------------------------------------------------------------------------
// NW = 8: two waves per SIMD -- wave w owns input channels 16 (w % 4) .. of the 9 taps for output
// channels 32 (w / 4) .. 32 (w / 4) + 31 (the X fragments are read by both halves; the single wave per
// SIMD of a 4-wave block left the MFMA pipe idle while its own LDS reads were in flight).
template <int TH, int NW>
__global__ __launch_bounds__(64 * NW) void halo3_wgrad_kernel(HaloWgradArgs a, int tiles_w, int tiles_h, int n_sp,
                                                              int G_per) {
  constexpr int TP = TH * HW_TW;              // output pixels per tile
  constexpr int HP = (TH + 2) * (HW_TW + 2);  // halo pixels
  constexpr int DCH = TP * 8, HCH = HP * 8;   // 16-B chunks per stage part
  constexpr int DI = DCH / (64 * NW);         // dY DMA instructions per wave
  constexpr int HI = (HCH + 64 * NW - 1) / (64 * NW);
  constexpr int STG = DCH + HCH;              // uint4 per stage
  constexpr int FM = 2, FN = 9;
  static_assert(NW == 8 && DCH % (64 * NW) == 0, "tile shape");
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wid & 3, wm = wid >> 2;  // input-channel group, output-channel half
  const int mtiles = a.Cout >> 6;
  const int grp = blockIdx.x / G_per, slot = blockIdx.x % G_per;
  const int mt = grp % mtiles, ct = grp / mtiles;
  const int my_tiles = slot < n_sp ? (n_sp - slot + G_per - 1) / G_per : 0;
  const bool first = ct * 64 < a.c1;
  const __amdgpu_buffer_rsrc_t rx = first ? srd(a.x1, a.x1_bytes) : srd(a.x2, a.x2_bytes);
  const unsigned ldxb = first ? (unsigned)a.ldc1b : (unsigned)a.ldc2b;
  const unsigned xcb = (unsigned)(first ? ct * 64 : ct * 64 - a.c1) * 2u;
  const __amdgpu_buffer_rsrc_t rdy = srd(a.dy, a.dy_bytes);
  const unsigned dycb = (unsigned)mt * 128u;

  // Lane constants of the DMA rows, so that a tile's loads cost one add (+ the halo edge test) per
  // row: the byte offset relative to the tile's first pixel (dY) / its halo's top-left pixel (X),
  // swizzle included, and for the halo its border flags (halo_flag).
  const int pc = lane & 7;
  unsigned doff[DI];
#pragma unroll
  for (int i = 0; i < DI; ++i) {
    const int px = ((i * NW + wid) * 64 + lane) >> 3;
    doff[i] = (unsigned)((px / HW_TW) * a.W + px % HW_TW) * (unsigned)a.ldyb + dycb + (unsigned)((pc ^ swz_tr8(px)) * 16);
  }
  unsigned hoff[HI], hflag[HI];
#pragma unroll
  for (int i = 0; i < HI; ++i) {
    const int idx = (i * NW + wid) * 64 + lane;
    const int hp = idx >> 3, hr = hp / (HW_TW + 2), hc = hp % (HW_TW + 2);
    hoff[i] = (unsigned)(hr * a.W + hc) * ldxb + xcb + (unsigned)((pc ^ swz_tr8(hp)) * 16);
    hflag[i] = halo_flag<TH>(hr, hc, idx >= HCH);
  }
  auto issue = [&](int t, int stage) {
    const Tile tl = tile_of(slot + t * G_per, tiles_w, tiles_h);
    const int h0 = tl.th * TH, w0 = tl.tw * HW_TW;
    const unsigned base = __builtin_amdgcn_readfirstlane(lds_addr(lds + stage * STG));
    const unsigned tb = __builtin_amdgcn_readfirstlane((unsigned)((tl.nb * a.H + h0) * a.W + w0) * (unsigned)a.ldyb);
#pragma unroll
    for (int i = 0; i < DI; ++i) dma16(rdy, base + (unsigned)((i * NW + wid) * 1024), tb + doff[i]);
    const unsigned hbase = base + DCH * 16;
    const unsigned hb = halo_origin(tl.nb, h0, w0, a.H, a.W, ldxb);
    const unsigned kill = halo_kill<TH>(h0, w0, a.H, a.W);
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      const unsigned off = (hflag[i] & kill) ? kOOB : hb + hoff[i];
      // only the last row can hold lanes past the halo (they must not write LDS)
      if (i < HI - 1 || HCH % (64 * NW) == 0 || hflag[i] != 16u) dma16(rx, hbase + (unsigned)((i * NW + wid) * 1024), off);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (my_tiles > 0) issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const int g = lane >> 4, i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3;
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  // Transposed fragment reads with no per-read address arithmetic.  A read covers image rows
  // R + 8g + qq and R + 8g + qq + 4 (lane-dependent) at 16-B chunk c; the swizzle depends on row
  // bits 1 and 3 only, so with R = B + rho (B a multiple of 16, rho = R mod 16 known at compile
  // time once the row loop is unrolled) the lane's byte offset is B * 128 (an immediate) plus a
  // per-lane value precomputed for each rho.  Wave w owns input channels 16w .. 16w+15 of all 9
  // taps, so every tap's (dh, dw) -- and with it R -- is a compile-time constant.
  auto lane_off = [&](int x, int chunk) -> unsigned {
    return (unsigned)(x * 128 + ((chunk ^ swz_tr8(x)) * 16) + (pp & 1) * 8);
  };
  unsigned pa[FM][2], pb[16][2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int i = 0; i < FM; ++i) pa[i][k] = lane_off(8 * g + qq + 4 * k, (wm * FM + i) * 2 + (pp >> 1));
#pragma unroll
    for (int r = 0; r < 16; ++r) pb[r][k] = lane_off(r + 8 * g + qq + 4 * k, wc * 2 + (pp >> 1));
  }
  auto tr2 = [&](const char* base, unsigned o0, unsigned o1) -> bf16x8 {
    s16x4 va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + o0));
    s16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + o1));
    s16x8 v = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
    return *reinterpret_cast<bf16x8*>(&v);
  };

  for (int t = 0; t < my_tiles; ++t) {
    const int stage = t & 1;
    if (t + 1 < my_tiles) issue(t + 1, stage ^ 1);
    const char* dbase = reinterpret_cast<const char*>(lds + stage * STG);
    const char* hbase = dbase + DCH * 16;
#pragma unroll
    for (int rr = 0; rr < TH; ++rr) {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = tr2(dbase + rr * HW_TW * 128, pa[i][0], pa[i][1]);
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int dh = j / 3 - 1, dw = j % 3 - 1;
        const int R = (rr + 1 + dh) * (HW_TW + 2) + 1 + dw, rho = R & 15;
        bfr[j] = tr2(hbase + (R - rho) * 128, pb[rho][0], pb[rho][1]);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // slab[slot][cout][tap*cin + c]
  const long Ng = 9L * a.cin;
  float* ws = a.ws + (long)slot * a.Cout * Ng;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = mt * 64 + (wm * FM + i) * 16 + g * 4 + e;
#pragma unroll
      for (int j = 0; j < FN; ++j) ws[(long)m * Ng + (long)j * a.cin + ct * 64 + wc * 16 + i16] = acc[i][j][e];
    }
}

template <int TH, int NW>
size_t halo_lds_bytes() {
  return (size_t)9 * 64 * 128 + 2 * (size_t)(TH + 2) * (HW_TW + 2) * 128 + NW * 64 * 4 + 64 * 4;
}

constexpr int kHalo3TH = 8, kHalo3NW = 8;  // tile rows and waves of every halo3_kernel launch
constexpr int kWgradTH = 8;                 // tile rows of halo3_wgrad_kernel

// the TH x HW_TW spatial tiles of n_img images of h x w pixels
struct HaloTiles {
  int tiles_w, tiles_h, n_sp;
};
HaloTiles halo_tiles(int n_img, int h, int w, int TH) {
  const int tiles_w = w / HW_TW, tiles_h = h / TH;
  return {tiles_w, tiles_h, n_img * tiles_h * tiles_w};
}

// grid of a halo3 launch: ntn output-channel tiles x G_per persistent blocks each, about one block per
// CU in all, which walk the n_sp spatial tiles
struct HaloGrid {
  int tiles_w, tiles_h, n_sp, ntn, G_per;
};
HaloGrid halo_grid(const FastTNArgs& a, int TH) {
  const HaloTiles t = halo_tiles(a.M / (a.hc * a.wc), a.hc, a.wc, TH);
  const int ntn = a.Ng / 64;
  int G_per = 256 / ntn;
  if (G_per < 1) G_per = 1;
  if (G_per > t.n_sp) G_per = t.n_sp;
  return {t.tiles_w, t.tiles_h, t.n_sp, ntn, G_per};
}

// raise kernel K's dynamic LDS limit to `bytes`, once per instantiation
template <auto K>
void allow_lds(size_t bytes) {
  static const hipError_t once =
      hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  (void)once;
}

}  // namespace

int halo_tile_m() { return kHalo3TH * HW_TW; }

bool halo3_ok(const FastTNArgs& a) {
  static const bool off = getenv("UNETSEG_NO_HALO") != nullptr;
  if (off) return false;
  if (a.x2 || a.c1 != 64 || a.cin != 64 || a.nr != 3 || a.ns != 3 || a.istride != 1) return false;
  if (a.dhs * a.dhs != 1 || a.dws * a.dws != 1) return false;
  const int dh_lo = a.dhs > 0 ? a.dh0 : a.dh0 - 2, dw_lo = a.dws > 0 ? a.dw0 : a.dw0 - 2;
  if (dh_lo != -1 || dw_lo != -1) return false;  // halo of one pixel on every side
  if (a.ostride != 1 || a.ph || a.pw || a.OH != a.hc || a.OW != a.wc || a.H != a.hc || a.W != a.wc) return false;
  if (a.Ng % 64 || a.hc % kHalo3TH || a.wc % HW_TW) return false;
  if ((long)a.M * a.ldy * 2 >= (1L << 31)) return false;
  if (a.post && a.post != 4 && (long)a.M * a.ld_aux * 2 >= (1L << 31)) return false;
  if (a.post == 4 && (long)a.M * (a.Ng >> 3) >= (1L << 31)) return false;
  return true;
}

template <int POST, int EPI, bool HS>
static int launch_halo3_hs(const FastTNArgs& a, hipStream_t st) {
  constexpr int TH = kHalo3TH, NW = kHalo3NW;
  const HaloGrid g = halo_grid(a, TH);
  const size_t lds = halo_lds_bytes<TH, NW>();
  allow_lds<&halo3_kernel<TH, NW, POST, EPI, HS>>(lds);
  const unsigned y_bytes = (unsigned)((long)a.M * a.ldy * 2);
  hipLaunchKernelGGL((halo3_kernel<TH, NW, POST, EPI, HS>), dim3(g.ntn * g.G_per), dim3(64 * NW), lds, st, a, g.tiles_w,
                     g.tiles_h, g.n_sp, g.G_per, y_bytes);
  return 0;
}

// The half-stage pipeline (HS) (UNETSEG_HALO_HS=1; default: the whole-tile double buffer; read per
// call, the parity tests run both).  Isolated, a 512^2 layer (64 tiles per
// block) is slower with it (fwd 349-363 vs 296-312 us: a second barrier per tile) and a 256^2 one
// faster (104.8 vs 124.6 us: the three-half prologue hides the first tile's load).  Round 4 (eager
// host) measured HS everywhere best in the step (C2 972.8 vs 962.1 img/s); with the replayed step plan
// of round 5 the double buffer is (C2 1016-1019 vs 1010-1011 on one box, 958-959 vs 957 on another).
template <int POST, int EPI>
static int launch_halo3_cfg(const FastTNArgs& a, hipStream_t st) {
  const char* e = getenv("UNETSEG_HALO_HS");
  const bool hs = e != nullptr && atoi(e) != 0;
  if (hs) return launch_halo3_hs<POST, EPI, true>(a, st);
  return launch_halo3_hs<POST, EPI, false>(a, st);
}

// blocks (= post-op partial rows) of a launch_halo3 call
int halo3_blocks(const FastTNArgs& a) {
  const HaloGrid g = halo_grid(a, kHalo3TH);
  return g.ntn * g.G_per;
}

int launch_halo3(const FastTNArgs& a, hipStream_t st) {
  // fused dgrad post-ops are separate instantiations: their registers must not cost the plain path
  const int epi = (a.bias ? kEpiBias : 0) | (a.relu ? kEpiRelu : 0) | (a.stats ? kEpiStats : 0) |
                  (a.accumulate ? kEpiAcc : 0);
  if (a.head_y) {  // fused head: bias + ReLU epilogue only (checked by the caller)
    if (a.post || epi != (kEpiBias | kEpiRelu) || (a.head_k != 1 && a.head_k != 2)) return -1;
    return a.head_k == 2 ? launch_halo3_cfg<0, kEpiBias | kEpiRelu | kEpiHead2>(a, st)
                         : launch_halo3_cfg<0, kEpiBias | kEpiRelu | kEpiHead1>(a, st);
  }
  if (a.mbits_out) {  // ReLU mask bits: bias + ReLU epilogue only (checked by the caller)
    if (a.post || epi != (kEpiBias | kEpiRelu)) return -1;
    return launch_halo3_cfg<0, kEpiBias | kEpiRelu | kEpiMask>(a, st);
  }
  if (a.post == 4) return epi == 0 ? launch_halo3_cfg<4, 0>(a, st) : -1;
  // fused dgrad post-ops come with a plain epilogue (no bias / ReLU / stats / accumulate): the C ABI's
  // post-op data gradient always plans with none of them, so no call reaches the kEpiDyn fallbacks of
  // post 1 / 2 today (compiled, untested)
  if (a.post == 1) return epi == 0 ? launch_halo3_cfg<1, 0>(a, st) : launch_halo3_cfg<1, kEpiDyn>(a, st);
  if (a.post == 2) return epi == 0 ? launch_halo3_cfg<2, 0>(a, st) : launch_halo3_cfg<2, kEpiDyn>(a, st);
  // the epilogues the U-Net runs: conv+bias+ReLU (decoder), conv with BN statistics (encoder),
  // plain data gradient, accumulated data gradient; any other combination reads its flags at run time
  switch (epi) {
    case kEpiBias | kEpiRelu: return launch_halo3_cfg<0, kEpiBias | kEpiRelu>(a, st);
    case kEpiStats: return launch_halo3_cfg<0, kEpiStats>(a, st);
    case 0: return launch_halo3_cfg<0, 0>(a, st);
    case kEpiAcc: return launch_halo3_cfg<0, kEpiAcc>(a, st);
    default: return launch_halo3_cfg<0, kEpiDyn>(a, st);
  }
}

// the stem forward on stem_halo_kernel: 64 output channels, even input sizes with P % 16 == 0 and
// Q % 32 == 0 (UNETSEG_STEM_TN=1: the TN stem)
bool stem_halo_ok(int n, int h, int w, int K, int ldy) {
  if (getenv("UNETSEG_STEM_TN")) return false;
  if (K != 64 || ldy < 64 || ldy % 4 || n <= 0 || h % 2 || w % 2) return false;
  const int P = h / 2, Q = w / 2;
  if (P % kStemTH || Q % HW_TW) return false;
  return (long)n * h * (w + 8) * 16 < (1L << 31) && (long)n * P * Q * ldy * 2 < (1L << 31);
}

int stem_halo_tiles(int n, int h, int w) { return n * (h / 2 / kStemTH) * (w / 2 / HW_TW); }
int stem_halo_tile_m() { return kStemTH * HW_TW; }

int launch_stem_halo(const void* xp, int n, int h, int w, const void* wk, void* y, int ldy, float* stats,
                     hipStream_t st) {
  constexpr int NW = 8, NST = 2;
  const int P = h / 2, Q = w / 2, Wp = w + 8;
  const int n_sp = stem_halo_tiles(n, h, w);
  const int blocks = n_sp < 256 ? n_sp : 256;
  constexpr int HPP = (kStemPR * kStemPC + 64 * NW - 1) / (64 * NW) * (64 * NW);
  const size_t lds = (size_t)7 * 64 * 128 + (size_t)NST * HPP * 16 + NW * 64 * 4;
  allow_lds<&stem_halo_kernel<NW, NST>>(lds);
  hipLaunchKernelGGL((stem_halo_kernel<NW, NST>), dim3(blocks), dim3(64 * NW), lds, st, (const bf16*)xp,
                     (unsigned)((long)n * h * Wp * 16), (const bf16*)wk, h, Wp, P, Q, n_sp, (bf16*)y, ldy,
                     (unsigned)((long)n * P * Q * ldy * 2), stats);
  return 0;
}

bool halo3_wgrad_ok(const HaloWgradArgs& a) {
  static const bool off = getenv("UNETSEG_NO_HALO") != nullptr;
  if (off) return false;
  return a.cin % 64 == 0 && a.c1 % 64 == 0 && a.Cout % 64 == 0 && a.H % kWgradTH == 0 && a.W % HW_TW == 0;
}

// Blocks per (cout, cin) group: one persistent block per CU at a time (152 KiB LDS), so the
// makespan is ceil(groups*G / 256) rounds of ceil(n_sp / G) tiles, plus the split-K reduce that
// reads G slabs.  Pick the G that minimises that estimate (tile ~1 us with 8 waves, reduce ~4 TB/s;
// A/B against the 4-wave kernel's 2 us: +0.3-0.9 %).
int halo3_wgrad_splits(const HaloWgradArgs& a) {
  const int groups = (a.Cout / 64) * (a.cin / 64);
  const int n_sp = halo_tiles(a.N, a.H, a.W, kWgradTH).n_sp;
  const double slab = 4.0 * a.Cout * 9.0 * a.cin;
  int best = 1;
  double best_t = 1e30;
  // with the weight gradients on their own stream the makespan matters less than the slab traffic
  // the reduce adds beside the compute stream: UNETSEG_HALO_WG_MAXG caps G (experiments)
  static const int maxg = getenv("UNETSEG_HALO_WG_MAXG") ? atoi(getenv("UNETSEG_HALO_WG_MAXG")) : 512;
  // seconds per (8 x 32)-pixel tile of one block (the makespan model; UNETSEG_HALO_WG_TILE_US overrides)
  static const double tile_s = (getenv("UNETSEG_HALO_WG_TILE_US") ? atof(getenv("UNETSEG_HALO_WG_TILE_US")) : 1.0) * 1e-6;
  // with several (cout, cin) groups, the blocks of one slot in different groups walk the same spatial
  // tiles in step; G a multiple of 8 would put them on one XCD (block b runs on XCD b % 8), so a tile's
  // dY or X halo came from that XCD's L2 after the first read -- but it forces G >= 8 and with it
  // G slabs of split-K partials (the 32^2 concat conv: 453 MB written and re-read by the reduce).  Any
  // G measured better in the step (round 4, three interleaved repeats: C2 979.8 vs 976.2 img/s, C4
  // 423.5 vs 418.8, C5 783.6 vs 765.9, allocator peak 8.11 vs 8.39 GiB); UNETSEG_HALO_WG_XCD=1 restores it
  static const bool xcd = getenv("UNETSEG_HALO_WG_XCD") && atoi(getenv("UNETSEG_HALO_WG_XCD")) != 0;
  const int step = (xcd && groups > 1) ? 8 : 1;
  for (int g = step; g <= maxg && g <= n_sp; g += step) {
    if (slab * g > 768.0 * (1 << 20)) break;  // workspace cap
    const double rounds = (double)((groups * g + 255) / 256);
    const double t = rounds * ((n_sp + g - 1) / g) * tile_s + slab * g / 4e12;
    if (t < best_t * 0.999) {
      best_t = t;
      best = g;
    }
  }
  return best;
}

int launch_halo3_wgrad(const HaloWgradArgs& a, int G_per, hipStream_t st) {
  constexpr int TH = kWgradTH;
  const HaloTiles t = halo_tiles(a.N, a.H, a.W, TH);
  const int groups = (a.Cout / 64) * (a.cin / 64);
  const size_t lds = 2 * ((size_t)TH * HW_TW + (size_t)(TH + 2) * (HW_TW + 2)) * 128;
  allow_lds<&halo3_wgrad_kernel<TH, 8>>(lds);
  hipLaunchKernelGGL((halo3_wgrad_kernel<TH, 8>), dim3(groups * G_per), dim3(512), lds, st, a, t.tiles_w, t.tiles_h,
                     t.n_sp, G_per);
  return 0;
}
