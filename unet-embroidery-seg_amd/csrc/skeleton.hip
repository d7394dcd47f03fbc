// Hard skeleton of class maps by topology-preserving parallel thinning (unetseg_hip/skeleton.py: the
// clDice metric of val.py and of the evaluate loops, the centerline export of predict.py; no reference
// counterpart), and the pair counts the clDice metric (Shit et al., CVPR 2021, section 3) is read from.
//
// The rule is Guo & Hall's two-subiteration algorithm (CACM 32(3), 1989, algorithm A1), per class.
// cls int32 [N][H][W]; class 0 is background; the classes are 1 .. 255, and a pixel with any other value
// counts as background and comes out 0.  A neighbour of pixel q counts as set iff it lies inside the image
// and has the class of q, so thinning a multi-class map is the union of thinning each class mask on its
// own.  With the neighbours of (y, x) named
//   P9 (y-1, x-1)   P2 (y-1, x)   P3 (y-1, x+1)
//   P8 (y,   x-1)                 P4 (y,   x+1)
//   P7 (y+1, x-1)   P6 (y+1, x)   P5 (y+1, x+1)
// and
//   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
//   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)
//   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
//   N  = min(N1, N2)
// a subiteration deletes (sets to 0) every non-zero pixel with C == 1, 2 <= N <= 3 and m == 0, where the
// first subiteration of a pass has m = (P6|P7|!P9) & P8 and the second m = (P2|P3|!P5) & P4.  Each
// subiteration is evaluated on the map as it stood before it.  A pass is the two subiterations in that
// order; thinning of an image ends after the first pass that deletes nothing, or after max_passes passes.
// unconverged[n] = 1 iff the last pass executed on image n still deleted a pixel; max_passes = 0 runs no
// pass and reports 0.
//
// Launches, all on the caller's stream, none waits on the host; their number is
// 2 + ceil(max_passes / kK), whatever the data:
//   1. pack:   cls -> one byte per pixel (map A of the workspace); the flags are cleared.
//   2. thin, ceil(max_passes / kK) times, map A -> map B -> map A ...: a block owns a kTW x kTH tile of one
//      image and stages it with a halo of 2 kK pixels in LDS.  A subiteration reads a 3 x 3 neighbourhood,
//      so after p passes everything further than 2 p pixels from the staged region's rim is what the whole
//      image would hold: kK passes (the last launch: the rest of max_passes) run between two LDS copies and
//      only the tile is written back.  Halo pixels are recomputed by every tile that needs them from the same
//      bytes, so no tile size and no kK shows in the result.  A thread takes four pixels of a row: nine
//      32-bit LDS reads and one write for them.  The staged region has a rim of zero bytes that no
//      subiteration writes, so no neighbour read needs a bounds test; pixels outside the image are zero and
//      stay so.  A region that is all background after staging writes its (zero) tile and is done; a pass
//      that changes nothing in the whole region ends the block's passes, because the next would not either.
//   3. finish: out = cls where the byte survived, else 0; unconverged[n] = the last launch's last-pass flag.
// Flags, int32, per image: a ring of three "a tile pixel was deleted in this launch" slots and one
// "deleted in the last pass of the last launch" word.  Launch l sets slot l % 3 (atomic or), reads slot
// (l - 1) % 3 and clears slot (l + 1) % 3 (one plain store by the image's first tile): three different words,
// so no launch reads a word that a block of the same launch writes.  A block whose image's previous launch
// deleted nothing returns at once: that launch's output equals its input, so both maps hold the image's
// final state and map (launches % 2) is right for every image.  Only deletions inside the tile count for a
// flag: a deletion in the halo is another tile's to report.
//
// Everything is integer and every decision is taken from values that do not depend on the order of the
// blocks, so the result is bitwise reproducible.
#include "seg_pixel.h"

namespace {

constexpr int kTW = 64;  // tile width
constexpr int kTH = 64;  // tile height
constexpr int kK = 4;    // passes per launch
constexpr int kHalo = 2 * kK;
constexpr int kRW = kTW + 2 * kHalo;  // staged region
constexpr int kRH = kTH + 2 * kHalo;
constexpr int kPitch = kRW + 8;       // a zero dword on either side of a row
constexpr int kRows = kRH + 2;        // a zero row above and below
constexpr int kLdsWords = kRows * kPitch / 4;
constexpr int kGroupsX = kRW / 4;     // a thread's unit: four pixels of a row
constexpr int kMaxClass = 255;
static_assert(kHalo % 4 == 0 && kTW % 4 == 0 && kPitch % 4 == 0, "a four-pixel group lies wholly inside or outside the tile");

#define SKEL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the workspace: map A | map B (bytes, each rounded up to 256) | flags int32 [4][N]
struct SkelLayout {
  size_t map, flags, bytes;
  SkelLayout(size_t total, int N) {
    map = up256(total);
    flags = 2 * map;
    bytes = flags + up256(4 * (size_t)N * sizeof(int));
  }
};

using SkelTiles = TileGrid<kTW, kTH>;

// ---- pack / finish ----------------------------------------------------------------------------------
// thread = four consecutive pixels of the flat batch; map is 4-byte aligned and padded to a multiple of 4
__global__ __launch_bounds__(256) void skel_pack_kernel(const int* cls, long total, uint32_t* map, int* flags,
                                                        int nflags) {
  const long groups = (total + 3) / 4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = i0 + k < total ? cls[i0 + k] : 0;
      w |= (v >= 1 && v <= kMaxClass ? (uint32_t)v : 0u) << (8 * k);
    }
    map[g] = w;
  }
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < nflags; i += 256) flags[i] = 0;
}

__global__ __launch_bounds__(256) void skel_finish_kernel(const int* cls, const uint32_t* map, long total, int* out,
                                                          const int* last, int N, int* unconverged) {
  const long groups = (total + 3) / 4;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += gridDim.x * 256L) {
    const long i0 = g * 4;
    const uint32_t w = map[g];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < total) out[i0 + k] = (w >> (8 * k)) & 0xFFu ? cls[i0 + k] : 0;
  }
  if (unconverged && blockIdx.x == 0)
    for (int n = threadIdx.x; n < N; n += 256) unconverged[n] = last ? (last[n] != 0 ? 1 : 0) : 0;
}

// ---- one subiteration on four pixels ----------------------------------------------------------------
// up, mid, dn: bytes x-1 .. x+4 of the rows y-1, y, y+1 (byte j = column x-1+j); returns the bytes x .. x+3 of
// row y after subiteration `sub`
__device__ __forceinline__ uint32_t thin4(uint64_t up, uint64_t mid, uint64_t dn, int sub) {
  uint32_t res = (uint32_t)(mid >> 8);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned v = (unsigned)(mid >> (8 * (k + 1))) & 0xFFu;
    if (v == 0) continue;
    const int p9 = ((unsigned)(up >> (8 * k)) & 0xFFu) == v, p2 = ((unsigned)(up >> (8 * k + 8)) & 0xFFu) == v,
              p3 = ((unsigned)(up >> (8 * k + 16)) & 0xFFu) == v;
    const int p8 = ((unsigned)(mid >> (8 * k)) & 0xFFu) == v, p4 = ((unsigned)(mid >> (8 * k + 16)) & 0xFFu) == v;
    const int p7 = ((unsigned)(dn >> (8 * k)) & 0xFFu) == v, p6 = ((unsigned)(dn >> (8 * k + 8)) & 0xFFu) == v,
              p5 = ((unsigned)(dn >> (8 * k + 16)) & 0xFFu) == v;
    const int C = ((p2 ^ 1) & (p3 | p4)) + ((p4 ^ 1) & (p5 | p6)) + ((p6 ^ 1) & (p7 | p8)) + ((p8 ^ 1) & (p9 | p2));
    const int n1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8);
    const int n2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9);
    const int n = n1 < n2 ? n1 : n2;
    const int m = sub == 0 ? ((p6 | p7 | (p9 ^ 1)) & p8) : ((p2 | p3 | (p5 ^ 1)) & p4);
    if (C == 1 && n >= 2 && n <= 3 && m == 0) res &= ~(0xFFu << (8 * k));
  }
  return res;
}

// the word w (four pixels) of the staged region s after subiteration `sub`
__device__ __forceinline__ uint32_t thin_word(const uint32_t* s, int w, int sub) {
  constexpr int kP = kPitch / 4;
  const uint32_t c = s[w];
  if (c == 0) return 0;
  const uint64_t up = (uint64_t)(s[w - kP - 1] >> 24) | (uint64_t)s[w - kP] << 8 | (uint64_t)(s[w - kP + 1] & 0xFFu) << 40;
  const uint64_t mid = (uint64_t)(s[w - 1] >> 24) | (uint64_t)c << 8 | (uint64_t)(s[w + 1] & 0xFFu) << 40;
  const uint64_t dn = (uint64_t)(s[w + kP - 1] >> 24) | (uint64_t)s[w + kP] << 8 | (uint64_t)(s[w + kP + 1] & 0xFFu) << 40;
  return thin4(up, mid, dn, sub);
}

// the word of group g of the staged region (row g / kGroupsX, pixels 4 (g % kGroupsX) ..)
__device__ __forceinline__ int group_word(int ry, int gx) { return ((ry + 1) * kPitch + 4 + gx * 4) / 4; }

// ---- kK passes on a tile ----------------------------------------------------------------------------
// src, dst: byte maps [N][H][W].  prev (NULL in the first launch) / cur / next: the flag slots of the previous, this
// and the next launch; last (NULL unless this is the last launch): the last-pass word.  All int32 [N].
__global__ __launch_bounds__(256) void skel_thin_kernel(const uint8_t* src, uint8_t* dst, int H, int W, int tiles_x,
                                                        int tiles_y, int passes, const int* prev, int* cur, int* next,
                                                        int* last) {
  __shared__ uint32_t S0[kLdsWords];
  __shared__ uint32_t S1[kLdsWords];
  __shared__ unsigned chg[kK];
  const SkelTiles::Pos tp = SkelTiles::pos(tiles_x, tiles_y);
  const long img = tp.img;
  const int y0 = tp.y0, x0 = tp.x0;
  // the next launch sets this slot; nothing reads or sets it in this launch
  if (tp.tile == 0 && threadIdx.x == 0) next[img] = 0;
  if (prev && __hip_atomic_load(prev + img, SKEL_RLX_AGENT) == 0) return;  // converged: both maps hold the result
  const long base = img * H * W;
  const bool words = W % 4 == 0;  // then every row starts on a word of the map, and a word is inside the image or outside
  for (int i = threadIdx.x; i < kLdsWords; i += 256) S0[i] = 0, S1[i] = 0;
  if (threadIdx.x < kK) chg[threadIdx.x] = 0;
  __syncthreads();
  unsigned any = 0;
  if (words) {
    for (int g = threadIdx.x; g < kGroupsX * kRH; g += 256) {
      const int ry = g / kGroupsX, gx = g - ry * kGroupsX;
      const int y = y0 + ry - kHalo, x = x0 + gx * 4 - kHalo;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(src + base + (long)y * W + x);
        S0[group_word(ry, gx)] = v;
        any |= v;
      }
    }
  } else {
    uint8_t* b0 = reinterpret_cast<uint8_t*>(S0);
    for (int i = threadIdx.x; i < kRW * kRH; i += 256) {
      const int ry = i / kRW, rx = i - ry * kRW;
      const int y = y0 + ry - kHalo, x = x0 + rx - kHalo;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const uint8_t v = src[base + (long)y * W + x];
        b0[(ry + 1) * kPitch + 4 + rx] = v;
        any |= v;
      }
    }
  }
  unsigned inner_any = 0, inner_last = 0;
  if (__syncthreads_or(any != 0)) {
    // ends: at most `passes` <= kK turns
    for (int p = 0; p < passes; ++p) {
      for (int g = threadIdx.x; g < kGroupsX * kRH; g += 256) {
        const int w = group_word(g / kGroupsX, g % kGroupsX);
        S1[w] = thin_word(S0, w, 0);
      }
      __syncthreads();
      // S0 <- the second subiteration of S1.  A thread touches no word of S0 but its own, and what the pass
      // deleted is where that word changes: a pixel the first subiteration deleted is zero in S1 and stays so
      unsigned c = 0;
      for (int g = threadIdx.x; g < kGroupsX * kRH; g += 256) {
        const int ry = g / kGroupsX, gx = g - ry * kGroupsX;
        const int w = group_word(ry, gx);
        const uint32_t r = thin_word(S1, w, 1);
        if (r != S0[w]) {
          const bool inner = ry >= kHalo && ry < kHalo + kTH && gx >= kHalo / 4 && gx < (kHalo + kTW) / 4;
          c |= inner ? 3u : 1u;
          S0[w] = r;
        }
      }
      if (c) atomicOr(&chg[p], c);
      __syncthreads();
      const unsigned all = chg[p];  // bit 0: a pixel of the region was deleted, bit 1: one of the tile
      inner_any |= all & 2u;
      inner_last = p == passes - 1 ? (all & 2u) : 0u;
      if (!(all & 1u)) break;  // nothing deleted in the whole region: no later pass deletes either
    }
  }
  // the tile, from S0 (every pass ends there)
  if (words) {
    for (int g = threadIdx.x; g < (kTW / 4) * kTH; g += 256) {
      const int ry = g / (kTW / 4), gx = g - ry * (kTW / 4);
      const int y = y0 + ry, x = x0 + gx * 4;
      if (y < H && x < W)
        *reinterpret_cast<uint32_t*>(dst + base + (long)y * W + x) = S0[group_word(ry + kHalo, gx + kHalo / 4)];
    }
  } else {
    const uint8_t* b0 = reinterpret_cast<const uint8_t*>(S0);
    for (int i = threadIdx.x; i < kTW * kTH; i += 256) {
      const int ry = i / kTW, rx = i - ry * kTW;
      const int y = y0 + ry, x = x0 + rx;
      if (y < H && x < W) dst[base + (long)y * W + x] = b0[(ry + kHalo + 1) * kPitch + 4 + kHalo + rx];
    }
  }
  if (threadIdx.x == 0) {
    if (inner_any) __hip_atomic_fetch_or(cur + img, 1, SKEL_RLX_AGENT);
    if (last && inner_last) __hip_atomic_fetch_or(last + img, 1, SKEL_RLX_AGENT);
  }
}

// ---- pair counts ------------------------------------------------------------------------------------
// out[0..3] += the four pixel counts of the head of unetseg_hip.h's section; block 0 adds out[4] and out[5]
__global__ __launch_bounds__(256) void skel_counts_kernel(const int* pred, const int* target, const int* sp,
                                                          const int* st, const int* up, const int* ut, long total,
                                                          int N, int c, int ignore, unsigned long long* out) {
  __shared__ unsigned acc[5];
  const bool has_ign = ignore != -1;
  if (threadIdx.x < 5) acc[threadIdx.x] = 0;
  __syncthreads();
  unsigned v[5] = {0, 0, 0, 0, 0};
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const int t = target[it];
    if (has_ign && t == ignore) continue;
    const bool a = sp[it] == c, b = st[it] == c;
    v[0] += a && t == c;
    v[1] += a;
    v[2] += b && pred[it] == c;
    v[3] += b;
  }
  if (blockIdx.x == 0)
    for (int n = threadIdx.x; n < N; n += 256) v[4] += (up[n] | ut[n]) != 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    unsigned s = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(acc + k, s);
  }
  __syncthreads();
  if (threadIdx.x < 5 && acc[threadIdx.x]) atomicAdd(out + threadIdx.x, (unsigned long long)acc[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 5) atomicAdd(out + 5, (unsigned long long)N);
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// host only: the seams of the thinning lie at the multiples of *tw and *th; one launch runs *passes_per_launch passes
UNETSEG_API int unetseg_skel_tile(int* tw, int* th, int* passes_per_launch) {
  US_CHECK_ARG(tw && th && passes_per_launch, "skel_tile: null pointer");
  *tw = kTW, *th = kTH, *passes_per_launch = kK;
  return 0;
}

// host only; 0 for a shape it refuses
UNETSEG_API size_t unetseg_skel_workspace(int N, int H, int W) {
  if (!SkelTiles::shape_ok(N, H, W)) return 0;
  return SkelLayout((size_t)N * H * W, N).bytes;
}

// out int32 [N][H][W] = cls with the pixels that thinning deletes set to 0 (see the head of this file);
// unconverged int32 [N] (may be NULL)
UNETSEG_API int unetseg_skel_thin(const int32_t* cls, int N, int H, int W, int max_passes, int32_t* out,
                                  int32_t* unconverged, void* ws, size_t ws_bytes, void* stream) {
  US_CHECK_ARG(cls && out && ws, "skel_thin: null pointer");  // unconverged may be NULL
  US_CHECK_ARG(SkelTiles::shape_ok(N, H, W), "skel_thin: bad shape N=%d H=%d W=%d", N, H, W);
  US_CHECK_ARG(max_passes >= 0, "skel_thin: max_passes %d must not be negative", max_passes);
  US_CHECK_ARG(ws_bytes >= unetseg_skel_workspace(N, H, W), "skel_thin: workspace too small");
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, "skel_thin: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)N * H * W;
  const SkelLayout lay((size_t)total, N);
  uint8_t* maps[2] = {(uint8_t*)ws, (uint8_t*)ws + lay.map};
  int* flags = (int*)((uint8_t*)ws + lay.flags);
  int* last = flags + 3 * (size_t)N;
  const int G = grid_for((total + 3) / 4, 4096);
  hipLaunchKernelGGL(skel_pack_kernel, dim3(G), dim3(256), 0, st, cls, total, (uint32_t*)maps[0], flags, 4 * N);
  const SkelTiles t(N, H, W);
  const int launches = max_passes / kK + (max_passes % kK != 0);
  for (int l = 0; l < launches; ++l) {
    const bool fin = l == launches - 1;
    const int passes = fin ? max_passes - l * kK : kK;
    hipLaunchKernelGGL(skel_thin_kernel, dim3((unsigned)t.blocks), dim3(256), 0, st, (const uint8_t*)maps[l & 1],
                       maps[(l + 1) & 1], H, W, t.tx, t.ty, passes,
                       l == 0 ? (const int*)nullptr : flags + (size_t)((l + 2) % 3) * N, flags + (size_t)(l % 3) * N,
                       flags + (size_t)((l + 1) % 3) * N, fin ? last : (int*)nullptr);
  }
  hipLaunchKernelGGL(skel_finish_kernel, dim3(G), dim3(256), 0, st, cls, (const uint32_t*)maps[launches & 1], total, out,
                     launches ? (const int*)last : (const int*)nullptr, N, unconverged);
  US_LAUNCH_CHECK("skel_thin");
  return 0;
}

// out int64 [6] += {#(skel_pred == c & target == c), #(skel_pred == c), #(skel_target == c & pred == c),
// #(skel_target == c), sum over n of (unconv_pred[n] | unconv_target[n]), N}; the pixels whose target is
// `ignore` (-1: none) are skipped
UNETSEG_API int unetseg_skel_counts(const int32_t* pred, const int32_t* target, const int32_t* skel_pred,
                                    const int32_t* skel_target, const int32_t* unconv_pred,
                                    const int32_t* unconv_target, int N, int H, int W, int c, int ignore, int64_t* out,
                                    void* stream) {
  US_CHECK_ARG(pred && target && skel_pred && skel_target && unconv_pred && unconv_target && out,
               "skel_counts: null pointer");
  US_CHECK_ARG(SkelTiles::shape_ok(N, H, W), "skel_counts: bad shape N=%d H=%d W=%d", N, H, W);
  US_CHECK_ARG(c >= 1 && c <= kMaxClass, "skel_counts: class %d outside 1 .. %d", c, kMaxClass);
  US_CHECK_ARG(ignore != c, "skel_counts: ignore is the counted class %d", c);
  const long total = (long)N * H * W;  // <= 2^40: a block's 32-bit counters hold its share (1024 blocks)
  hipLaunchKernelGGL(skel_counts_kernel, dim3(grid_for(total, 1024)), dim3(256), 0, (hipStream_t)stream, pred, target,
                     skel_pred, skel_target, unconv_pred, unconv_target, total, N, c, ignore, (unsigned long long*)out);
  US_LAUNCH_CHECK("skel_counts");
  return 0;
}
