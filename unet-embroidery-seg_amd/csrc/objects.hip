// Object-level agreement of two class maps (unetseg_hip/objects.py: Panoptic Quality, object F1, split and
// merge counts of val.py and of the evaluate loops; no reference counterpart).
//
// Semantics.  pred, target int32 [N][H][W] (the caller has set the ignored pixels to 0 in both).  Both are
// labelled with unetseg_ccl_label at `connectivity` and measured with unetseg_ccl_stats.  For a class c in
// 1 .. 255 an object is a component of class c; a predicted object p and a target object g (named by their
// roots) overlap when some pixel has pred == c, target == c, root_pred == p and root_target == g; inter(p, g)
// counts those pixels and union = area_p + area_g - inter.  out int64 [20] += the counts listed in
// include/unetseg_hip.h: objects, objects with a partner, splits and merges, the pairs with IoU > k / 20
// decided as 20 inter > k union in 64-bit integers, and sum floor(inter 2^32 / union) over the pairs with
// IoU > 1/2.  IoU > 1/2 is strict, so such pairs are a matching already (Kirillov et al., Panoptic
// Segmentation, CVPR 2019, section 4.1) and no assignment step exists.
//
// Pair table.  One open-addressing table per image: u64 key (root_pred << 32) | root_target claimed with a
// 64-bit compare-and-swap (all ones = empty), u32 count added with integer atomics.  Its capacity is the
// smallest power of two >= max(H W, 2), and it is never more than about half full:
//   - two edge-adjacent overlap pixels (pred == c and target == c at both) have equal class in both maps, so
//     they are joined in both labellings, under either connectivity;
//   - hence the pair (root_pred, root_target) is constant on every 4-connected component of the overlap set,
//     and the number of distinct pairs is at most the number of those components;
//   - pick one pixel per component: no two picks are edge neighbours, and a set of pixels without two edge
//     neighbours has at most ceil(H W / 2) members (one per domino of a domino tiling, plus the odd pixel).
// The probe loop is bounded by the capacity all the same; an insertion that finds no slot adds to a word that
// lands in out[18] and drops its pixels, so a bug is a message and never a spinning kernel.  No result depends
// on the hash or on the order of the slots: the counts are sums over the occupied slots.
//
// Launches, all on the caller's stream, none waits on the host, their number fixed by the shape:
//   label: unetseg_ccl_label and unetseg_ccl_stats for each map, into the workspace.
//   pairs: two memsets (keys to all ones; counts and the failure word to 0) and the pair kernel.  A block owns
//     a tile of kPW x kPH pixels; a wave takes a 64-pixel row segment with coalesced loads of the two class maps
//     and the two root maps.  A lane is a run head where its pair differs from the lane before it (one wave
//     shuffle); only run heads insert, and they insert the run length, so a large object costs one atomic per
//     row segment and not one per pixel on one address.  Run heads first meet in an LDS table of kSlots slots
//     (linear probing, LDS integer atomics); the block then makes one global insertion per distinct pair.  A run
//     that finds no LDS slot within kLdsProbes probes goes to the global table itself.
//   match: one memset (the degree planes) and two kernels.  The match kernel has one thread per table slot: for
//     an occupied slot it reads the two areas at the roots, makes the ten comparisons and the fixed-point term
//     and adds 1 to the int32 degree planes at the two roots.  The count kernel runs over the pixels: at the
//     root positions of class c it counts objects and objects of degree >= 1 and >= 2.  Both reduce in the
//     block before one u64 atomic per counter per block.
// Everything is integer, every atomic is relaxed and agent scope (workgroup scope in LDS), and the result is
// bitwise reproducible.
#include "seg_pixel.h"

UNETSEG_API int unetseg_ccl_label(const int32_t* cls, int N, int H, int W, int connectivity, int32_t* root,
                                  void* stream);
UNETSEG_API int unetseg_ccl_stats(const int32_t* root, int N, int H, int W, int32_t* stats, void* stream);

namespace {

constexpr int kPW = 64;         // pair tile width: one wave64 per row segment
constexpr int kPH = 32;         // pair tile height: 8 rows per wave
constexpr int kSlotBits = 9;
constexpr int kSlots = 1 << kSlotBits;  // LDS table of a block: 6 KB
constexpr int kLdsProbes = 16;  // then the run goes to the global table
constexpr int kMaxClass = 255;
constexpr unsigned long long kEmpty = ~0ull;  // no key: a root is < 2^31

#define OBJ_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define OBJ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

using PairTiles = TileGrid<kPW, kPH>;

// the smallest power of two >= max(hw, 2), as its exponent; hw <= 2^31 - 1
inline int cap_log2(long hw) {
  int b = 1;
  while ((1L << b) < hw) ++b;
  return b;
}

// the workspace: roots int32 [2][T] | stats int32 [2][4][T] | keys u64 [N][cap] | counts u32 [N][cap], then
// the failure word | degrees int32 [2][T], with T = N H W and pred before target; each part rounded up to 256
struct ObjLayout {
  size_t total, cap, root, stats, keys, vals, fail, deg, bytes;
  size_t keys_bytes, vals_bytes, deg_bytes;
  int cap_bits;
  ObjLayout(int N, int H, int W) {
    total = (size_t)N * H * W;
    cap_bits = cap_log2((long)H * W);
    cap = (size_t)1 << cap_bits;
    root = 0;
    stats = root + up256(2 * total * 4);
    keys = stats + up256(8 * total * 4);
    keys_bytes = (size_t)N * cap * 8;
    vals = keys + up256(keys_bytes);
    fail = vals + (size_t)N * cap * 4;
    vals_bytes = (size_t)N * cap * 4 + 4;
    deg = vals + up256(vals_bytes);
    deg_bytes = 2 * total * 4;
    bytes = deg + up256(deg_bytes);
  }
};

__device__ __forceinline__ unsigned slot_of(unsigned long long key, int bits) {
  return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> (64 - bits));  // 1 <= bits <= 31
}

// count more pixels of the pair `key` in one image's table of 2^bits slots
__device__ __forceinline__ void table_add(unsigned long long* keys, unsigned* vals, int bits, unsigned long long key,
                                          unsigned count, unsigned* fail) {
  const unsigned mask = (1u << bits) - 1u;
  unsigned s = slot_of(key, bits);
  // ends: at most 2^bits turns
  for (unsigned probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
    unsigned long long k = __hip_atomic_load(keys + s, OBJ_RLX_AGENT);
    if (k == kEmpty) {
      unsigned long long expect = kEmpty;
      k = __hip_atomic_compare_exchange_strong(keys + s, &expect, key, __ATOMIC_RELAXED, OBJ_RLX_AGENT) ? key : expect;
    }
    if (k == key) {
      __hip_atomic_fetch_add(vals + s, count, OBJ_RLX_AGENT);
      return;
    }
  }
  __hip_atomic_fetch_add(fail, 1u, OBJ_RLX_AGENT);
}

// block = one tile of one image; wave w holds rows w, w + 4, ... of the tile, lane = column.  AGG: the runs of
// the block meet in LDS first
template <bool AGG>
__global__ __launch_bounds__(256) void obj_pair_kernel(const int* pred, const int* target, const int* root_p,
                                                       const int* root_t, int H, int W, int c, int tiles_x,
                                                       int tiles_y, int bits, unsigned long long* keys,
                                                       unsigned* vals, unsigned* fail) {
  __shared__ unsigned long long lkey[AGG ? kSlots : 1];
  __shared__ unsigned lcnt[AGG ? kSlots : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PairTiles::Pos tp = PairTiles::pos(tiles_x, tiles_y);
  const long base = tp.img * ((long)H * W);
  unsigned long long* tk = keys + ((size_t)tp.img << bits);
  unsigned* tv = vals + ((size_t)tp.img << bits);
  if (AGG) {
    for (int s = threadIdx.x; s < kSlots; s += 256) lkey[s] = kEmpty, lcnt[s] = 0;
    __syncthreads();
  }
  const int rows = H - tp.y0 < kPH ? H - tp.y0 : kPH;  // rows of the tile inside the image (>= 1)
  const int x = tp.x0 + lane;
  const bool in = x < W;  // lane 0 always is
  for (int r = wave; r < rows; r += 4) {
    unsigned long long key = kEmpty;
    if (in) {
      const long i = base + (long)(tp.y0 + r) * W + x;
      if (pred[i] == c && target[i] == c) key = (unsigned long long)(unsigned)root_p[i] << 32 | (unsigned)root_t[i];
    }
    const unsigned long long left = __shfl_up(key, 1, 64);
    // a lane outside the overlap starts a run of no key: it ends the run before it
    const bool start = lane == 0 || left != key;
    const unsigned long long starts = __ballot(start);
    if (start && key != kEmpty) {
      const unsigned long long later = lane == 63 ? 0ull : starts & (~0ull << (lane + 1));
      const unsigned len = (unsigned)((later ? __ffsll((long long)later) - 1 : 64) - lane);
      bool placed = false;
      if (AGG) {
        unsigned s = slot_of(key, kSlotBits);
        // ends: at most kLdsProbes turns
        for (int probe = 0; probe < kLdsProbes && !placed; ++probe, s = (s + 1) & (kSlots - 1)) {
          unsigned long long k = __hip_atomic_load(lkey + s, OBJ_RLX_WG);
          if (k == kEmpty) {
            unsigned long long expect = kEmpty;
            k = __hip_atomic_compare_exchange_strong(lkey + s, &expect, key, __ATOMIC_RELAXED, OBJ_RLX_WG) ? key : expect;
          }
          if (k == key) {
            __hip_atomic_fetch_add(lcnt + s, len, OBJ_RLX_WG);
            placed = true;
          }
        }
      }
      if (!placed) table_add(tk, tv, bits, key, len, fail);
    }
  }
  if (AGG) {
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots; s += 256)
      if (lkey[s] != kEmpty) table_add(tk, tv, bits, lkey[s], lcnt[s], fail);
  }
}

// a block's counters v[0 .. K) summed over its 256 threads and added to out[at[k]]: one u64 atomic per
// non-zero counter and block.  acc: K words of LDS, zero on entry for every thread (a barrier lies behind)
template <int K>
__device__ __forceinline__ void block_add(unsigned long long (&v)[K], unsigned long long* acc,
                                          unsigned long long* out, const int* at) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    unsigned long long s = v[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) __hip_atomic_fetch_add(acc + k, s, OBJ_RLX_WG);
  }
  __syncthreads();
  if (threadIdx.x < K && acc[threadIdx.x]) __hip_atomic_fetch_add(out + at[threadIdx.x], acc[threadIdx.x], OBJ_RLX_AGENT);
}

// thread = one slot of one image's table.  area_p / area_t: the area planes of the two stats, deg_p / deg_t:
// the degree planes, all [N][H][W]
__global__ __launch_bounds__(256) void obj_match_kernel(const unsigned long long* keys, const unsigned* vals, int bits,
                                                        long slots, long HW, const int* area_p, const int* area_t,
                                                        int* deg_p, int* deg_t, unsigned long long* out) {
  __shared__ unsigned long long acc[12];
  __shared__ int at[12];
  if (threadIdx.x < 12) {
    acc[threadIdx.x] = 0;
    at[threadIdx.x] = threadIdx.x < 10 ? 6 + threadIdx.x : threadIdx.x == 10 ? 16 : 17;
  }
  __syncthreads();
  unsigned long long v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long it = blockIdx.x * 256L + threadIdx.x; it < slots; it += gridDim.x * 256L) {
    const unsigned long long key = keys[it];
    if (key == kEmpty) continue;
    const long at_p = (it >> bits) * HW + (long)(key >> 32), at_t = (it >> bits) * HW + (long)(key & 0xFFFFFFFFull);
    const unsigned long long inter = vals[it];
    const unsigned long long uni = (unsigned long long)area_p[at_p] + (unsigned long long)area_t[at_t] - inter;
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] += 20ull * inter > (unsigned long long)(10 + k) * uni;
    if (2ull * inter > uni) v[10] += (inter << 32) / uni;  // inter < 2^31; uni >= inter >= 1
    v[11] += 1;
    __hip_atomic_fetch_add(deg_p + at_p, 1, OBJ_RLX_AGENT);
    __hip_atomic_fetch_add(deg_t + at_t, 1, OBJ_RLX_AGENT);
  }
  block_add(v, acc, out, at);
}

// thread = one pixel.  out[0 .. 5] += the objects of class c of target / pred, those of degree >= 1 and
// those of degree >= 2; block 0 adds the failure word to out[18] and N to out[19]
__global__ __launch_bounds__(256) void obj_count_kernel(const int* pred, const int* target, const int* root_p,
                                                        const int* root_t, const int* deg_p, const int* deg_t,
                                                        long total, long HW, int N, int c, const unsigned* fail,
                                                        unsigned long long* out) {
  __shared__ unsigned long long acc[6];
  __shared__ int at[6];
  if (threadIdx.x < 6) acc[threadIdx.x] = 0, at[threadIdx.x] = threadIdx.x;
  __syncthreads();
  unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
  for (long it = blockIdx.x * 256L + threadIdx.x; it < total; it += gridDim.x * 256L) {
    const int idx = (int)(it % HW);
    if (target[it] == c && root_t[it] == idx) {
      const int d = deg_t[it];
      v[0] += 1, v[2] += d >= 1, v[4] += d >= 2;
    }
    if (pred[it] == c && root_p[it] == idx) {
      const int d = deg_p[it];
      v[1] += 1, v[3] += d >= 1, v[5] += d >= 2;
    }
  }
  block_add(v, acc, out, at);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (*fail) __hip_atomic_fetch_add(out + 18, (unsigned long long)*fail, OBJ_RLX_AGENT);
    __hip_atomic_fetch_add(out + 19, (unsigned long long)N, OBJ_RLX_AGENT);
  }
}

// the checks shared by the entry points: 0; 1 with the message set; -1 for an empty batch (nothing to do)
int obj_geometry(const char* name, int N, int H, int W, const void* ws, size_t ws_bytes) {
  US_CHECK_ARG(N >= 0 && H >= 0 && W >= 0, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
  if (N == 0 || H == 0 || W == 0) return -1;
  US_CHECK_ARG((long)H * W <= INT32_MAX, "%s: H * W = %d * %d exceeds the 2^31 - 1 pixels of one image", name, H, W);
  US_CHECK_ARG(PairTiles::shape_ok(N, H, W), "%s: shape N=%d H=%d W=%d is too large", name, N, H, W);
  US_CHECK_ARG(ws, "%s: null workspace", name);
  US_CHECK_ARG(ws_bytes >= ObjLayout(N, H, W).bytes, "%s: workspace too small", name);
  US_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", name);
  return 0;
}

#define OBJ_GEOMETRY(name)                                               \
  do {                                                                   \
    const int g_ = obj_geometry(name, N, H, W, ws, ws_bytes);            \
    if (g_ != 0) return g_ < 0 ? 0 : 1;                                  \
  } while (0)

#define OBJ_CHECK_CLASS(name) US_CHECK_ARG(c >= 1 && c <= kMaxClass, "%s: class %d outside 1 .. %d", name, c, kMaxClass)

#define OBJ_HIP(name, call)                                                          \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) {                                                          \
      unetseg_set_error("%s: %s failed: %s", name, #call, hipGetErrorString(e_));    \
      return 2;                                                                      \
    }                                                                                \
  } while (0)

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================

// the tile of the pair kernel (host only): a block's LDS table gathers the runs of *tw x *th pixels
UNETSEG_API int unetseg_objects_tile(int* tw, int* th) {
  US_CHECK_ARG(tw && th, "objects_tile: null pointer");
  *tw = kPW, *th = kPH;
  return 0;
}

// host only; 0 for a shape the entry points refuse and for an empty batch
UNETSEG_API size_t unetseg_objects_workspace(int N, int H, int W) {
  if (!PairTiles::shape_ok(N, H, W) || (long)H * W > INT32_MAX) return 0;
  return ObjLayout(N, H, W).bytes;
}

// host only: at[0 .. 5) = the byte offsets in the workspace of roots int32 [2][N][H][W], stats int32
// [2][4][N][H][W], keys u64 [N][cap] (all ones = empty), counts u32 [N][cap] and degrees int32 [2][N][H][W]
// (pred before target); at[5] = cap
UNETSEG_API int unetseg_objects_layout(int N, int H, int W, int64_t* at) {
  US_CHECK_ARG(at, "objects_layout: null pointer");
  US_CHECK_ARG(unetseg_objects_workspace(N, H, W) != 0, "objects_layout: bad shape N=%d H=%d W=%d", N, H, W);
  const ObjLayout lay(N, H, W);
  at[0] = (int64_t)lay.root, at[1] = (int64_t)lay.stats, at[2] = (int64_t)lay.keys, at[3] = (int64_t)lay.vals;
  at[4] = (int64_t)lay.deg, at[5] = (int64_t)lay.cap;
  return 0;
}

// the workspace's roots and stats of pred and target (four calls of the ccl entry points)
UNETSEG_API int unetseg_objects_label(const int32_t* pred, const int32_t* target, int N, int H, int W,
                                      int connectivity, void* ws, size_t ws_bytes, void* stream) {
  US_CHECK_ARG(pred && target, "objects_label: null pointer");
  US_CHECK_ARG(connectivity == 4 || connectivity == 8, "objects_label: connectivity %d is neither 4 nor 8",
               connectivity);
  OBJ_GEOMETRY("objects_label");
  const ObjLayout lay(N, H, W);
  int32_t* root = (int32_t*)((uint8_t*)ws + lay.root);
  int32_t* stats = (int32_t*)((uint8_t*)ws + lay.stats);
  const int32_t* maps[2] = {pred, target};
  for (int k = 0; k < 2; ++k) {
    if (int rc = unetseg_ccl_label(maps[k], N, H, W, connectivity, root + k * lay.total, stream)) return rc;
    if (int rc = unetseg_ccl_stats(root + k * lay.total, N, H, W, stats + 4 * k * lay.total, stream)) return rc;
  }
  return 0;
}

// the workspace's pair table of class c from its roots (unetseg_objects_label on the same maps); aggregate
// != 0: the block's runs meet in LDS first (the product path), 0: every run goes to the global table
UNETSEG_API int unetseg_objects_pairs(const int32_t* pred, const int32_t* target, int N, int H, int W, int c,
                                      int aggregate, void* ws, size_t ws_bytes, void* stream) {
  US_CHECK_ARG(pred && target, "objects_pairs: null pointer");
  OBJ_CHECK_CLASS("objects_pairs");
  OBJ_GEOMETRY("objects_pairs");
  const ObjLayout lay(N, H, W);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  const int* root = (const int*)(w + lay.root);
  unsigned long long* keys = (unsigned long long*)(w + lay.keys);
  unsigned* vals = (unsigned*)(w + lay.vals);
  OBJ_HIP("objects_pairs", hipMemsetAsync(keys, 0xFF, lay.keys_bytes, st));
  OBJ_HIP("objects_pairs", hipMemsetAsync(vals, 0, lay.vals_bytes, st));
  const PairTiles t(N, H, W);
  if (aggregate)
    hipLaunchKernelGGL(obj_pair_kernel<true>, dim3((unsigned)t.blocks), dim3(256), 0, st, pred, target, root,
                       root + lay.total, H, W, c, t.tx, t.ty, lay.cap_bits, keys, vals, (unsigned*)(w + lay.fail));
  else
    hipLaunchKernelGGL(obj_pair_kernel<false>, dim3((unsigned)t.blocks), dim3(256), 0, st, pred, target, root,
                       root + lay.total, H, W, c, t.tx, t.ty, lay.cap_bits, keys, vals, (unsigned*)(w + lay.fail));
  US_LAUNCH_CHECK("objects_pairs");
  return 0;
}

// out int64 [20] += the counts of class c from the workspace's table (unetseg_objects_pairs for c), roots and
// stats
UNETSEG_API int unetseg_objects_match(const int32_t* pred, const int32_t* target, int N, int H, int W, int c,
                                      int64_t* out, void* ws, size_t ws_bytes, void* stream) {
  US_CHECK_ARG(pred && target && out, "objects_match: null pointer");
  OBJ_CHECK_CLASS("objects_match");
  OBJ_GEOMETRY("objects_match");
  const ObjLayout lay(N, H, W);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* w = (uint8_t*)ws;
  const int* root = (const int*)(w + lay.root);
  const int* stats = (const int*)(w + lay.stats);
  int* deg = (int*)(w + lay.deg);
  OBJ_HIP("objects_match", hipMemsetAsync(deg, 0, lay.deg_bytes, st));
  const long slots = (long)(lay.cap * (size_t)N), HW = (long)H * W, total = (long)lay.total;
  // at most 2^40 slots or pixels: a thread's counters stay far below 2^64
  hipLaunchKernelGGL(obj_match_kernel, dim3(grid_for(slots, 4096)), dim3(256), 0, st,
                     (const unsigned long long*)(w + lay.keys), (const unsigned*)(w + lay.vals), lay.cap_bits, slots, HW,
                     stats, stats + 4 * lay.total, deg, deg + lay.total, (unsigned long long*)out);
  hipLaunchKernelGGL(obj_count_kernel, dim3(grid_for(total, 4096)), dim3(256), 0, st, pred, target, root,
                     root + lay.total, (const int*)deg, (const int*)(deg + lay.total), total, HW, N, c,
                     (const unsigned*)(w + lay.fail), (unsigned long long*)out);
  US_LAUNCH_CHECK("objects_match");
  return 0;
}
