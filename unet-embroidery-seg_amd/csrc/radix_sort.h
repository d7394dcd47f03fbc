// Segmented, stable LSD radix sort (4 x 8-bit passes) on 32-bit keys with a 32-bit value word, shared
// by the Lovasz hinge (loss.hip) and the Lovasz-softmax (lovasz_softmax.hip).  grid.y is the segment:
// S segments of P keys each, contiguous in memory.  The keys order floats descending; ties keep
// their input order (the reference's torch.sort is not stable, so only the loss VALUE is
// tie-order independent).  The value word carries the element's index in bits 0..30 and its 0/1
// label in bit 31; lovasz_count_kernel counts the labels per 4096-key chunk of the sorted order.
#pragma once
#include "common.h"

namespace {

constexpr int kTile = 4096;  // keys per radix tile (256 threads x 16)

__device__ __forceinline__ uint32_t desc_key(float f) {
  uint32_t u = __float_as_uint(f);
  uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
  uint32_t asc = ~k;
  uint32_t u = (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
  return __uint_as_float(u);
}

__global__ void radix_hist_kernel(const uint32_t* keys, long P, int T, int shift, uint32_t* hist) {
  __shared__ uint32_t h[256];
  const int t = blockIdx.x, b = blockIdx.y;
  h[threadIdx.x] = 0;
  __syncthreads();
  const long base = (long)b * P + (long)t * kTile;
  const long n = min((long)kTile, P - (long)t * kTile);
  for (long i = threadIdx.x; i < n; i += 256) atomicAdd(&h[(keys[base + i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[((long)b * 256 + threadIdx.x) * T + t] = h[threadIdx.x];
}

// exclusive scan of hist[b][256*T] (digit-major) in place; one 1024-thread block per segment.  Each
// thread owns a contiguous run of the segment, loaded once into registers; the runs' totals are
// scanned with wave shuffles and one LDS exchange of the 16 wave totals.
constexpr int kScanPer = 32;  // entries per thread held in registers (up to 128 tiles = 524288 pixels per image)
__global__ __launch_bounds__(1024) void radix_scan_kernel(uint32_t* hist, int T) {
  __shared__ uint32_t wsum[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t* h = hist + (long)b * 256 * T;
  const long n = 256L * T;
  const long per = (n + 1023) / 1024;
  const long lo = tid * per, hi = min(n, lo + per);
  const bool regs = per <= kScanPer;  // else (more than 524288 pixels per image) two passes over memory
  uint32_t v[kScanPer];
  uint32_t s = 0;
  if (regs) {
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      v[i] = (i < per && lo + i < hi) ? h[lo + i] : 0u;
      s += v[i];
    }
  } else {
    for (long i = lo; i < hi; ++i) s += h[i];
  }
  // inclusive scan of the per-thread totals within the wave, then across the 16 waves
  uint32_t x = s;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  uint32_t run = x - s;
  for (int w = 0; w < wid; ++w) run += wsum[w];
  if (regs) {
#pragma unroll
    for (int i = 0; i < kScanPer; ++i) {
      if (i < per && lo + i < hi) h[lo + i] = run;
      run += v[i];
    }
  } else {
    for (long i = lo; i < hi; ++i) {
      const uint32_t c = h[i];
      h[i] = run;
      run += c;
    }
  }
}

// stable scatter.  The tile is ranked in 16 rounds of 256 keys (original order = round-major) into LDS
// in digit order, then written out from LDS: consecutive slots of one digit go to consecutive global
// positions, so the writes leave as runs (~16 keys per digit and tile) instead of one scattered 4-B
// store per key.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
                                                            uint32_t* vout, long P, int T, int shift,
                                                            const uint32_t* hist) {
  __shared__ uint32_t gbase[256];  // global position of this tile's first key of each digit
  __shared__ uint32_t lstart[256];  // tile-local first slot of each digit
  __shared__ uint32_t run[256];     // keys of each digit placed so far
  __shared__ uint32_t wcnt[4][256];
  __shared__ uint32_t sk[kTile], sv[kTile];
  const int t = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t* hb = hist + (long)b * 256 * T;
  const long seg = (long)b * P;
  const long tbase = (long)t * kTile;
  const long n = min((long)kTile, P - tbase);
  // this tile's count of digit `tid`: the next entry of the digit-major exclusive scan minus this one
  const long hi = (long)tid * T + t;
  const uint32_t g0 = hb[hi];
  const uint32_t cnt = (hi + 1 < 256L * T ? hb[hi + 1] : (uint32_t)P) - g0;
  gbase[tid] = g0;
  // exclusive scan of the 256 counts (wave prefix sums, then the four wave totals)
  uint32_t x = cnt;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wcnt[0][wid] = x;
  __syncthreads();
  uint32_t off = 0;
  for (int w = 0; w < wid; ++w) off += wcnt[0][w];
  lstart[tid] = off + x - cnt;
  run[tid] = 0;
  __syncthreads();
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  for (int round = 0; round < kTile / 256; ++round) {
    const long i = round * 256L + tid;
    const bool ok = i < n;
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    uint32_t key = 0, val = 0, d = 0;
    if (ok) {
      key = kin[seg + tbase + i];
      val = vin[seg + tbase + i];
      d = (key >> shift) & 255u;
    }
    unsigned long long m = __ballot(ok);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long bal = __ballot(ok && ((d >> bit) & 1u));
      m &= ((d >> bit) & 1u) ? bal : ~bal;
    }
    const int lrank = __popcll(m & lt_mask);
    if (ok && lrank == 0) wcnt[wid][d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (ok) {
      uint32_t pos = lstart[d] + run[d] + lrank;
      for (int w = 0; w < wid; ++w) pos += wcnt[w][d];
      sk[pos] = key;
      sv[pos] = val;
    }
    __syncthreads();
    run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
  }
  __syncthreads();
  for (int j = tid; j < n; j += 256) {
    const uint32_t key = sk[j];
    const uint32_t d = (key >> shift) & 255u;
    const uint32_t pos = gbase[d] + (uint32_t)j - lstart[d];
    kout[seg + pos] = key;
    vout[seg + pos] = sv[j];
  }
}

// positives per (image, 4096-key chunk) of the sorted order
__global__ void lovasz_count_kernel(const uint32_t* vals, long P, int T, uint32_t* cnt) {
  __shared__ uint32_t sc[4];
  const int t = blockIdx.x, b = blockIdx.y;
  const long lo = (long)t * kTile, hi = min(P, lo + kTile);
  const uint32_t* v = vals + (long)b * P;
  uint32_t c = 0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) c += v[i] >> 31;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(long)b * T + t] = sc[0] + sc[1] + sc[2] + sc[3];
}

}  // namespace
