// Bilinear x2 upsample forward and its adjoints, NHWC (layout and element types as bn.hip).
//
// Reference ops replaced:
//   Upsample x2      model/unet_resnet.py:21,71 (align_corners=True)  model/unet_plain.py:36 (False)
#include <algorithm>

#include "elem_util.h"

namespace {

// ------------------------------------------------------------------------------------------
// Bilinear x2 upsample, NHWC (source index / weight: up_src, the blend: up_blend in common.h).
// ------------------------------------------------------------------------------------------

// Row-blocked: a block covers (pixel, 8-channel) lanes of whole output rows, kRowsPB rows in turn,
// so the per-row source index and weight are wave-uniform and the per-column ones are computed
// once per lane (the flat form spent its time in 64-bit index division).
constexpr int kUpRowsPB = 4;
// rows per block actually launched (UNETSEG_UP_ROWS = 2 or 8 overrides kUpRowsPB: experiments only;
// latched on first use)
static int up_rows_pb() {
  static const int r = [] {
    const char* e = getenv("UNETSEG_UP_ROWS");
    const int v = e ? atoi(e) : 0;
    return v == 2 || v == 8 ? v : kUpRowsPB;
  }();
  return r;
}

template <typename T>
__global__ void upsample_fwd_kernel(const T* x, int ldx, int N, int H, int W, int C, int align, T* y, int ldy,
                                    int rows_pb) {
  constexpr int V = VE<T>;
  const int cv = C / V, OH = 2 * H, OW = 2 * W;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= OW * cv) return;
  const int ow = idx / cv, c0 = (idx - ow * cv) * V;
  int w0, w1;
  float lw;
  up_src(ow, W, OW, align, w0, w1, lw);
  const float wl0 = 1.f - lw;
  const int r0 = blockIdx.y * rows_pb, r1 = min(r0 + rows_pb, N * OH);
  for (int r = r0; r < r1; ++r) {
    const int n = r / OH, oh = r - n * OH;
    int h0, h1;
    float lh;
    up_src(oh, H, OH, align, h0, h1, lh);
    const T* x0 = x + (long)(n * H + h0) * W * ldx + c0;
    const T* x1 = x + (long)(n * H + h1) * W * ldx + c0;
    float a[V], b[V], c[V], d[V], o[V];
    load_vec(x0 + (long)w0 * ldx, a);
    load_vec(x0 + (long)w1 * ldx, b);
    load_vec(x1 + (long)w0 * ldx, c);
    load_vec(x1 + (long)w1 * ldx, d);
    const float hl0 = 1.f - lh;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = up_blend(a[e], b[e], c[e], d[e], wl0, lw, hl0, lh);
    store_vec(y + ((long)r * OW + ow) * ldy + c0, o);
  }
}

// weight of output index d on input index i along one axis
__device__ __forceinline__ float up_w(int d, int i, int in, int out, int align) {
  int i0, i1;
  float l1;
  up_src(d, in, out, align, i0, i1, l1);
  float w = 0.f;
  if (i0 == i) w += 1.f - l1;
  if (i1 == i) w += l1;
  return w;
}

// candidate output range of input index i along one axis (a superset; exact weights decide)
__device__ __forceinline__ void up_range(int i, int in, int out, int align, int& lo, int& hi) {
  if (align) {
    lo = in > 1 ? (int)floorf((float)(i - 1) * (out - 1) / (float)(in - 1)) : 0;
    hi = in > 1 ? (int)ceilf((float)(i + 1) * (out - 1) / (float)(in - 1)) : out - 1;
  } else {
    lo = 2 * i - 2;
    hi = i == in - 1 ? out - 1 : 2 * i + 2;
  }
  lo = max(lo, 0);
  hi = min(hi, out - 1);
}

// Nonzero taps of input index i along one axis: the bilinear hat's support is contiguous and holds
// at most kUpK output indices at x2 in either align mode (open interval of length 4 + 2/(in-1) for
// align_corners, 4 for half-pixel) -> d0 and the weights of d0 .. d0 + kUpK - 1 (zero past the end).
constexpr int kUpK = 5;
__device__ __forceinline__ void up_taps(int i, int in, int out, int align, int& d0, float (&wt)[kUpK]) {
  int lo, hi;
  up_range(i, in, out, align, lo, hi);
  d0 = hi + 1;
  for (int d = hi; d >= lo; --d)
    if (up_w(d, i, in, out, align) != 0.f) d0 = d;
#pragma unroll
  for (int k = 0; k < kUpK; ++k) wt[k] = d0 + k <= hi ? up_w(d0 + k, i, in, out, align) : 0.f;
  if (d0 > hi) d0 = lo;
}

// Separable adjoint of the block's input rows r0 .. r0+nr-1 (r = n*H + h, nr <= R, wave-uniform):
// the dy rows J = n*OH + oh feeding them are contiguous in J (also across an image boundary), so
// each is gathered once per lane -- its column taps cw summed first (cs) -- and added to every
// block row it feeds with that row's weight: (2R+3)*4 loads per lane instead of R*16 for the
// per-pixel 2-D gather (+0.4% bench step at R = 4; R = 8 loses occupancy).  Row J+1's taps are
// loaded before row J's are consumed.  Zero weights are skipped (no 0 * inf).
template <typename T, int R, int PF = 1>
__device__ __forceinline__ void up_adjoint_rows(const T* dy, int ldy, int r0, int nr, int H, int OH, int OW,
                                                int align, int cd0, const float (&cw)[kUpK], int c0,
                                                float (&acc)[R][VE<T>]) {
  constexpr int V = VE<T>;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[i][e] = 0.f;
  int nh[R], hh[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int r = r0 + min(i, nr - 1);
    nh[i] = r / H;
    hh[i] = r - nh[i] * H;
  }
  int lo, hi, t;
  up_range(hh[0], H, OH, align, lo, t);
  up_range(hh[R - 1], H, OH, align, t, hi);
  const int J0 = nh[0] * OH + lo, J1 = nh[R - 1] * OH + hi;
  auto gather = [&](int J, uint4 (&g)[kUpK]) {
    const T* row = dy + ((long)J * OW + cd0) * ldy + c0;
#pragma unroll
    for (int kw = 0; kw < kUpK; ++kw)
      g[kw] = (J <= J1 && cw[kw] != 0.f) ? *reinterpret_cast<const uint4*>(row + (long)kw * ldy)
                                         : uint4{0u, 0u, 0u, 0u};
  };
  uint4 gc[kUpK];
  gather(J0, gc);
  // PF 2: rows J+1 and J+2 in flight while row J is consumed
  uint4 gm[kUpK];
  if constexpr (PF == 2) gather(J0 + 1, gm);
  for (int J = J0; J <= J1; ++J) {
    uint4 gn[kUpK];
    gather(J + PF, gn);
    const int n = J / OH, oh = J - n * OH;
    float cs[V];
#pragma unroll
    for (int e = 0; e < V; ++e) cs[e] = 0.f;
#pragma unroll
    for (int kw = 0; kw < kUpK; ++kw)
      if (cw[kw] != 0.f) {
        float gv[V];
        cvt16<T>(gc[kw], gv);
#pragma unroll
        for (int e = 0; e < V; ++e) cs[e] += cw[kw] * gv[e];
      }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float w = (i < nr && nh[i] == n) ? up_w(oh, hh[i], H, OH, align) : 0.f;
      if (w != 0.f) {
#pragma unroll
        for (int e = 0; e < V; ++e) acc[i][e] += w * cs[e];
      }
    }
#pragma unroll
    for (int kw = 0; kw < kUpK; ++kw) {
      if constexpr (PF == 2) {
        gc[kw] = gm[kw];
        gm[kw] = gn[kw];
      } else {
        gc[kw] = gn[kw];
      }
    }
  }
}

#ifndef UNETSEG_UPBWD_PF
#define UNETSEG_UPBWD_PF 2
#endif
// gather form of the adjoint: dx[h][w] (+)= sum_{oh,ow} wh(oh,h) ww(ow,w) dy[oh][ow]; row-blocked
// like the forward (row weights wave-uniform, column weights once per lane)
template <typename T, int R>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const T* dy, int ldy, int N, int H, int W, int C, int align, T* dx, int ldx,
                                    int accumulate) {
  constexpr int V = VE<T>;
  const int cv = C / V, OH = 2 * H, OW = 2 * W;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= W * cv) return;
  const int w = idx / cv, c0 = (idx - w * cv) * V;
  int cd0;
  float cw[kUpK];
  up_taps(w, W, OW, align, cd0, cw);
  const int r0 = blockIdx.y * R, nr = min(R, N * H - r0);
  float acc[R][V];
  up_adjoint_rows<T, R, UNETSEG_UPBWD_PF>(dy, ldy, r0, nr, H, OH, OW, align, cd0, cw, c0, acc);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    if (i >= nr) break;
    T* o = dx + ((long)(r0 + i) * W + w) * ldx + c0;
    if (accumulate) {
      float old[V];
      load_vec(o, old);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[i][e] += old[e];
    }
    store_vec(o, acc[i]);
  }
}

// upsample_bwd with the backward of the ReLU that produced x fused in (x = that ReLU's output, the
// upsample its sole consumer: the decoder's unetUp conv2 -> next block's Upsample,
// model/unet_resnet.py:25-33): dx = (A > 0) ? adjoint(dy) : 0, rounded to T as stored; part[g][0][c]
// = per-block column sums of the stored dx (the producer conv's bias-gradient partials, reduced by
// unetseg_colsum_rows), g = blockIdx.y * gridDim.x + blockIdx.x.  No accumulate.
template <typename T, int R>
__global__ __launch_bounds__(256) void upsample_bwd_relu_kernel(const T* dy, int ldy, int N, int H, int W, int C,
                                                                 int align, const T* A, int lda, T* dx, int ldx,
                                                                 float* part) {
  constexpr int V = VE<T>;
  __shared__ float red[256 * V];
  const int cv = C / V, OH = 2 * H, OW = 2 * W;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < W * cv;
  const int w = live ? idx / cv : 0, c0 = live ? (idx - w * cv) * V : 0;
  float s[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = 0.f;
  if (live) {
    int cd0;
    float cw[kUpK];
    up_taps(w, W, OW, align, cd0, cw);
    const int r0 = blockIdx.y * R, nr = min(R, N * H - r0);
    uint4 am[R];  // masks first: their latency hides under the gather
#pragma unroll
    for (int i = 0; i < R; ++i)
      am[i] = i < nr ? *reinterpret_cast<const uint4*>(A + ((long)(r0 + i) * W + w) * lda + c0) : uint4{0u, 0u, 0u, 0u};
    float acc[R][V];
    up_adjoint_rows<T, R>(dy, ldy, r0, nr, H, OH, OW, align, cd0, cw, c0, acc);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i >= nr) break;
      float a[V];
      cvt16<T>(am[i], a);
      T o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        o[e] = (T)(a[e] > 0.f ? acc[i][e] : 0.f);  // == upsample_bwd's stored value, then relu_bwd's mask
        s[e] += (float)o[e];
      }
      *reinterpret_cast<uint4*>(dx + ((long)(r0 + i) * W + w) * ldx + c0) = *reinterpret_cast<uint4*>(o);
    }
  }
  // block partials: the threads of one 8-channel group are tid % cv (256 % cv == 0, blocks start
  // at a pixel boundary)
#pragma unroll
  for (int e = 0; e < V; ++e) red[threadIdx.x * V + e] = s[e];
  __syncthreads();
  const long g = (long)blockIdx.y * gridDim.x + blockIdx.x;
  for (int i = threadIdx.x; i < cv * V; i += 256) {
    const int cx = i / V, e = i - cx * V;
    float t = 0.f;
    for (int j = cx; j < 256; j += cv) t += red[j * V + e];
    part[g * 2 * C + cx * V + e] = t;
  }
}

// Row-streaming form of upsample_bwd_relu (round 6): a block owns RS input rows of one image (RS | H)
// and walks the dy rows feeding them ONCE, top to bottom, keeping only the two input rows the current
// dy row touches (every dy row oh feeds rows i0 = floor(src) and i1 = i0 + 1, and i0 never decreases):
// a row is finished -- masked, stored, summed -- as soon as the walk passes it.  Against the R = 4
// row-blocked kernel above: (2 RS + 2) dy rows gathered per RS rows instead of (2 R + 3) per R
// (1.06x instead of 1.4x of dy re-read), K = 4 column taps where no column has a fifth (the U-Net
// sizes: up_taps_max), two rows in flight in 3 x K registers of 16 B, and the 32 accumulators of the
// R = 4 form down to 16.  Arithmetic identical to upsample_bwd (same up_taps / up_w weights, same
// per-row J order, same expressions): bit-identical dx.  part[g][0][c] as upsample_bwd_relu_kernel
// (g = blockIdx.y * gridDim.x + blockIdx.x).
// MASK false: the plain adjoint (unetseg_upsample2x_bwd: no ReLU, no partials, dx (+)= as upsample_bwd's).
template <typename T, int RS, int K, int PF, bool MASK = true>
__global__ __launch_bounds__(256, PF == 1 ? 4 : 3) void upsample_bwd_relu_stream_kernel(const T* dy, int ldy, int N, int H, int W,
                                                                        int C, int align, const T* A, int lda, T* dx,
                                                                        int ldx, float* part, int accumulate = 0) {
  constexpr int V = VE<T>;
  __shared__ float red[256 * V];
  const int cv = C / V, OH = 2 * H, OW = 2 * W;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < W * cv;
  const int w = live ? idx / cv : 0, c0 = live ? (idx - w * cv) * V : 0;
  float s[V];
#pragma unroll
  for (int e = 0; e < V; ++e) s[e] = 0.f;
  if (live) {
    int cd0;
    float cw5[kUpK];
    up_taps(w, W, OW, align, cd0, cw5);
    float cw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cw[k] = cw5[k];  // K = 4: the host checked cw5[4] == 0 for every column
    const int rb = blockIdx.y * RS;              // first stacked input row (n * H + h0), RS | H
    const int n = rb / H, h0 = rb - n * H;
    int lo, hi, t;
    up_range(h0, H, OH, align, lo, t);
    up_range(h0 + RS - 1, H, OH, align, t, hi);
    // dy through a buffer descriptor: per-lane tap offsets are constants (kOOB for a zero tap), the
    // dy row's offset is scalar -- no 64-bit address per tap and row
    const __amdgpu_buffer_rsrc_t rdy =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(dy), (short)0, (int)((long)N * OH * OW * ldy * (long)sizeof(T)), 0x00020000);
    unsigned toff[K];
#pragma unroll
    for (int k = 0; k < K; ++k) toff[k] = cw[k] != 0.f ? (unsigned)(((cd0 + k) * ldy + c0) * (int)sizeof(T)) : 0x80000000u;
    auto gather = [&](int oh, uint4 (&g)[K]) {
      const int ohc = oh <= hi ? oh : hi;  // past the block's last dy row: a re-read, never consumed
      const int soff = (int)(((long)n * OH + ohc) * OW * ldy * (long)sizeof(T));
#pragma unroll
      for (int k = 0; k < K; ++k) {
        typedef int i32x4_t __attribute__((ext_vector_type(4)));
        i32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rdy, (int)toff[k], soff, 0);
        g[k] = *reinterpret_cast<uint4*>(&v);
      }
    };
    const T* An = A + ((long)n * H * W + w) * lda + c0;
    T* dxn = dx + ((long)n * H * W + w) * ldx + c0;
    auto amask = [&](int r) -> uint4 {
      if constexpr (!MASK) return uint4{0u, 0u, 0u, 0u};
      return (r >= h0 && r < h0 + RS) ? *reinterpret_cast<const uint4*>(An + (long)r * W * lda) : uint4{0u, 0u, 0u, 0u};
    };
    // finish input row r (acc = its adjoint): mask, round as stored, partial sums
    auto finish = [&](int r, const float (&acc)[V], const uint4& am) {
      if (r < h0 || r >= h0 + RS) return;
      if constexpr (!MASK) {
        T* o = dxn + (long)r * W * ldx;
        float v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = acc[e];
        if (accumulate) {
          float old[V];
          load_vec(o, old);
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] += old[e];
        }
        store_vec(o, v);
        return;
      }
      float a[V];
      cvt16<T>(am, a);
      T o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        o[e] = (T)(a[e] > 0.f ? acc[e] : 0.f);
        s[e] += (float)o[e];
      }
      *reinterpret_cast<uint4*>(dxn + (long)r * W * ldx) = *reinterpret_cast<uint4*>(o);
    };
    int i0, i1;
    float l1;
    up_src(lo, H, OH, align, i0, i1, l1);
    int ra = i0;  // rows ra (accA) and ra + 1 (accB)
    float accA[V], accB[V];
#pragma unroll
    for (int e = 0; e < V; ++e) accA[e] = accB[e] = 0.f;
    uint4 mA = amask(ra), mB = amask(ra + 1);
    // PF dy rows in flight beyond the one being consumed (1 or 2)
    uint4 gc[K], gm[PF == 2 ? K : 1];
    gather(lo, gc);
    if constexpr (PF == 2) gather(lo + 1, gm);
    for (int oh = lo; oh <= hi; ++oh) {
      uint4 gn[K];
      gather(oh + PF, gn);
      up_src(oh, H, OH, align, i0, i1, l1);
      if (i0 > ra) {  // row ra has had its last dy row (i0 advances by at most one per dy row)
        finish(ra, accA, mA);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          accA[e] = accB[e];
          accB[e] = 0.f;
        }
        mA = mB;
        ++ra;
        mB = amask(ra + 1);
      }
      float cs[V];
#pragma unroll
      for (int e = 0; e < V; ++e) cs[e] = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (cw[k] != 0.f) {
          float gv[V];
          cvt16<T>(gc[k], gv);
#pragma unroll
          for (int e = 0; e < V; ++e) cs[e] += cw[k] * gv[e];
        }
      // the weights of upsample_bwd (up_w: rows i0 and i1, summed where they coincide)
      const float wA = up_w(oh, ra, H, OH, align), wB = up_w(oh, ra + 1, H, OH, align);
      if (wA != 0.f) {
#pragma unroll
        for (int e = 0; e < V; ++e) accA[e] += wA * cs[e];
      }
      if (wB != 0.f) {
#pragma unroll
        for (int e = 0; e < V; ++e) accB[e] += wB * cs[e];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if constexpr (PF == 2) {
          gc[k] = gm[k];
          gm[k] = gn[k];
        } else {
          gc[k] = gn[k];
        }
      }
    }
    finish(ra, accA, mA);
    finish(ra + 1, accB, mB);
  }
  if constexpr (!MASK) return;
#pragma unroll
  for (int e = 0; e < V; ++e) red[threadIdx.x * V + e] = s[e];
  __syncthreads();
  const long g = (long)blockIdx.y * gridDim.x + blockIdx.x;
  for (int i = threadIdx.x; i < cv * V; i += 256) {
    const int cx = i / V, e = i - cx * V;
    float t = 0.f;
    for (int j = cx; j < 256; j += cv) t += red[j * V + e];
    part[g * 2 * C + cx * V + e] = t;
  }
}

// host restatement of up_taps' tap count: the most nonzero column taps any input column has (4 or 5)
int up_taps_max(int in, int align) {
  const int out = 2 * in;
  int best = 0;
  for (int i = 0; i < in; ++i) {
    int lo, hi;
    if (align) {
      lo = in > 1 ? (int)floorf((float)(i - 1) * (out - 1) / (float)(in - 1)) : 0;
      hi = in > 1 ? (int)ceilf((float)(i + 1) * (out - 1) / (float)(in - 1)) : out - 1;
    } else {
      lo = 2 * i - 2;
      hi = i == in - 1 ? out - 1 : 2 * i + 2;
    }
    lo = std::max(lo, 0);
    hi = std::min(hi, out - 1);
    int cnt = 0;
    for (int d = lo; d <= hi; ++d) {
      float src;
      if (align) {
        const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
        src = scale * (float)d;
      } else {
        src = ((float)d + 0.5f) * 0.5f - 0.5f;
        if (src < 0.f) src = 0.f;
      }
      int i0 = (int)src;
      if (i0 > in - 1) i0 = in - 1;
      const int i1 = i0 + 1 < in ? i0 + 1 : in - 1;
      const float l1 = src - (float)i0;
      float wgt = 0.f;
      if (i0 == i) wgt += 1.f - l1;
      if (i1 == i) wgt += l1;
      if (wgt != 0.f) ++cnt;
    }
    best = std::max(best, cnt);
  }
  return best;
}

// rows per block of the row-streaming upsample backward (0: the row-blocked kernel): 16 where that
// still gives >= 2048 blocks, else 8; h must be a multiple (UNETSEG_UP_STREAM=0: off; read at every call)
int up_stream_rows(int dtype, int n, int h, int w, int c) {
  const char* e = getenv("UNETSEG_UP_STREAM");
  if (e && atoi(e) == 0) return 0;
  const long xb = ceil_div((long)w * (c / vec_elems(dtype)), 256);
  for (int rs : {16, 8})
    if (h % rs == 0 && (xb * ((long)n * h / rs) >= 2048 || rs == 8)) return rs;
  return 0;
}

// dy rows in flight ahead of the consumed one in the masked streaming kernel (UNETSEG_UP_STREAM_PF = 1
// or 2; latched on first use)
int up_stream_pf() {
  static const int pf = getenv("UNETSEG_UP_STREAM_PF") && atoi(getenv("UNETSEG_UP_STREAM_PF")) == 2 ? 2 : 1;
  return pf;
}

// How one upsample backward runs.  unetseg_upsample2x_bwd, _bwd_relu and the size query _bwd_tiles all
// read this, so the partial rows the caller allocates are the blocks the launch writes.
struct UpBwdPlan {
  bool stream;  // the row-streaming kernel (else the row-blocked one)
  int rows;     // input rows per block: 16 or 8 streaming, else up_rows_pb()
  int K;        // streaming: column taps carried, 4 where no input column has a fifth, else 5
  dim3 grid;    // x: (pixel, vector) lanes of one row / 256, y: row blocks
};
// align < 0: geometry only (K stays 0).  The masked streaming kernel's prefetch depth is no part of the
// plan: up_stream_pf() latches its knob, which only a streaming _bwd_relu launch may do.
UpBwdPlan up_bwd_plan(int dtype, int n, int h, int w, int c, int align) {
  UpBwdPlan p;
  const int rs = up_stream_rows(dtype, n, h, w, c);
  p.stream = rs != 0;
  p.rows = rs ? rs : up_rows_pb();
  p.K = p.stream && align >= 0 ? (up_taps_max(w, align) <= 4 ? 4 : 5) : 0;
  p.grid = dim3(ceil_div((long)w * (c / vec_elems(dtype)), 256), ceil_div((long)n * h, p.rows));
  return p;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
UNETSEG_API int unetseg_upsample2x_fwd(int dtype, const void* x, int ldx, int n, int h, int w, int c,
                                       int align_corners, void* y, int ldy, void* stream) {
  CHECK_VEC(dtype, c, "upsample_fwd");
  US_CHECK_ARG(x && y && n >= 0 && h >= 0 && w >= 0, "upsample_fwd: null pointer or negative size");
  DISPATCH_T(dtype, hipLaunchKernelGGL(upsample_fwd_kernel<T>,
                                       dim3(ceil_div(2 * w * (c / VE<T>), 256), ceil_div(n * 2 * h, up_rows_pb())),
                                       dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, n, h, w, c, align_corners,
                                       (T*)y, ldy, up_rows_pb()));
  US_LAUNCH_CHECK("upsample_fwd");
  return 0;
}

UNETSEG_API int unetseg_upsample2x_bwd(int dtype, const void* dy, int ldy, int n, int h, int w, int c,
                                       int align_corners, void* dx, int ldx, int accumulate, void* stream) {
  CHECK_VEC(dtype, c, "upsample_bwd");
  US_CHECK_ARG(dy && dx && n >= 0 && h >= 0 && w >= 0, "upsample_bwd: null pointer or negative size");
  const UpBwdPlan pl = up_bwd_plan(dtype, n, h, w, c, align_corners);
  hipStream_t st = (hipStream_t)stream;
  bool launched = false;
  if (pl.stream)
    // the row-streaming adjoint without the mask (as upsample_bwd_relu's default), bit-identical
    DISPATCH_T(dtype, with_const<16, 8>(pl.rows, [&](auto rs) {
      launched = with_const<4, 5>(pl.K, [&](auto k) {
        hipLaunchKernelGGL((upsample_bwd_relu_stream_kernel<T, decltype(rs)::value, decltype(k)::value, 1, false>),
                           pl.grid, dim3(256), 0, st, (const T*)dy, ldy, n, h, w, c, align_corners, (const T*)nullptr,
                           0, (T*)dx, ldx, (float*)nullptr, accumulate);
      });
    }));
  else
    DISPATCH_T(dtype, launched = with_const<2, 4, 8>(pl.rows, [&](auto r) {
      hipLaunchKernelGGL((upsample_bwd_kernel<T, decltype(r)::value>), pl.grid, dim3(256), 0, st, (const T*)dy, ldy, n,
                         h, w, c, align_corners, (T*)dx, ldx, accumulate);
    }));
  US_CHECK_ARG(launched, "upsample_bwd: no kernel for %d rows per block, %d taps", pl.rows, pl.K);
  US_LAUNCH_CHECK("upsample_bwd");
  return 0;
}

// partial rows (blocks) of unetseg_upsample2x_bwd_relu for this shape
UNETSEG_API int unetseg_upsample2x_bwd_tiles(int dtype, int n, int h, int w, int c) {
  const UpBwdPlan pl = up_bwd_plan(dtype, n, h, w, c, -1);
  return (int)pl.grid.x * (int)pl.grid.y;
}

UNETSEG_API int unetseg_upsample2x_bwd_relu(int dtype, const void* dy, int ldy, int n, int h, int w, int c,
                                            int align_corners, const void* a, int lda, void* dx, int ldx, float* part,
                                            int rows, void* stream) {
  CHECK_VEC(dtype, c, "upsample_bwd_relu");
  US_CHECK_ARG(dy && a && dx && part, "upsample_bwd_relu: null pointer");
  const int V = vec_elems(dtype);
  US_CHECK_ARG(c / V <= 256 && 256 % (c / V) == 0, "upsample_bwd_relu: channels / vector must divide 256");
  const UpBwdPlan pl = up_bwd_plan(dtype, n, h, w, c, align_corners);
  US_CHECK_ARG(rows == (int)pl.grid.x * (int)pl.grid.y, "upsample_bwd_relu: rows mismatch");
  hipStream_t st = (hipStream_t)stream;
  bool launched = false;
  if (pl.stream) {
    const int pfd = up_stream_pf();
    DISPATCH_T(dtype, with_const<16, 8>(pl.rows, [&](auto rs) {
      with_const<4, 5>(pl.K, [&](auto k) {
        launched = with_const<1, 2>(pfd, [&](auto pf) {
          hipLaunchKernelGGL(
              (upsample_bwd_relu_stream_kernel<T, decltype(rs)::value, decltype(k)::value, decltype(pf)::value>),
              pl.grid, dim3(256), 0, st, (const T*)dy, ldy, n, h, w, c, align_corners, (const T*)a, lda, (T*)dx, ldx,
              part);
        });
      });
    }));
  } else {
    DISPATCH_T(dtype, launched = with_const<2, 4, 8>(pl.rows, [&](auto r) {
      hipLaunchKernelGGL((upsample_bwd_relu_kernel<T, decltype(r)::value>), pl.grid, dim3(256), 0, st, (const T*)dy,
                         ldy, n, h, w, c, align_corners, (const T*)a, lda, (T*)dx, ldx, part);
    }));
  }
  US_CHECK_ARG(launched, "upsample_bwd_relu: no kernel for %d rows per block, %d taps", pl.rows, pl.K);
  US_LAUNCH_CHECK("upsample_bwd_relu");
  return 0;
}
