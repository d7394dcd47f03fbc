"""Float64 references of the memory-bound NHWC operations (BatchNorm apply / backward, channel statistics,
ReLU backward, add, column sums, max pool, bilinear x2 upsample, general bilinear resize, zero padding, the
narrow 1x1 heads, the attention gate, global average pooling, input packing) and the helpers of the per-element
contract tests (tests/test_gpu_elem_contract.py, test_gpu_resample_contract.py, test_gpu_pointwise_contract.py;
the references themselves are checked against PyTorch on the CPU in tests/test_nhwc_ref_cpu.py).

Written from the text of include/unetseg_hip.h, in torch float64 on the CPU; nothing here imports the library
or touches a GPU.  Activations are [pixels..][C] tensors (any leading shape), statistics are [C].

Every reference returns, next to its value, a *magnitude* of the same shape: the float64 sum of the absolute
values of the terms it added (|y*sc| + |sh| + |r|, sum w |x|, ...).  A kernel that evaluates the same
expression in fp32 with k roundings on its longest path and stores the result in the storage type lands within

    |got - ref| <= ulp_store(ref) + 1.01 * k * 2^-24 * mag

of the float64 value (assert_elementwise).  2^-24 is the relative error of one fp32 rounding, ulp_store the
spacing of the storage type at |ref| (2^-7 * 2^e for bf16, 2^-23 * 2^e for fp32, e = floor(log2 |ref|)).  Each
reference states its k with a one-line count; for a sum of n addends k = n, which holds for every summation
order and so for every block geometry.
"""
import math

import torch

F64 = torch.float64
EPS32 = 2.0 ** -24

#: elements of a 16-byte vector (the V of the header)
VEC = {torch.bfloat16: 8, torch.float32: 4}


def f64(x):
    return x.detach().to("cpu").to(F64)


def round_store(x, dtype):
    """x (float64) as the storage type holds it (through fp32, as the kernels round)"""
    return x.to(torch.float32).to(dtype)


# ------------------------------------------------------------------------------------------------
# contract helpers
# ------------------------------------------------------------------------------------------------
SENTINEL = 777.0  # finite, not produced by the data: inputs and accumulated outputs
NAN = float("nan")  # outputs that are written, not accumulated into


def sliced(shape_nhwc, C, ld, c0, dtype, fill, device="cpu"):
    """(buf, view): buf [*shape_nhwc][ld] filled with the sentinel `fill`, view = buf[..., c0:c0+C], the
    channel slice a kernel is handed (pointer view.data_ptr(), pixel stride ld)"""
    assert 0 <= c0 and c0 + C <= ld
    buf = torch.full(tuple(shape_nhwc) + (ld,), fill, dtype=dtype, device=device)
    return buf, buf[..., c0:c0 + C]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_guard(buf, c0, C, fill, what="buffer"):
    """every element of buf outside [..., c0:c0+C] still holds the sentinel, bit for bit"""
    want = _bits(torch.full((1,), fill, dtype=buf.dtype, device=buf.device))[0]
    b = _bits(buf)
    bad = b != want
    bad[..., c0:c0 + C] = False
    n = int(bad.sum())
    if n:
        first = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{what}: {n} guard elements outside channels [{c0}, {c0 + C}) were written; first at "
                             f"{first}: {buf[tuple(first)].item()!r} (sentinel {fill!r})")


def assert_tail(flat, n, fill, what="buffer"):
    """flat[n:] (the sentinel tail of an exact-size contiguous output) is untouched"""
    want = _bits(torch.full((1,), fill, dtype=flat.dtype, device=flat.device))[0]
    bad = _bits(flat.reshape(-1)[n:]) != want
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements past its {n} were written"


def ulp_store(ref, store_dtype):
    """spacing of the storage type at |ref| (float64 tensor), at least that of the smallest normal"""
    p = 7 if store_dtype == torch.bfloat16 else 23
    a = ref.abs().clamp_min(2.0 ** -126)
    e = torch.floor(torch.log2(a))
    # log2 of a value just below a power of two may round up: step back where 2^e > a
    e = torch.where(torch.pow(2.0, e) > a, e - 1, e)
    return torch.pow(2.0, e - p)


def bound(ref, mag, store_dtype, k):
    return ulp_store(ref, store_dtype) + 1.01 * k * EPS32 * mag


def assert_elementwise(got, ref, mag, store_dtype, k, what="output"):
    """|got - ref| <= ulp_store(ref) + 1.01 k 2^-24 mag at every element; returns the largest |got - ref| / bound.
    On failure reports the worst element's index with its got / ref / bound."""
    got, ref, mag = f64(got), f64(ref), f64(mag)
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    if ref.numel() == 0:
        return 0.0
    bnd = bound(ref, mag, store_dtype, k)
    err = (got - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    worst = float(ratio.max())
    if not worst <= 1.0:
        nbad = int((~(ratio <= 1.0)).sum())
        i = int(ratio.reshape(-1).argmax())
        idx = []
        for n in reversed(ref.shape):
            idx.insert(0, i % n)
            i //= n
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {nbad} of {ref.numel()} elements out of bound (k={k}); worst at {idx}: got "
                             f"{got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} bound "
                             f"{bnd.reshape(-1)[i].item():.3e} ratio {worst:.3g}")
    return worst


def k_measured(k_any, ratio):
    """The any-order k of a reduction of n addends cannot see a dropped addend once n is large.  `ratio` is the
    worst |got - ref| / bound measured for that reduction at k_any on an MI355X; below 1/50 the check uses
    k = 8 x ratio x k_any (rounded up) instead; None (not measured) or >= 1/50 keeps k_any."""
    return k_any if ratio is None or ratio >= 1 / 50 else math.ceil(8 * ratio * k_any)


def pack_mask(m, V):
    """bool [M][C] -> uint8 [M][C/V], bit e of byte (p, c/V) = m[p][c/V*V + e]"""
    M, C = m.shape
    w = m.reshape(M, C // V, V).to(torch.int32) << torch.arange(V, dtype=torch.int32)
    return w.sum(-1).to(torch.uint8)


def unpack_mask(b, V):
    M, cv = b.shape
    return ((b.to(torch.int32).unsqueeze(-1) >> torch.arange(V, dtype=torch.int32)) & 1).bool().reshape(M, cv * V)


# ------------------------------------------------------------------------------------------------
# BatchNorm forward
# ------------------------------------------------------------------------------------------------
#: fp32 roundings of out = [relu](y*sc + sh [+ r | + r*sc2 + sh2]) by res_mode: fma -> 1; fma, add -> 2;
#: fma, mul, add, add -> 4
K_BN_APPLY = {0: 1, 1: 2, 2: 4}


def bn_apply(y, sc, sh, r, sc2, sh2, res_mode, relu, store_dtype):
    """-> (value, mag, mask bytes [M][C/V] of the value rounded to the storage type, pre-ReLU value).
    k = K_BN_APPLY[res_mode] (the ReLU adds no rounding)."""
    y, sc, sh = f64(y), f64(sc), f64(sh)
    pre = y * sc + sh
    mag = (y * sc).abs() + sh.abs()
    if res_mode == 1:
        r = f64(r)
        pre = pre + r
        mag = mag + r.abs()
    elif res_mode == 2:
        r, sc2, sh2 = f64(r), f64(sc2), f64(sh2)
        pre = pre + (r * sc2 + sh2)
        mag = mag + (r * sc2).abs() + sh2.abs()
    val = pre.clamp_min(0.0) if relu else pre
    V = VEC[store_dtype]
    bits = pack_mask((round_store(val, store_dtype).to(F64) > 0).reshape(-1, y.shape[-1]), V)
    return val, mag, bits, pre


def channel_stats(x, tile):
    """x [M][C] -> (part [G][2][C] = (sum, M2 about the tile mean) per tile of `tile` rows, mag [G][2][C], k [G]).
    k per tile of n rows: the sum n adds -> n; M2: sub, square (d enters twice), n adds -> n + 3."""
    x = f64(x)
    M, C = x.shape
    G = (M + tile - 1) // tile
    part, mag, ks = torch.zeros(G, 2, C, dtype=F64), torch.zeros(G, 2, C, dtype=F64), []
    for g in range(G):
        t = x[g * tile:min(M, (g + 1) * tile)]
        d = t - t.mean(0)
        part[g, 0], part[g, 1] = t.sum(0), (d * d).sum(0)
        mag[g, 0], mag[g, 1] = t.abs().sum(0), (d * d).sum(0)
        ks.append(t.shape[0])
    return part, mag, ks


def batch_stats(x):
    """full-M (mean, biased variance) per channel"""
    x = f64(x)
    return x.mean(0), x.var(0, unbiased=False)


def bn_finalize(mean, var, M, gamma, beta, rmean, rvar, momentum, eps):
    """from the full-M statistics: dict of mean, invstd, scale, shift and the updated running statistics
    (momentum update with the unbiased variance, as nn.BatchNorm2d)"""
    gamma, beta = f64(gamma), f64(beta)
    inv = 1.0 / torch.sqrt(var + eps)
    unb = var * M / (M - 1) if M > 1 else var
    return dict(mean=mean, invstd=inv, scale=gamma * inv, shift=beta - mean * gamma * inv,
                rmean=(1 - momentum) * f64(rmean) + momentum * mean, rvar=(1 - momentum) * f64(rvar) + momentum * unb)


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps, conv_bias=None):
    """eval-mode scale = gamma / sqrt(rvar + eps), shift = beta - rmean * scale (+ conv_bias * scale: bn_fold)
    -> (scale, shift, mag of shift).  k: scale add, sqrt, div, mul -> 4; shift the same chain, mul, sub
    (fold: mul, add) -> 8."""
    gamma, beta, rmean, rvar = f64(gamma), f64(beta), f64(rmean), f64(rvar)
    sc = gamma / torch.sqrt(rvar + eps)
    sh = beta - rmean * sc
    mag = beta.abs() + (rmean * sc).abs()
    if conv_bias is not None:
        sh = sh + f64(conv_bias) * sc
        mag = mag + (f64(conv_bias) * sc).abs()
    return sc, sh, mag


# ------------------------------------------------------------------------------------------------
# BatchNorm backward
# ------------------------------------------------------------------------------------------------
K_BN_DY = 5  # dy: mul (c2*inv), mul (k1*.), sub (y - mean), fma, fma -> 5
K_DZ_ACC = 1  # dzout accumulate: one add (a plain store is exact: 0)


def bn_bwd(dA, mask, y1, mean1, inv1, y2, mean2, inv2, g1, g2, M, round_coef=False, want_dy=True):
    """Backward through [relu](BN(y1) [+ BN(y2)]) with dz = dA * mask (mask bool [M][C] or None).
    -> dict: dz; sums [3][C] = (sum dz, sum dz*xhat1, sum dz*xhat2) with sums_mag and k_sums = (M, M + 2, M + 2)
    (per term sub, mul, then the fma chain of M adds); coef [6][C] = (g1*inv1, mean dz, mean dz*xhat1, g2*inv2,
    mean dz, mean dz*xhat2) from these sums; dy1 / dy2 = c0 (dz - c1 - xhat c2) with their magnitudes, formed
    from coef_used: the exact table, or with round_coef that table rounded to fp32 (what the kernel under test is
    handed).  want_dy=False stops after the sums and the table.  k = K_BN_DY."""
    dA, y1, mean1, inv1, g1 = f64(dA), f64(y1), f64(mean1), f64(inv1), f64(g1)
    C = dA.shape[-1]
    dz = dA if mask is None else torch.where(mask, dA, torch.zeros((), dtype=F64))
    xh1 = (y1 - mean1) * inv1
    nb = 1 if y2 is None else 2
    sums, smag = torch.zeros(3, C, dtype=F64), torch.zeros(3, C, dtype=F64)
    sums[0], smag[0] = dz.sum(0), dz.abs().sum(0)
    sums[1], smag[1] = (dz * xh1).sum(0), (dz * xh1).abs().sum(0)
    exact = torch.zeros(6, C, dtype=F64)
    exact[0], exact[1], exact[2] = g1 * inv1, sums[0] / M, sums[1] / M
    if nb == 2:
        y2, mean2, inv2, g2 = f64(y2), f64(mean2), f64(inv2), f64(g2)
        xh2 = (y2 - mean2) * inv2
        sums[2], smag[2] = (dz * xh2).sum(0), (dz * xh2).abs().sum(0)
        exact[3], exact[4], exact[5] = g2 * inv2, sums[0] / M, sums[2] / M
    cf = exact.to(torch.float32).to(F64) if round_coef else exact
    out = dict(coef_used=cf[:3 * nb], dz=dz, sums=sums[:1 + nb], sums_mag=smag[:1 + nb], k_sums=(M, M + 2, M + 2)[:1 + nb],
               coef=exact[:3 * nb])
    if not want_dy:
        return out
    out["dy1"] = cf[0] * (dz - cf[1] - xh1 * cf[2])
    out["dy1_mag"] = (cf[0] * dz).abs() + (cf[0] * cf[1]).abs() + (cf[0] * xh1 * cf[2]).abs()
    if nb == 2:
        out["dy2"] = cf[3] * (dz - cf[4] - xh2 * cf[5])
        out["dy2_mag"] = (cf[3] * dz).abs() + (cf[3] * cf[4]).abs() + (cf[3] * xh2 * cf[5]).abs()
    return out


def relu_bwd_bias(dA, A):
    """-> (dY = dA where A > 0 else 0: exact, k = 0; column sums of dY, their mag; k = M adds)"""
    dA, A = f64(dA), f64(A)
    dY = torch.where(A > 0, dA, torch.zeros((), dtype=F64))
    return dY, dY.sum(0), dY.abs().sum(0)


def add(x, out0):
    """out = out0 + x -> (value, mag); k = 1 (one add)"""
    x, out0 = f64(x), f64(out0)
    return out0 + x, out0.abs() + x.abs()


def colsum(part, accumulate, out0=None):
    """part [G][C] (fp32 partials, summed in fp64 by the finalize kernels) -> out[c] = sum_g part (+ out0)
    -> (value, mag); k = 2: the cast of the fp64 sum to fp32, the add onto out0"""
    part = f64(part)
    v, m = part.sum(0), part.abs().sum(0)
    if accumulate:
        v, m = v + f64(out0), m + f64(out0).abs()
    return v, m


# ------------------------------------------------------------------------------------------------
# max pool
# ------------------------------------------------------------------------------------------------
def pool_out(h, k, s, ceil):
    p = (h - k + s - 1) // s + 1 if ceil else (h - k) // s + 1
    if ceil and (p - 1) * s >= h:  # the last window starts inside the input
        p -= 1
    return p


def maxpool(x, k, s, ceil):
    """x [N][H][W][C] (no padding) -> (y [N][P][Q][C], idx uint8 = r*k+u of the maximum inside the window, the
    first in raster order on a tie, backward).  backward(dy, dx0=None) -> (dx, mag, k_roundings): dx[h][w] =
    sum of dy over the windows whose maximum sits at (h, w) (+ dx0); one add per window and one for dx0."""
    x = f64(x)
    N, H, W, C = x.shape
    P, Q = pool_out(H, k, s, ceil), pool_out(W, k, s, ceil)
    y = torch.full((N, P, Q, C), -math.inf, dtype=F64)
    idx = torch.zeros(N, P, Q, C, dtype=torch.uint8)
    for r in range(k):
        for u in range(k):
            # windows (p, q) whose tap (r, u) lies inside the input
            pn, qn = min(P, (H - 1 - r) // s + 1), min(Q, (W - 1 - u) // s + 1)
            if pn <= 0 or qn <= 0:
                continue
            tap = x[:, r:r + (pn - 1) * s + 1:s, u:u + (qn - 1) * s + 1:s]
            better = tap > y[:, :pn, :qn]  # strict: a tie keeps the earlier position
            y[:, :pn, :qn] = torch.where(better, tap, y[:, :pn, :qn])
            idx[:, :pn, :qn] = torch.where(better, torch.tensor(r * k + u, dtype=torch.uint8), idx[:, :pn, :qn])

    def backward(dy, dx0=None):
        dy = f64(dy)
        dx, mag = torch.zeros(N, H, W, C, dtype=F64), torch.zeros(N, H, W, C, dtype=F64)
        for r in range(k):
            for u in range(k):
                pn, qn = min(P, (H - 1 - r) // s + 1), min(Q, (W - 1 - u) // s + 1)
                if pn <= 0 or qn <= 0:
                    continue
                hit = idx[:, :pn, :qn] == r * k + u
                g = torch.where(hit, dy[:, :pn, :qn], torch.zeros((), dtype=F64))
                dx[:, r:r + (pn - 1) * s + 1:s, u:u + (qn - 1) * s + 1:s] += g
                mag[:, r:r + (pn - 1) * s + 1:s, u:u + (qn - 1) * s + 1:s] += g.abs()
        kk = ((k + s - 1) // s) ** 2
        if dx0 is not None:
            dx, mag, kk = dx + f64(dx0), mag + f64(dx0).abs(), kk + 1
        return dx, mag, kk

    return y, idx, backward


# ------------------------------------------------------------------------------------------------
# bilinear resize (ATen's source-index rule) and the x2 upsample
# ------------------------------------------------------------------------------------------------
def axis_taps(n_in, n_out, align, index_dtype=torch.float32, fused=True):
    """(i0, i1, l1) per output index along one axis, computed in `index_dtype` (float32: the rule as printed in
    the header and at the top of resize.hip):
      align_corners: src = dst * (in-1)/(out-1)   (scale 0 when out == 1)
      otherwise:     src = max(0, fma(dst + 0.5, in/out, -0.5))   (fused=False: the product rounded first)
      i0 = (int)src (at most in-1), i1 = i0 + (i0 < in-1), l1 = src - i0"""
    d = torch.arange(n_out, dtype=index_dtype)
    one = torch.ones((), dtype=index_dtype)
    if align:
        scale = (one * (n_in - 1)) / (one * (n_out - 1)) if n_out > 1 else one * 0
        src = d * scale
    else:
        scale = (one * n_in) / (one * n_out)
        # the library's rule: one fused multiply-add, rounded once (the fp32 product is exact in float64).  ATen
        # builds that contract the expression (GPU, AVX2 and later) evaluate the same; one that rounds the
        # product first (fused=False) moves l1 by up to 2^-24 * src
        if fused:
            src = ((d.to(F64) + 0.5) * scale.to(F64) - 0.5).to(index_dtype).clamp_min(0)
        else:
            src = ((d + 0.5) * scale - 0.5).clamp_min(0)
    i0 = src.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = src - i0.to(index_dtype)
    return i0, i1, l1.to(F64)


def axis_matrix(n_in, n_out, align, index_dtype=torch.float32, fused=True):
    """dense float64 W [n_out][n_in]: row d holds 1 - l1 at i0 and l1 at i1 (summed where they coincide)"""
    i0, i1, l1 = axis_taps(n_in, n_out, align, index_dtype, fused)
    Wm = torch.zeros(n_out, n_in, dtype=F64)
    rows = torch.arange(n_out)
    Wm.index_put_((rows, i0), 1.0 - l1, accumulate=True)
    Wm.index_put_((rows, i1), l1, accumulate=True)
    return Wm


K_RESIZE_FWD = 6  # 1 - lx, mul, add, 1 - ly, mul, add on the longest chain of the four-tap blend


def resize(x, oh, ow, align, index_dtype=torch.float32):
    """x [N][H][W][C] -> (y = Wy x Wx^T, mag = Wy |x| Wx^T, backward).  k = K_RESIZE_FWD.
    backward(dy, dx0=None) -> (dx = Wy^T dy Wx (+ dx0), mag, k): per term the two weights (1 - l, and an add where
    both taps name the pixel: 2 each), their product, the product with dy, then one add per contributing
    output pixel (the most any input pixel has) and one for dx0."""
    x = f64(x)
    N, H, W, C = x.shape
    Wy, Wx = axis_matrix(H, oh, align, index_dtype), axis_matrix(W, ow, align, index_dtype)

    def apply(A, B, t):  # A over the row axis, B over the column axis
        return torch.einsum("ph,nhwc,qw->npqc", A, t, B)

    y, mag = apply(Wy, Wx, x), apply(Wy, Wx, x.abs())

    def backward(dy, dx0=None):
        dy = f64(dy)
        dx, m = apply(Wy.t(), Wx.t(), dy), apply(Wy.t(), Wx.t(), dy.abs())
        terms = int((Wy != 0).sum(0).max()) * int((Wx != 0).sum(0).max())
        kk = 6 + terms
        if dx0 is not None:
            dx, m, kk = dx + f64(dx0), m + f64(dx0).abs(), kk + 1
        return dx, m, kk

    return y, mag, backward


def upsample2x(x, align, index_dtype=torch.float32):
    """bilinear x2: the resize to (2H, 2W) (in/out = 0.5 exactly; align_corners (in-1)/(2 in - 1) in fp32)"""
    return resize(x, 2 * x.shape[1], 2 * x.shape[2], align, index_dtype)


# ------------------------------------------------------------------------------------------------
# zero padding
# ------------------------------------------------------------------------------------------------
def pad2d(x, top, left, oh, ow):
    """x [N][H][W][C] into zeros [N][oh][ow][C] at (top, left) -> (y: exact, k = 0; backward).
    backward(dy, dx0=None) -> (dx = the window of dy (+ dx0), mag, k = 0 or 1)"""
    x = f64(x)
    N, H, W, C = x.shape
    y = torch.zeros(N, oh, ow, C, dtype=F64)
    y[:, top:top + H, left:left + W] = x

    def backward(dy, dx0=None):
        g = f64(dy)[:, top:top + H, left:left + W].clone()
        if dx0 is None:
            return g, g.abs(), 0
        return g + f64(dx0), g.abs() + f64(dx0).abs(), 1

    return y, backward


# ------------------------------------------------------------------------------------------------
# narrow 1x1 heads (pw_small_*, pw_head_*): y planar [N][K][HW], x NHWC [M][C], M = N * HW
# ------------------------------------------------------------------------------------------------
#: one double-precision rounding in units of an fp32 rounding: a sum of n addends accumulated in double and cast
#: to float once has k = 1 (the summand's own fp32 roundings) or 0, plus n * K_DOUBLE
K_DOUBLE = 2.0 ** -29


def tile_ranges(M, tile):
    """[(p0, p1)] of the pixel tiles a kernel's grid runs: tile pixels each, the last one ragged"""
    return [(p0, min(M, p0 + tile)) for p0 in range(0, M, tile)]


def _planar(v, N):
    """[M][K] -> planar [N][K][HW]"""
    M, K = v.shape
    return v.reshape(N, M // N, K).permute(0, 2, 1).contiguous()


def _rows(v):
    """planar [N][K][HW] -> [M][K]"""
    N, K, HW = v.shape
    return v.permute(0, 2, 1).reshape(N * HW, K)


def pw_fwd(x, w, b, N):
    """y[n][k][hw] = sum_c x[p][c] w[k][c] + b[k] (b may be None) -> (y, mag) planar [N][K][HW].
    k = C + 2: C addends, their products rounded (a fused multiply-add saves that one), the bias add."""
    x, w = f64(x), f64(w)
    y, mag = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        y, mag = y + f64(b), mag + f64(b).abs()
    return _planar(y, N), _planar(mag, N)


def pw_bwd(dy, x, w, dx0, tile):
    """Backward of pw_fwd over pixel tiles of `tile`: dy planar [N][K][HW], x [M][C], w [K][C], dx0 [M][C] or None.
    -> dict: dx = dy . W (+ dx0) with dx_mag, k = K + 1 (+ 1 with dx0): K addends, rounded products, the add
    onto dx0; part_w [K][C][G] = sum over the tile's pixels of dy[p][k] x[p][c] with part_w_mag, k = n + 1 (n
    pixels of the tile, rounded products); part_b [K][G] = sum of dy[p][k] with part_b_mag, k = n; n [G]."""
    g, x, w = _rows(f64(dy)), f64(x), f64(w)
    M, C = x.shape
    K = w.shape[0]
    dx, dmag = g @ w, g.abs() @ w.abs()
    if dx0 is not None:
        dx, dmag = dx + f64(dx0), dmag + f64(dx0).abs()
    tiles = tile_ranges(M, tile)
    G = len(tiles)
    pw, pwm = torch.zeros(K, C, G, dtype=F64), torch.zeros(K, C, G, dtype=F64)
    pb, pbm = torch.zeros(K, G, dtype=F64), torch.zeros(K, G, dtype=F64)
    for i, (p0, p1) in enumerate(tiles):
        pw[:, :, i], pwm[:, :, i] = g[p0:p1].t() @ x[p0:p1], g[p0:p1].abs().t() @ x[p0:p1].abs()
        pb[:, i], pbm[:, i] = g[p0:p1].sum(0), g[p0:p1].abs().sum(0)
    return dict(dx=dx, dx_mag=dmag, part_w=pw, part_w_mag=pwm, part_b=pb, part_b_mag=pbm, n=[b - a for a, b in tiles])


def tile_colsum(v, tile):
    """v [M][C] -> (per-tile column sums [G][C], their magnitudes); k = n (the tile's pixels)"""
    v = f64(v)
    tiles = tile_ranges(v.shape[0], tile)
    return (torch.stack([v[a:b].sum(0) for a, b in tiles]), torch.stack([v[a:b].abs().sum(0) for a, b in tiles]))


def pw_bwd_relu(dy, x, w, tile, store_dtype):
    """pw_bwd with the backward of the ReLU that produced x fused: -> pw_bwd's dict with
    dx_pre = dy . W where x > 0, else 0 (the value before the store; its bound is pw_bwd's, k = K + 1, and
    the zeros are exact), dx = round_store(dx_pre), part_d [G][2][C]: slot 0 the column sums of the *stored*
    dx over the tile (k = n), slot 1 zero, with part_d_mag."""
    out = pw_bwd(dy, x, w, None, tile)
    pos = f64(x) > 0
    zero = torch.zeros((), dtype=F64)
    out["dx_pre"] = torch.where(pos, out["dx"], zero)
    out["dx_mag"] = torch.where(pos, out["dx_mag"], zero)
    out["dx"] = round_store(out["dx_pre"], store_dtype).to(F64)
    s, m = tile_colsum(out["dx"], tile)
    out["part_d"] = torch.stack([s, torch.zeros_like(s)], 1)
    out["part_d_mag"] = torch.stack([m, torch.zeros_like(m)], 1)
    return out


def tile_stats(v, tile):
    """v [M] (the fp32 psi a kernel stored) -> (part [G][2] = (sum, M2 about the tile mean), mag [G][2], n [G]).
    Accumulated in double from the stored fp32 values and cast once: k = n * K_DOUBLE (sum), (n + 3) * K_DOUBLE
    (M2), each next to the store's own ulp."""
    part, mag, n = channel_stats(f64(v).reshape(-1, 1), tile)
    return part[:, :, 0], mag[:, :, 0], n


# ------------------------------------------------------------------------------------------------
# attention gate: alpha = sigmoid(psi * sc + sh), gated = skip * alpha, and its backward
# ------------------------------------------------------------------------------------------------
def attn_alpha(psi, sc, sh):
    """-> (alpha = sigmoid(z), z = psi * sc + sh, mag of z) in float64"""
    psi, sc, sh = f64(psi), f64(sc).reshape(()), f64(sh).reshape(())
    z = psi * sc + sh
    return torch.sigmoid(z), z, (psi * sc).abs() + sh.abs()


def attn_apply(skip, alpha):
    """gated[p][c] = skip[p][c] alpha[p] -> (value, mag); k = 1 (one product)"""
    v = f64(skip) * f64(alpha).unsqueeze(-1)
    return v, v.abs()


def attn_bwd1(dg, skip, alpha, ds0=None):
    """-> dict: dskip = dg alpha (+ ds0) with dskip_mag, k = 1 (+ 1 with ds0; a fused multiply-add saves it);
    dpsibn[p] = (sum_c dg skip) alpha (1 - alpha) with dpsibn_mag, k = C + 4: C addends, rounded products,
    the product with alpha, 1 - alpha, the product with it."""
    dg, skip, al = f64(dg), f64(skip), f64(alpha)
    ds = dg * al.unsqueeze(-1)
    dsm = ds.abs()
    if ds0 is not None:
        ds, dsm = ds + f64(ds0), dsm + f64(ds0).abs()
    s = al * (1 - al)
    return dict(dskip=ds, dskip_mag=dsm, dpsibn=(dg * skip).sum(-1) * s, dpsibn_mag=(dg * skip).abs().sum(-1) * s)


def attn_bwd1_part(dpsibn, psi, mean, inv, tile=128):
    """per-tile partials [2][G1] of the psi BatchNorm's backward from the stored fp32 dpsibn: sum of dpsibn, sum of
    dpsibn * xhat with xhat = (psi - mean) * inv -> (part, mag, n [G1]).  Accumulated in double: k = n * K_DOUBLE
    for the first; the second forms psi - mean in fp32: k = 1 + n * K_DOUBLE."""
    d, psi, mean, inv = f64(dpsibn), f64(psi), f64(mean).reshape(()), f64(inv).reshape(())
    t = d * ((psi - mean) * inv)
    tiles = tile_ranges(d.shape[0], tile)
    part = torch.stack([torch.stack([d[a:b].sum() for a, b in tiles]), torch.stack([t[a:b].sum() for a, b in tiles])])
    mag = torch.stack([torch.stack([d[a:b].abs().sum() for a, b in tiles]),
                       torch.stack([t[a:b].abs().sum() for a, b in tiles])])
    return part, mag, [b - a for a, b in tiles]


K_ATTN_DPSI = 5  # psi - mean, * inv, dpsibn - coef1, the multiply-add with coef2, * coef0


def attn_bwd2(dpsibn, psi, mean, inv, coef, f, wpsi, tile):
    """dpsi = coef0 (dpsibn - coef1 - xhat coef2) (k = K_ATTN_DPSI); dzf[p][c] = dpsi[p] wpsi[c] where f > 0, else 0
    (k = K_ATTN_DPSI + 1); part_w [C][G] = sum over the tile's pixels of dpsi f (k = n + K_ATTN_DPSI); part_b [G] =
    sum of dpsi (k = n + K_ATTN_DPSI) -> dict with the magnitudes and n [G]."""
    d, psi, mean, inv, coef = f64(dpsibn), f64(psi), f64(mean).reshape(()), f64(inv).reshape(()), f64(coef).reshape(-1)
    f, w = f64(f), f64(wpsi).reshape(-1)
    xh = (psi - mean) * inv
    dp = coef[0] * (d - coef[1] - xh * coef[2])
    dpm = coef[0].abs() * (d.abs() + coef[1].abs() + (xh * coef[2]).abs())
    pos = f > 0
    zero = torch.zeros((), dtype=F64)
    dzf = torch.where(pos, dp.unsqueeze(-1) * w, zero)
    dzm = torch.where(pos, dpm.unsqueeze(-1) * w.abs(), zero)
    tiles = tile_ranges(d.shape[0], tile)
    pw = torch.stack([dp[a:b] @ f[a:b] for a, b in tiles], 1)
    pwm = torch.stack([dpm[a:b] @ f[a:b].abs() for a, b in tiles], 1)
    pb = torch.stack([dp[a:b].sum() for a, b in tiles])
    pbm = torch.stack([dpm[a:b].sum() for a, b in tiles])
    return dict(dpsi=dp, dpsi_mag=dpm, dzf=dzf, dzf_mag=dzm, part_w=pw, part_w_mag=pwm, part_b=pb, part_b_mag=pbm,
                n=[b - a for a, b in tiles])


# ------------------------------------------------------------------------------------------------
# global average pooling, input packing
# ------------------------------------------------------------------------------------------------
def gap_fwd(x):
    """x [B][HW][C] -> (g [B][C] = the mean over the pixels, mag).  Summed in double, divided in double, cast
    once: k = (HW + 1) * K_DOUBLE next to the store's ulp."""
    x = f64(x)
    return x.mean(1), x.abs().mean(1)


def gap_bwd(dg, HW, dx0=None):
    """dx[b][p][c] = dg[b][c] / HW (+ dx0) -> (value [B][HW][C], mag); k = 1 (the division), + 1 with dx0"""
    v = (f64(dg) / HW).unsqueeze(1).expand(-1, HW, -1).clone()
    m = v.abs()
    if dx0 is not None:
        v, m = v + f64(dx0), m + f64(dx0).abs()
    return v, m


def pack_input(x, cpad, store_dtype):
    """NCHW fp32 [N][C][H][W] -> NHWC [N][H][W][cpad] in the storage type, channels >= C zero: exact"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, cpad, dtype=store_dtype)
    y[..., :C] = x.detach().cpu().permute(0, 2, 3, 1).to(torch.float32).to(store_dtype)
    return y


def pack_input_stem(x):
    """NCHW fp32 [N][C][H][W], C <= 8 -> bf16 [N][H][W + 8][8]: image column w at packed column w + 3, the 3 left
    and 5 right border columns and the channels >= C zero: exact"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W + 8, 8, dtype=torch.bfloat16)
    y[:, :, 3:3 + W, :C] = x.detach().cpu().permute(0, 2, 3, 1).to(torch.float32).to(torch.bfloat16)
    return y
