"""GPU: per-element contract of the pooling and resampling kernels (csrc/pool.hip, upsample.hip, resize.hip)
against the float64 references of tests/nhwc_ref.py: max pool through its three kernel pairs, the bilinear x2
upsample with its two adjoints, the general bilinear resize and the zero padding.  Inputs, outputs and
gradients are channel slices of wider buffers whose other channels hold a sentinel that must survive; values are
held element by element to |got - ref| <= ulp_store(ref) + 1.01 k 2^-24 mag (nhwc_ref.assert_elementwise), pooled
values, argmax bytes and padded values exactly.  The resize reference is a product of dense per-axis weight
matrices, so a contribution the backward's candidate range misses is a wrong element.  Each test prints the
largest |got - ref| / bound per operation; DESIGN.md (section 4a) holds the table measured on an MI355X.
"""
import zlib

import pytest
import torch

import nhwc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
WORST = {}
ANY = {}  # (reduction, dtype, n) -> worst ratio at the any-order k, printed at the end: the source of RED_MEASURED


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()
    yield
    for (op, dt), r in sorted(WORST.items()):
        print(f"\nworst ratio  {op:<28s} {dt:<5s} {r:.4g}", end="")
    for key, r in sorted(ANY.items()):
        print(f"\nany-order    {key!r}: {r:.4g},", end="")
    print()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(name):
    from unetseg_hip.lib import DT_BF16, DT_F32
    return (DT_BF16, torch.bfloat16, 8) if name == "bf16" else (DT_F32, torch.float32, 4)


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _rnd(g, shape, tdt):
    return torch.randn(*shape, generator=g).to(tdt)


def _put(t, ld, c0, fill=R.SENTINEL):
    buf, v = R.sliced(t.shape[:-1], t.shape[-1], ld, c0, t.dtype, fill, DEV)
    v.copy_(t)
    return buf, v


def _check(op, dtname, got, ref, mag, store, k):
    r = R.assert_elementwise(got, ref, mag, store, k, what=f"{op} {dtname}")
    WORST[(op, dtname)] = max(WORST.get((op, dtname), 0.0), r)
    print(f"ratio {op} {dtname} k={k}: {r:.4g}")
    return r


#: Worst |got - ref| / bound of the long sums this file checks, at the any-order k, measured on an MI355X per
#: (operation, dtype, n): n = pixels for the column sums of upsample2x_bwd_relu, n = the any-order k (6 + the most
#: output pixels one input pixel gathers, + 1 accumulating) for resize_bilinear_bwd.  _check_red asserts the
#: any-order bound and, where the entry is below 1/50, the bound with k = 8 x ratio x k_any
#: (nhwc_ref.k_measured): the measured value of each call is its entry here.
RED_MEASURED = {
    ('resize_bilinear_bwd', 'bf16', 7): 0.5,
    ('resize_bilinear_bwd', 'bf16', 8): 0.5,
    ('resize_bilinear_bwd', 'bf16', 9): 0.5,
    ('resize_bilinear_bwd', 'bf16', 10): 0.4999,
    ('resize_bilinear_bwd', 'bf16', 18): 0.4604,
    ('resize_bilinear_bwd', 'bf16', 19): 0.4371,
    ('resize_bilinear_bwd', 'bf16', 24): 0.4986,
    ('resize_bilinear_bwd', 'bf16', 25): 0.4993,
    ('resize_bilinear_bwd', 'bf16', 31): 0.4995,
    ('resize_bilinear_bwd', 'bf16', 32): 0.4996,
    ('resize_bilinear_bwd', 'bf16', 1182): 0.4499,
    ('resize_bilinear_bwd', 'bf16', 1183): 0.4146,
    ('resize_bilinear_bwd', 'fp32', 7): 0.1764,
    ('resize_bilinear_bwd', 'fp32', 8): 0.1479,
    ('resize_bilinear_bwd', 'fp32', 9): 0.102,
    ('resize_bilinear_bwd', 'fp32', 10): 0.04589,
    ('resize_bilinear_bwd', 'fp32', 18): 0.04747,
    ('resize_bilinear_bwd', 'fp32', 19): 0.04169,
    ('resize_bilinear_bwd', 'fp32', 24): 0.08347,
    ('resize_bilinear_bwd', 'fp32', 25): 0.06856,
    ('resize_bilinear_bwd', 'fp32', 31): 0.08874,
    ('resize_bilinear_bwd', 'fp32', 32): 0.07092,
    ('resize_bilinear_bwd', 'fp32', 1182): 0.002326,
    ('resize_bilinear_bwd', 'fp32', 1183): 0.002347,
    ('upsample2x_bwd_relu colsum', 'bf16', 3): 0,
    ('upsample2x_bwd_relu colsum', 'bf16', 35): 0,
    ('upsample2x_bwd_relu colsum', 'bf16', 42): 0,
    ('upsample2x_bwd_relu colsum', 'bf16', 512): 0.0001035,
    ('upsample2x_bwd_relu colsum', 'fp32', 3): 0.2092,
    ('upsample2x_bwd_relu colsum', 'fp32', 35): 0.0291,
    ('upsample2x_bwd_relu colsum', 'fp32', 42): 0.01436,
    ('upsample2x_bwd_relu colsum', 'fp32', 512): 0.0009385,
}


def _check_red(op, dtname, n, got, ref, mag, store, k_any):
    r = R.assert_elementwise(got, ref, mag, store, k_any, what=f"{op} {dtname} n={n} (any order)")
    key = (op, dtname, n)
    ANY[key] = max(ANY.get(key, 0.0), r)
    print(f"ratio {op} {dtname} n={n} any-order k={k_any}: {r:.4g}")
    k = R.k_measured(k_any, RED_MEASURED.get(key))
    if k != k_any:
        _check(f"{op} n={n}", dtname, got, ref, mag, store, k)
    else:
        WORST[(f"{op} n={n}", dtname)] = max(WORST.get((f"{op} n={n}", dtname), 0.0), r)


def _same(got, ref64, tdt, what):
    assert torch.equal(R._bits(got.cpu()), R._bits(R.round_store(ref64, tdt))), f"{what}: not exact"


def _grad_out(g, shape, tdt, ld, c0, accumulate):
    """the gradient output slice: NaN guards and content when written, a sentinel guard around random content when
    accumulated into -> (buf, view, dx0 or None, fill)"""
    if accumulate:
        dx0 = _rnd(g, shape, tdt)
        buf, v = _put(dx0, ld, c0)
        return buf, v, dx0, R.SENTINEL
    buf, v = R.sliced(shape[:-1], shape[-1], ld, c0, tdt, R.NAN, DEV)
    return buf, v, None, R.NAN


# ------------------------------------------------------------------------------------------------
# max pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,cmul", [(2, 6, 10, 2), (1, 7, 9, 1), (3, 3, 4, 3)])
@pytest.mark.parametrize("k,s,ceil", [(2, 2, 0), (3, 2, 1), (3, 1, 0)])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_maxpool(dtname, k, s, ceil, N, H, W, cmul):
    """2x2 / s2 (the exact-tiling kernels at 6 x 10, the generic ones at the odd sizes), 3x3 / s2 ceil mode (the
    stem pool's kernels), 3x3 / s1 (generic, nine windows per pixel)"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cmul * V
    g = _gen("pool", dtname, k, s, H, W)
    x = (torch.randint(-3, 4, (N, H, W, C), generator=g) * 0.5).to(tdt)  # a coarse grid: ties in most windows
    x[0, :2, :2, :] = 1.5
    y, idx, backward = R.maxpool(x, k, s, ceil)
    P, Q = y.shape[1], y.shape[2]
    xbuf, xv = _put(x, C + V, V)
    ybuf, yv = R.sliced((N, P, Q), C, C + 2 * V, V, tdt, R.NAN, DEV)
    n_idx = N * P * Q * C
    didx = torch.full((n_idx + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    lib.maxpool_fwd(dt, xv.data_ptr(), C + V, N, H, W, C, k, s, ceil, yv.data_ptr(), C + 2 * V, didx.data_ptr(), None,
                    None, _st())
    torch.cuda.synchronize()
    _same(yv, y, tdt, "pooled values")
    assert torch.equal(didx[:n_idx].cpu().view(N, P, Q, C), idx), "argmax bytes (a tie goes to the first position)"
    R.assert_tail(didx, n_idx, 0xEE, "idx")
    R.assert_guard(ybuf, V, C, R.NAN, "maxpool y")
    R.assert_guard(xbuf, V, C, R.SENTINEL, "maxpool x")
    dy = _rnd(g, (N, P, Q, C), tdt)
    dybuf, dyv = _put(dy, C + 2 * V, V)
    for accumulate in (0, 1):
        dbuf, dv, dx0, fill = _grad_out(g, (N, H, W, C), tdt, C + V, V, accumulate)
        lib.maxpool_bwd(dt, dyv.data_ptr(), C + 2 * V, didx.data_ptr(), N, H, W, C, k, s, P, Q, dv.data_ptr(), C + V,
                        accumulate, _st())
        torch.cuda.synchronize()
        dx, mag, kk = backward(dy, dx0)
        _check(f"maxpool_bwd k{k}s{s}", dtname, dv, dx, mag, tdt, kk)
        R.assert_guard(dbuf, V, C, fill, "maxpool dx")
    R.assert_guard(dybuf, V, C, R.SENTINEL, "maxpool dy")


# ------------------------------------------------------------------------------------------------
# bilinear x2 upsample
# ------------------------------------------------------------------------------------------------
K_UP_FWD = R.K_RESIZE_FWD
#: the separable adjoint: per axis a weight (1 - l: 1), its product (1) and up to five taps added (5) -> 2 * 7;
#: one more for the add onto the old gradient when accumulating
K_UP_BWD = 14
UP_SIZES = [(1, 1, 3), (1, 5, 7), (3, 7, 2), (2, 16, 16)]


@pytest.mark.parametrize("cmul", [1, 3, "64"])
@pytest.mark.parametrize("N,H,W", UP_SIZES)
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_upsample2x(dtname, align, N, H, W, cmul):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = 64 if cmul == "64" else cmul * V
    g = _gen("up", dtname, align, H, W, C)
    x = _rnd(g, (N, H, W, C), tdt)
    y, mag, backward = R.upsample2x(x, bool(align))
    xbuf, xv = _put(x, C + V, V)
    ybuf, yv = R.sliced((N, 2 * H, 2 * W), C, C + 2 * V, V, tdt, R.NAN, DEV)
    lib.upsample2x_fwd(dt, xv.data_ptr(), C + V, N, H, W, C, align, yv.data_ptr(), C + 2 * V, _st())
    torch.cuda.synchronize()
    _check("upsample2x_fwd", dtname, yv, y, mag, tdt, K_UP_FWD)
    R.assert_guard(ybuf, V, C, R.NAN, "upsample y")
    R.assert_guard(xbuf, V, C, R.SENTINEL, "upsample x")
    dy = _rnd(g, (N, 2 * H, 2 * W, C), tdt)
    dybuf, dyv = _put(dy, C + 3 * V, V)
    for accumulate in (0, 1):
        dbuf, dv, dx0, fill = _grad_out(g, (N, H, W, C), tdt, C + 2 * V, V, accumulate)
        lib.upsample2x_bwd(dt, dyv.data_ptr(), C + 3 * V, N, H, W, C, align, dv.data_ptr(), C + 2 * V, accumulate, _st())
        torch.cuda.synchronize()
        dx, m, _ = backward(dy, dx0)
        _check("upsample2x_bwd", dtname, dv, dx, m, tdt, K_UP_BWD + accumulate)
        R.assert_guard(dbuf, V, C, fill, "upsample dx")
    R.assert_guard(dybuf, V, C, R.SENTINEL, "upsample dy")
    # the adjoint with the producer ReLU's backward fused: the mask A > 0 read from a slice, slot 0 of the
    # partials = column sums of the stored dx
    A = torch.relu(torch.randn(N, H, W, C, generator=g)).to(tdt)
    abuf, av = _put(A, C + 4 * V, V)
    if 256 % (C // V):
        # header: channels / vector must divide 256 (the block's column-sum layout)
        with pytest.raises(RuntimeError, match="divide 256"):
            lib.upsample2x_bwd_relu(dt, dyv.data_ptr(), C + 3 * V, N, H, W, C, align, av.data_ptr(), C + 4 * V,
                                    dyv.data_ptr(), C + 3 * V, dyv.data_ptr(), 1, _st())
        return
    rows = lib.upsample2x_bwd_tiles(dt, N, H, W, C)
    part = torch.full((rows * 2 * C + 64,), R.SENTINEL, device=DEV)
    dbuf, dv = R.sliced((N, H, W), C, C + 2 * V, V, tdt, R.NAN, DEV)
    lib.upsample2x_bwd_relu(dt, dyv.data_ptr(), C + 3 * V, N, H, W, C, align, av.data_ptr(), C + 4 * V, dv.data_ptr(),
                            C + 2 * V, part.data_ptr(), rows, _st())
    torch.cuda.synchronize()
    dx, m, _ = backward(dy)
    on = A.to(F64) > 0
    zero = torch.zeros((), dtype=F64)
    _check("upsample2x_bwd_relu", dtname, dv, torch.where(on, dx, zero), torch.where(on, m, zero), tdt, K_UP_BWD)
    assert bool((dv.cpu()[~on] == 0).all()), "gradient where A <= 0"
    R.assert_guard(dbuf, V, C, R.NAN, "upsample_bwd_relu dx")
    R.assert_guard(abuf, V, C, R.SENTINEL, "upsample_bwd_relu A")
    R.assert_tail(part, rows * 2 * C, R.SENTINEL, "upsample_bwd_relu part")
    stored = dv.cpu().to(F64).reshape(-1, C)  # the partials sum the stored (rounded) gradient: k = pixels
    got = part[:rows * 2 * C].cpu().view(rows, 2, C)[:, 0].to(F64).sum(0)
    _check_red("upsample2x_bwd_relu colsum", dtname, N * H * W, got, stored.sum(0), stored.abs().sum(0), torch.float32,
               N * H * W)


# ------------------------------------------------------------------------------------------------
# general bilinear resize
# ------------------------------------------------------------------------------------------------
RESIZE_CASES = [(1, 1, 4, 3, 1), (3, 1, 5, 1, 1), (4, 5, 1, 1, 1), (2, 3, 37, 64, 0), (37, 64, 2, 3, 0),
                (11, 11, 31, 31, 1), (8, 10, 8, 10, 0), (9, 11, 4, 5, 0), (7, 7, 13, 20, 1)]


@pytest.mark.parametrize("h,w,oh,ow,align", RESIZE_CASES)
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_resize_bilinear(dtname, h, w, oh, ow, align):
    """out == 1 (zero scale), in == 1, a 30x upscale and downscale (the width of the backward's candidate range),
    a scale of 1/3 (fp32 products next to integers), identity; C = 5 in a pixel stride of 16 at channel 3"""
    from unetseg_hip.lib import lib
    dt, tdt, _ = _dt(dtname)
    N, C, ld, c0 = 2, 5, 16, 3
    g = _gen("resize", dtname, h, w, oh, ow)
    x = _rnd(g, (N, h, w, C), tdt)
    y, mag, backward = R.resize(x, oh, ow, bool(align))
    xbuf, xv = _put(x, ld, c0)
    ybuf, yv = R.sliced((N, oh, ow), C, ld, c0, tdt, R.NAN, DEV)
    lib.resize_bilinear_fwd(dt, xv.data_ptr(), ld, N, h, w, C, oh, ow, align, yv.data_ptr(), ld, _st())
    torch.cuda.synchronize()
    _check("resize_bilinear_fwd", dtname, yv, y, mag, tdt, R.K_RESIZE_FWD)
    R.assert_guard(ybuf, c0, C, R.NAN, "resize y")
    R.assert_guard(xbuf, c0, C, R.SENTINEL, "resize x")
    dy = _rnd(g, (N, oh, ow, C), tdt)
    dybuf, dyv = _put(dy, ld, c0)
    for accumulate in (0, 1):
        dbuf, dv, dx0, fill = _grad_out(g, (N, h, w, C), tdt, ld, c0, accumulate)
        lib.resize_bilinear_bwd(dt, dyv.data_ptr(), ld, N, h, w, C, oh, ow, align, dv.data_ptr(), ld, accumulate, _st())
        torch.cuda.synchronize()
        dx, m, kk = backward(dy, dx0)
        _check_red("resize_bilinear_bwd", dtname, kk, dv, dx, m, tdt, kk)
        R.assert_guard(dbuf, c0, C, fill, "resize dx")
    R.assert_guard(dybuf, c0, C, R.SENTINEL, "resize dy")


# ------------------------------------------------------------------------------------------------
# zero padding
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,oh,ow", [(5, 6, 8, 9), (5, 6, 5, 9), (4, 3, 4, 3)])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pad2d(dtname, h, w, oh, ow):
    from unetseg_hip.lib import lib
    dt, tdt, _ = _dt(dtname)
    N, C, ld, c0 = 2, 5, 16, 3
    for top, left in sorted({(0, 0), (min(1, oh - h), min(2, ow - w)), (oh - h, ow - w)}):
        g = _gen("pad", dtname, h, oh, ow, top, left)
        x = _rnd(g, (N, h, w, C), tdt)
        y, backward = R.pad2d(x, top, left, oh, ow)
        xbuf, xv = _put(x, ld, c0)
        ybuf, yv = R.sliced((N, oh, ow), C, ld + 1, c0, tdt, R.NAN, DEV)
        lib.pad2d_fwd(dt, xv.data_ptr(), ld, N, h, w, C, top, left, oh, ow, yv.data_ptr(), ld + 1, _st())
        torch.cuda.synchronize()
        _same(yv, y, tdt, "padded values")
        R.assert_guard(ybuf, c0, C, R.NAN, "pad y")
        R.assert_guard(xbuf, c0, C, R.SENTINEL, "pad x")
        dy = _rnd(g, (N, oh, ow, C), tdt)
        dybuf, dyv = _put(dy, ld + 1, c0)
        for accumulate in (0, 1):
            dbuf, dv, dx0, fill = _grad_out(g, (N, h, w, C), tdt, ld, c0, accumulate)
            lib.pad2d_bwd(dt, dyv.data_ptr(), ld + 1, N, h, w, C, top, left, oh, ow, dv.data_ptr(), ld, accumulate,
                          _st())
            torch.cuda.synchronize()
            dx, m, kk = backward(dy, dx0)
            if accumulate:
                _check("pad2d_bwd accumulate", dtname, dv, dx, m, tdt, kk)
            else:
                _same(dv, dx, tdt, "pad backward")
            R.assert_guard(dbuf, c0, C, fill, "pad dx")
        R.assert_guard(dybuf, c0, C, R.SENTINEL, "pad dy")
