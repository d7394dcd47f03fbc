"""GPU: per-element contract of the BatchNorm / ReLU / add kernels (csrc/elem.hip, unetseg_add in pointwise.hip,
unetseg_channel_stats in resize.hip) against the float64 references of tests/nhwc_ref.py.

Every kernel is called through the C ABI, judged alone (statistics and coefficients it reads are the float64
reference rounded to fp32) and held, element by element, to

    |got - ref| <= ulp_store(ref) + 1.01 k 2^-24 mag        (nhwc_ref.assert_elementwise)

with k the fp32 roundings of its expression.  Every activation is a channel slice of a wider buffer (c0 = V, a
different pixel stride per tensor) whose other channels hold a sentinel that must survive bit for bit.  The
shapes reach every path of the reduction geometry (elem.hip tile_geom): an odd vector count (tv = 1, 256 pixel
rows per block), channel groups, tv = 64, fewer pixels than rows, the unrolled main loop with and without a
tail, and the 256-iteration clamp.  Each test prints the largest |got - ref| / bound per operation; DESIGN.md
(section 4a) holds the table measured on an MI355X.
"""
import ctypes
import math
import os
import zlib

import pytest
import torch

import nhwc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
WORST = {}  # (operation, dtype) -> largest |got - ref| / bound seen in this module
ANY = {}  # (reduction, dtype, n) -> the same at the any-order k, printed at the end: the source of RED_MEASURED


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


def _rnd(g, shape, tdt, scale=1.0):
    """randn rounded to the storage type (CPU)"""
    return (torch.randn(*shape, generator=g) * scale).to(tdt)


def _put(t, ld, c0, fill=R.SENTINEL):
    """t [..., C] (storage type, CPU) as a channel slice of a GPU buffer of pixel stride ld -> (buf, view)"""
    buf, v = R.sliced(t.shape[:-1], t.shape[-1], ld, c0, t.dtype, fill, DEV)
    v.copy_(t)
    return buf, v


def _f32(t):
    """float64 reference statistics as the fp32 array a kernel reads (GPU), and back as the float64 it holds"""
    d = t.to(torch.float32).to(DEV).contiguous()
    return d, d.cpu().to(F64)


def _note(op, dtname, ratio):
    WORST[(op, dtname)] = max(WORST.get((op, dtname), 0.0), ratio)
    return ratio


def _check(op, dtname, got, ref, mag, store, k):
    r = _note(op, dtname, R.assert_elementwise(got, ref, mag, store, k, what=f"{op} {dtname}"))
    print(f"ratio {op} {dtname} k={k}: {r:.4g}")
    return r


def _geom(dt, M, C):
    from unetseg_hip.lib import load
    tv, ppb = ctypes.c_int(-1), ctypes.c_int(-1)
    G = load().unetseg_reduce_tiles(dt, M, C, ctypes.byref(tv), ctypes.byref(ppb))
    return G, tv.value, ppb.value


def _bn_inputs(g, M, C, tdt):
    """y with sc * y + sh away from zero: |value| >= 2^-6 by construction (a target of magnitude >= 2^-5, moved by
    the rounding of y to the storage type by less than 2^-8 (|target| + |sh|)) -> y (storage), sc, sh (fp32)"""
    sc = (torch.rand(C, generator=g) + 0.5).to(torch.float32)
    sh = ((torch.rand(C, generator=g) - 0.5) * 0.5).to(torch.float32)
    t = torch.randn(M, C, generator=g, dtype=F64)
    t = torch.where(t < 0, t - 2.0 ** -5, t + 2.0 ** -5)
    y = ((t - sh.to(F64)) / sc.to(F64)).to(torch.float32).to(tdt)
    assert float((y.to(F64) * sc.to(F64) + sh.to(F64)).abs().min()) >= 2.0 ** -6
    return y, sc, sh


# ------------------------------------------------------------------------------------------------
# bn_apply / bn_apply_mask
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmul", [1, 3, "64", 12])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res_mode", [0, 1, 2])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_bn_apply(dtname, res_mode, relu, cmul):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = 64 if cmul == "64" else cmul * V
    for M in (1, 255, 257, 1031):
        g = _gen("apply", dtname, res_mode, relu, C, M)
        y, sc, sh = _bn_inputs(g, M, C, tdt)
        r = _rnd(g, (M, C), tdt)
        sc2 = (torch.rand(C, generator=g) + 0.5).to(torch.float32)
        sh2 = (torch.randn(C, generator=g) * 0.2).to(torch.float32)
        ref, mag, bits_ref, pre = R.bn_apply(y, sc, sh, r, sc2, sh2, res_mode, relu, tdt)
        k = R.K_BN_APPLY[res_mode]
        ybuf, yv = _put(y, C + 3 * V, V)
        rbuf, rv = _put(r, C + 4 * V, V)
        d = [t.to(DEV) for t in (sc, sh, sc2, sh2)]
        rp = rv.data_ptr() if res_mode else 0
        c2 = (d[2].data_ptr(), d[3].data_ptr()) if res_mode == 2 else (0, 0)
        obuf, ov = R.sliced((M,), C, C + 5 * V, V, tdt, R.NAN, DEV)
        lib.bn_apply(dt, yv.data_ptr(), C + 3 * V, d[0].data_ptr(), d[1].data_ptr(), rp, C + 4 * V, *c2, res_mode, relu,
                     ov.data_ptr(), C + 5 * V, M, C, _st())
        torch.cuda.synchronize()
        _check(f"bn_apply res{res_mode}", dtname, ov, ref, mag, tdt, k)
        R.assert_guard(obuf, V, C, R.NAN, "bn_apply out")
        R.assert_guard(ybuf, V, C, R.SENTINEL, "bn_apply y")
        R.assert_guard(rbuf, V, C, R.SENTINEL, "bn_apply r")
        if not relu:
            continue
        mbuf, mv = R.sliced((M,), C, C + 5 * V, V, tdt, R.NAN, DEV)
        nb = M * C // V
        bits = torch.full((nb + 64,), 0xEE, dtype=torch.uint8, device=DEV)
        lib.bn_apply_mask(dt, yv.data_ptr(), C + 3 * V, d[0].data_ptr(), d[1].data_ptr(), rp, C + 4 * V, *c2, res_mode,
                          mv.data_ptr(), C + 5 * V, M, C, bits.data_ptr(), _st())
        torch.cuda.synchronize()
        _check(f"bn_apply_mask res{res_mode}", dtname, mv, ref, mag, tdt, k)
        assert torch.equal(R._bits(mv), R._bits(ov)), "bn_apply_mask stores another activation than bn_apply"
        R.assert_guard(mbuf, V, C, R.NAN, "bn_apply_mask out")
        R.assert_tail(bits, nb, 0xEE, "mbits")
        # the mask is exact except where the value itself is within its bound of zero
        near = pre.abs() < R.bound(pre, mag, tdt, k)
        assert int(near.sum()) <= 0.005 * M * C, f"{int(near.sum())} of {M * C} reference values within their bound of 0"
        got = R.unpack_mask(bits[:nb].cpu().view(M, C // V), V)
        bad = (got != R.unpack_mask(bits_ref, V)) & ~near
        assert not bool(bad.any()), (f"{int(bad.sum())} mask bits differ, first (pixel, channel) "
                                     f"{[int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]}")
        assert torch.equal(got, mv.cpu().to(F64) > 0), "mask bits are not (stored out > 0)"


# ------------------------------------------------------------------------------------------------
# bn_bwd_reduce -> bn_bwd_finalize -> bn_bwd_apply
# ------------------------------------------------------------------------------------------------
#: Worst |got - ref| / bound of every reduction this file checks, at its any-order k (k = n addends, plus the
#: roundings per addend), measured on an MI355X per (reduction, dtype, n); n is M for the pixel reductions and the
#: finalize, the tile's rows for channel_stats.  _check_red asserts the any-order bound and, where the entry is
#: below 1/50, the bound with k = 8 x ratio x k_any (nhwc_ref.k_measured): the measured value of each call is its
#: entry here.
RED_MEASURED = {
    ('bn_bwd_reduce', 'bf16', 1): 0,
    ('bn_bwd_reduce', 'bf16', 7): 0.2601,
    ('bn_bwd_reduce', 'bf16', 429): 0.001386,
    ('bn_bwd_reduce', 'bf16', 2049): 0.0001171,
    ('bn_bwd_reduce', 'bf16', 5003): 2.769e-05,
    ('bn_bwd_reduce', 'bf16', 70001): 1.476e-06,
    ('bn_bwd_reduce', 'fp32', 1): 0,
    ('bn_bwd_reduce', 'fp32', 7): 0.2398,
    ('bn_bwd_reduce', 'fp32', 429): 0.001041,
    ('bn_bwd_reduce', 'fp32', 2049): 0.0001016,
    ('bn_bwd_reduce', 'fp32', 5003): 2.388e-05,
    ('bn_finalize invstd', 'bf16', 1): 0.3468,
    ('bn_finalize invstd', 'bf16', 255): 0.04972,
    ('bn_finalize invstd', 'bf16', 256): 0.2325,
    ('bn_finalize invstd', 'bf16', 257): 0.2244,
    ('bn_finalize invstd', 'bf16', 1031): 0.06346,
    ('bn_finalize invstd', 'fp32', 1): 0.3468,
    ('bn_finalize invstd', 'fp32', 255): 0.04761,
    ('bn_finalize invstd', 'fp32', 256): 0.0489,
    ('bn_finalize invstd', 'fp32', 257): 0.02155,
    ('bn_finalize invstd', 'fp32', 1031): 0.01299,
    ('bn_finalize mean', 'bf16', 1): 0,
    ('bn_finalize mean', 'bf16', 255): 0.002595,
    ('bn_finalize mean', 'bf16', 256): 0,
    ('bn_finalize mean', 'bf16', 257): 0.002559,
    ('bn_finalize mean', 'bf16', 1031): 0.002538,
    ('bn_finalize mean', 'fp32', 1): 0,
    ('bn_finalize mean', 'fp32', 255): 0.04574,
    ('bn_finalize mean', 'fp32', 256): 0.03862,
    ('bn_finalize mean', 'fp32', 257): 0.04801,
    ('bn_finalize mean', 'fp32', 1031): 0.02333,
    ('bn_finalize running_mean', 'bf16', 1): 0.1848,
    ('bn_finalize running_mean', 'bf16', 255): 0.003664,
    ('bn_finalize running_mean', 'bf16', 256): 0.004008,
    ('bn_finalize running_mean', 'bf16', 257): 0.003753,
    ('bn_finalize running_mean', 'bf16', 1031): 0.003867,
    ('bn_finalize running_mean', 'fp32', 1): 0.1983,
    ('bn_finalize running_mean', 'fp32', 255): 0.02193,
    ('bn_finalize running_mean', 'fp32', 256): 0.02963,
    ('bn_finalize running_mean', 'fp32', 257): 0.03424,
    ('bn_finalize running_mean', 'fp32', 1031): 0.01605,
    ('bn_finalize running_var', 'bf16', 1): 0.1407,
    ('bn_finalize running_var', 'bf16', 255): 0.004582,
    ('bn_finalize running_var', 'bf16', 256): 0.008491,
    ('bn_finalize running_var', 'bf16', 257): 0.008189,
    ('bn_finalize running_var', 'bf16', 1031): 0.006233,
    ('bn_finalize running_var', 'fp32', 1): 0.1414,
    ('bn_finalize running_var', 'fp32', 255): 0.004251,
    ('bn_finalize running_var', 'fp32', 256): 0.003925,
    ('bn_finalize running_var', 'fp32', 257): 0.003745,
    ('bn_finalize running_var', 'fp32', 1031): 0.003648,
    ('channel_stats M2', 'bf16', 1): 0,
    ('channel_stats M2', 'bf16', 7): 0.1853,
    ('channel_stats M2', 'bf16', 255): 0.047,
    ('channel_stats M2', 'bf16', 256): 0.2733,
    ('channel_stats M2', 'fp32', 1): 0,
    ('channel_stats M2', 'fp32', 7): 0.1893,
    ('channel_stats M2', 'fp32', 255): 0.04935,
    ('channel_stats M2', 'fp32', 256): 0.05081,
    ('channel_stats sum', 'bf16', 1): 0,
    ('channel_stats sum', 'bf16', 7): 0,
    ('channel_stats sum', 'bf16', 255): 0,
    ('channel_stats sum', 'bf16', 256): 0,
    ('channel_stats sum', 'fp32', 1): 0,
    ('channel_stats sum', 'fp32', 7): 0.2227,
    ('channel_stats sum', 'fp32', 255): 0.04391,
    ('channel_stats sum', 'fp32', 256): 0.05415,
    ('relu_bwd_bias', 'bf16', 7): 0,
    ('relu_bwd_bias', 'bf16', 429): 0.0001461,
    ('relu_bwd_bias', 'bf16', 5003): 8.027e-06,
    ('relu_bwd_bias', 'fp32', 7): 0.1947,
    ('relu_bwd_bias', 'fp32', 429): 0.0006844,
    ('relu_bwd_bias', 'fp32', 5003): 2.014e-05,
}


def _check_red(op, dtname, n, got, ref, mag, k_any):
    """a reduction of n addends: the any-order bound, then the measured-ratio bound where RED_MEASURED has one"""
    r = R.assert_elementwise(got, ref, mag, torch.float32, k_any, what=f"{op} {dtname} n={n} (any order)")
    key = (op, dtname, n)
    ANY[key] = max(ANY.get(key, 0.0), r)
    print(f"ratio {op} {dtname} n={n} any-order k={k_any}: {r:.4g}")
    k = R.k_measured(k_any, RED_MEASURED.get(key))
    if k != k_any:
        _check(f"{op} n={n}", dtname, got, ref, mag, torch.float32, k)
    else:
        _note(f"{op} n={n}", dtname, r)


def _bn_bwd_case(dtname, mode, has_y2, dzmode, C, M, seed=0, apply=True):
    """one BN backward through all three kernels (apply=False: the reduce and the finalize only)"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    g = _gen("bwd", dtname, C, M, seed)
    y1, msc, msh = _bn_inputs(g, M, C, tdt)
    dA, y2 = _rnd(g, (M, C), tdt), _rnd(g, (M, C), tdt, 2.0)
    mask = (y1.to(F64) * msc.to(F64) + msh.to(F64)) > 0
    st1, st2 = R.batch_stats(y1), R.batch_stats(y2)
    (mean1, m1), (inv1, i1) = _f32(st1[0]), _f32(1 / torch.sqrt(st1[1] + 1e-5))
    (mean2, m2), (inv2, i2) = _f32(st2[0]), _f32(1 / torch.sqrt(st2[1] + 1e-5))
    (g1, g1h), (g2, g2h) = _f32(torch.rand(C, generator=g) + 0.5), _f32(torch.rand(C, generator=g) + 0.5)
    nb = 2 if has_y2 else 1
    # dy from the reference's coefficients rounded to fp32: the table pass 3 is handed below
    ref = R.bn_bwd(dA, mask if mode else None, y1, m1, i1, y2 if has_y2 else None, m2, i2, g1h, g2h, M,
                   round_coef=True, want_dy=apply)
    # the mask source
    dbuf, dv = _put(dA, C + 3 * V, V)
    y1buf, y1v = _put(y1, C + 4 * V, V)
    y2buf, y2v = _put(y2, C + 5 * V, V)
    dsc, dsh = msc.to(DEV), msh.to(DEV)
    A, lda, mp = 0, 0, (0, 0)
    abuf = None
    if mode == 1:
        act = R.round_store(R.bn_apply(y1, msc, msh, None, None, None, 0, 1, tdt)[0], tdt)
        abuf, av = _put(act, C + 2 * V, V)
        A, lda = av.data_ptr(), C + 2 * V
    elif mode == 2:
        mp = (dsc.data_ptr(), dsh.data_ptr())
    elif mode == 3:  # the packed (contiguous) bytes of a real bn_apply_mask call
        scratch = torch.empty(M, C, dtype=tdt, device=DEV)
        bits = torch.full((M * C // V + 64,), 0xEE, dtype=torch.uint8, device=DEV)
        lib.bn_apply_mask(dt, y1v.data_ptr(), C + 4 * V, dsc.data_ptr(), dsh.data_ptr(), 0, 0, 0, 0, 0,
                          scratch.data_ptr(), C, M, C, bits.data_ptr(), _st())
        torch.cuda.synchronize()
        assert torch.equal(bits[:M * C // V].cpu().view(M, C // V), R.pack_mask(mask, V))
        A, lda = bits.data_ptr(), 0
    y2a = (y2v.data_ptr(), C + 5 * V, mean2.data_ptr(), inv2.data_ptr()) if has_y2 else (0, 0, 0, 0)
    # pass 1
    G, tv, ppb = _geom(dt, M, C)
    nq = 1 + nb
    part = torch.full((nq * C * G + 64,), R.SENTINEL, device=DEV)
    lib.bn_bwd_reduce(dt, dv.data_ptr(), C + 3 * V, A, lda, *mp, y1v.data_ptr(), C + 4 * V, mean1.data_ptr(),
                      inv1.data_ptr(), *y2a, M, C, part.data_ptr(), G, _st())
    torch.cuda.synchronize()
    R.assert_tail(part, nq * C * G, R.SENTINEL, "bn_bwd_reduce part")
    pg = part[:nq * C * G].cpu().view(nq, C, G)
    psum = pg.to(F64).sum(2)
    for q in range(nq):
        _check_red("bn_bwd_reduce", dtname, M, psum[q], ref["sums"][q], ref["sums_mag"][q], ref["k_sums"][q])
    # pass 2, on the partials pass 1 wrote: dgamma / dbeta accumulated onto non-zero values, the coefficient table
    grads0 = [torch.randn(C, generator=g).to(torch.float32) for _ in range(4)]
    dg1, db1, dg2, db2 = (t.to(DEV) for t in grads0)
    coef = torch.full((6 * C + 64,), R.SENTINEL, device=DEV)
    b2 = (g2.data_ptr(), inv2.data_ptr(), dg2.data_ptr(), db2.data_ptr()) if has_y2 else (0, 0, 0, 0)
    lib.bn_bwd_finalize(part.data_ptr(), C, G, M, nb, g1.data_ptr(), inv1.data_ptr(), dg1.data_ptr(), db1.data_ptr(),
                        *b2, coef.data_ptr(), _st())
    torch.cuda.synchronize()
    R.assert_tail(coef, 3 * nb * C, R.SENTINEL, "bn_bwd_finalize coef")
    cg = coef[:3 * nb * C].cpu().view(3 * nb, C)
    want_g = [(dg1, 1, 0), (db1, 0, 1)] + ([(dg2, 2, 2), (db2, 0, 3)] if has_y2 else [])
    for got, q, j in want_g:  # k = 2: the fp64 total cast to fp32, the add
        v, m = R.colsum(pg[q].t(), 1, grads0[j])
        _check("bn_bwd_finalize dgamma/dbeta", dtname, got, v, m, torch.float32, 2)
    for b in range(nb):  # k = 1: one product / one quotient, rounded once
        gi = (g1h * i1, g2h * i2)[b]
        _check("bn_bwd_finalize coef", dtname, cg[3 * b], gi, gi.abs(), torch.float32, 1)
        _check("bn_bwd_finalize coef", dtname, cg[3 * b + 1], psum[0] / M, (psum[0] / M).abs(), torch.float32, 1)
        _check("bn_bwd_finalize coef", dtname, cg[3 * b + 2], psum[1 + b] / M, (psum[1 + b] / M).abs(),
               torch.float32, 1)
    if not apply:
        return
    # pass 3, from the reference's coefficients rounded to fp32
    cfull = torch.zeros(6, C, dtype=F64)
    cfull[:3 * nb] = ref["coef_used"]
    cdev, _ = _f32(cfull)
    o1buf, o1v = R.sliced((M,), C, C + 6 * V, V, tdt, R.NAN, DEV)
    o2buf, o2v = R.sliced((M,), C, C + 7 * V, V, tdt, R.NAN, DEV)
    dz0 = _rnd(g, (M, C), tdt)
    zbuf, zv = _put(dz0, C + 8 * V, V, R.SENTINEL if dzmode == 2 else R.NAN)
    if dzmode != 2:
        zbuf.fill_(R.NAN)
    y2b = (y2v.data_ptr(), C + 5 * V, mean2.data_ptr(), inv2.data_ptr(), o2v.data_ptr(), C + 7 * V) if has_y2 else \
        (0, 0, 0, 0, 0, 0)
    lib.bn_bwd_apply(dt, dv.data_ptr(), C + 3 * V, A, lda, *mp, y1v.data_ptr(), C + 4 * V, mean1.data_ptr(),
                     inv1.data_ptr(), o1v.data_ptr(), C + 6 * V, *y2b, cdev.data_ptr(), zv.data_ptr() if dzmode else 0,
                     C + 8 * V, int(dzmode == 2), M, C, _st())
    torch.cuda.synchronize()
    _check("bn_bwd_apply dy1", dtname, o1v, ref["dy1"], ref["dy1_mag"], tdt, R.K_BN_DY)
    R.assert_guard(o1buf, V, C, R.NAN, "dy1")
    if has_y2:
        _check("bn_bwd_apply dy2", dtname, o2v, ref["dy2"], ref["dy2_mag"], tdt, R.K_BN_DY)
    R.assert_guard(o2buf, V, C if has_y2 else 0, R.NAN, "dy2")
    if dzmode == 1:
        assert torch.equal(R._bits(zv.cpu()), R._bits(R.round_store(ref["dz"], tdt))), "dzout (store) is not dA * mask"
    elif dzmode == 2:
        v, m = R.add(ref["dz"], dz0)
        _check("bn_bwd_apply dz accumulate", dtname, zv, v, m, tdt, R.K_DZ_ACC)
    R.assert_guard(zbuf, V, C if dzmode else 0, R.SENTINEL if dzmode == 2 else R.NAN, "dzout")
    for buf, what in ((dbuf, "dA"), (y1buf, "y1"), (y2buf, "y2")) + (((abuf, "A"),) if abuf is not None else ()):
        R.assert_guard(buf, V, C, R.SENTINEL, what)


@pytest.mark.parametrize("dzmode", [0, 1, 2])
@pytest.mark.parametrize("has_y2", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_bn_bwd_cross(dtname, mode, has_y2, dzmode):
    """every mask mode x second branch x dz mode instantiation of the reduce and apply kernels, C = 64, M = 429"""
    _bn_bwd_case(dtname, mode, has_y2, dzmode, 64, 429)


SWEEP_C = {"bf16": (8, 24, 64, 96, 512, 1024), "fp32": (4, 12, 64, 256, 512)}
SWEEP_M = (1, 7, 429, 2049, 5003)


@pytest.mark.parametrize("dtname,C", [(d, c) for d in SWEEP_C for c in SWEEP_C[d]])
def test_bn_bwd_geometry_sweep(dtname, C):
    for M in SWEEP_M:
        _bn_bwd_case(dtname, 1, True, 2, C, M)


def test_sweep_reaches_the_geometry():
    """the sweep holds, for every C, a case with >= 3 pixel blocks whose last is ragged, and a case with fewer
    pixels than the block has rows; over the C it holds tv = 1 (odd vector count), channel groups and tv = 64"""
    seen = set()
    for dtname in SWEEP_C:
        dt, _, V = _dt(dtname)
        for C in SWEEP_C[dtname]:
            geo = {M: _geom(dt, M, C) for M in SWEEP_M}
            assert any(G >= 3 and M % ppb != 0 for M, (G, tv, ppb) in geo.items()), (dtname, C, geo)
            assert any(M < 256 // tv for M, (G, tv, ppb) in geo.items()), (dtname, C, geo)
            tv = geo[1][1]
            seen.add(("tv1", tv == 1))
            seen.add(("groups", C // V // tv > 1))
            seen.add(("tv64", tv == 64))
    assert {("tv1", True), ("groups", True), ("tv64", True)} <= seen


def test_bn_bwd_per_clamp():
    """C = 512, M = 70001 under UNETSEG_RED_TARGET=64 (read at every call): the pixel rows one thread walks hit the
    clamp at 256.  The knob moves the reduction's geometry only (the apply pass has its own), so the case stops
    after the finalize."""
    dt, _, V = _dt("bf16")
    before = os.environ.get("UNETSEG_RED_TARGET")
    os.environ["UNETSEG_RED_TARGET"] = "64"
    try:
        G, tv, ppb = _geom(dt, 70001, 512)
        rows = 256 // tv
        assert math.ceil(70001 / (rows * 64)) > 256 and ppb == rows * 256 and G == math.ceil(70001 / ppb)
        _bn_bwd_case("bf16", 1, True, 2, 512, 70001, apply=False)
    finally:
        if before is None:
            os.environ.pop("UNETSEG_RED_TARGET", None)
        else:
            os.environ["UNETSEG_RED_TARGET"] = before


@pytest.mark.parametrize("has_y2", [False, True])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_bn_bwd_mask_modes_bit_identical(dtname, has_y2):
    """with A = the bn_apply_mask output of the same y1 (res_mode 0), the partials under the activation mask, the
    recomputed mask and the packed bits are bit-identical (elem.hip: "== bwd mask recompute", "the same rounding
    in every MASK / Y2 instantiation")"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C, M = 64, 429
    g = _gen("ident", dtname, has_y2)
    y1, msc, msh = _bn_inputs(g, M, C, tdt)
    dA, y2 = _rnd(g, (M, C), tdt), _rnd(g, (M, C), tdt)
    mean, inv = (torch.randn(C, generator=g) * 0.1).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    ybuf, yv = _put(y1, C + 3 * V, V)
    _, dv = _put(dA, C + 4 * V, V)
    _, y2v = _put(y2, C + 5 * V, V)
    abuf, av = R.sliced((M,), C, C + 2 * V, V, tdt, R.NAN, DEV)
    bits = torch.empty(M * C // V, dtype=torch.uint8, device=DEV)
    dsc, dsh = msc.to(DEV), msh.to(DEV)
    lib.bn_apply_mask(dt, yv.data_ptr(), C + 3 * V, dsc.data_ptr(), dsh.data_ptr(), 0, 0, 0, 0, 0, av.data_ptr(),
                      C + 2 * V, M, C, bits.data_ptr(), _st())
    G, _, _ = _geom(dt, M, C)
    nq = 3 if has_y2 else 2
    y2a = (y2v.data_ptr(), C + 5 * V, mean.data_ptr(), inv.data_ptr()) if has_y2 else (0, 0, 0, 0)
    parts = []
    for A, lda, mp in ((av.data_ptr(), C + 2 * V, (0, 0)), (0, 0, (dsc.data_ptr(), dsh.data_ptr())),
                       (bits.data_ptr(), 0, (0, 0))):
        part = torch.full((nq, C, G), R.NAN, device=DEV)
        lib.bn_bwd_reduce(dt, dv.data_ptr(), C + 4 * V, A, lda, *mp, yv.data_ptr(), C + 3 * V, mean.data_ptr(),
                          inv.data_ptr(), *y2a, M, C, part.data_ptr(), G, _st())
        torch.cuda.synchronize()
        parts.append(part.view(torch.int32).cpu())
    assert torch.equal(parts[0], parts[1]), "activation mask vs recomputed mask"
    assert torch.equal(parts[0], parts[2]), "activation mask vs packed bits"


# ------------------------------------------------------------------------------------------------
# relu_bwd_bias -> colsum_finalize, colsum_rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtname,C", [(d, c) for d in SWEEP_C for c in SWEEP_C[d]])
def test_relu_bwd_bias_colsum(dtname, C, accumulate):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    for M in (7, 429, 5003):
        g = _gen("relu", dtname, C, M)
        dA, A = _rnd(g, (M, C), tdt), torch.relu(torch.randn(M, C, generator=g)).to(tdt)
        dY, s, smag = R.relu_bwd_bias(dA, A)
        dbuf, dv = _put(dA, C + 3 * V, V)
        abuf, av = _put(A, C + 4 * V, V)
        obuf, ov = R.sliced((M,), C, C + 5 * V, V, tdt, R.NAN, DEV)
        G, _, _ = _geom(dt, M, C)
        part = torch.full((C * G + 64,), R.SENTINEL, device=DEV)
        lib.relu_bwd_bias(dt, dv.data_ptr(), C + 3 * V, av.data_ptr(), C + 4 * V, ov.data_ptr(), C + 5 * V, M, C,
                          part.data_ptr(), G, _st())
        torch.cuda.synchronize()
        assert torch.equal(R._bits(ov.cpu()), R._bits(R.round_store(dY, tdt))), "dY is not dA where A > 0"
        R.assert_guard(obuf, V, C, R.NAN, "dY")
        R.assert_guard(dbuf, V, C, R.SENTINEL, "dA")
        R.assert_guard(abuf, V, C, R.SENTINEL, "A")
        R.assert_tail(part, C * G, R.SENTINEL, "relu_bwd_bias part")
        pg = part[:C * G].cpu().view(C, G)
        _check_red("relu_bwd_bias", dtname, M, pg.to(F64).sum(1), s, smag, M)
        out0 = torch.randn(C, generator=g).to(torch.float32)
        out = torch.full((C + 64,), R.SENTINEL, device=DEV)
        out[:C] = out0.to(DEV)
        lib.colsum_finalize(part.data_ptr(), C, G, out.data_ptr(), accumulate, _st())
        torch.cuda.synchronize()
        v, m = R.colsum(pg.t(), accumulate, out0)
        _check("colsum_finalize", dtname, out[:C], v, m, torch.float32, 2)
        R.assert_tail(out, C, R.SENTINEL, "colsum_finalize out")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("C,G", [(3, 1), (64, 65), (260, 513), (7, 2100)])
def test_colsum_rows(C, G, k, accumulate):
    """out[c] (+)= sum_g part[g][k][c] over row partials [G][2][C]: one wave per channel up to 512 rows, a block
    above, several rounds past 2048"""
    from unetseg_hip.lib import lib
    g = _gen("rows", C, G)
    part = torch.randn(G, 2, C, generator=g)
    out0 = torch.randn(C, generator=g)
    out = torch.full((C + 64,), R.SENTINEL, device=DEV)
    out[:C] = out0.to(DEV)
    dpart = part.to(DEV)
    lib.colsum_rows(dpart.data_ptr(), C, G, k, out.data_ptr(), accumulate, _st())
    torch.cuda.synchronize()
    v, m = R.colsum(part[:, k], accumulate, out0)
    _check("colsum_rows", "fp32", out[:C], v, m, torch.float32, 2)
    R.assert_tail(out, C, R.SENTINEL, "colsum_rows out")
    assert torch.equal(dpart.cpu(), part)


# ------------------------------------------------------------------------------------------------
# channel_stats -> bn_finalize
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", ["V", 3, 20, 260])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_channel_stats_finalize(dtname, cname):
    """x = 3 + 0.5 randn (a sum-of-squares variance would lose half its digits), ld = C + 5, tile = 256"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = V if cname == "V" else cname
    tile, eps, mom = 256, 1e-5, 0.1
    for M in (1, 255, 256, 257, 1031):
        g = _gen("stats", dtname, C, M)
        x = (3 + 0.5 * torch.randn(M, C, generator=g)).to(tdt)
        xbuf, xv = _put(x, C + 5, 2)
        G = lib.channel_stats_tiles(M, tile)
        pref, pmag, ks = R.channel_stats(x, tile)
        assert G == len(ks)
        part = torch.full((G * 2 * C + 64,), R.SENTINEL, device=DEV)
        lib.channel_stats(dt, xv.data_ptr(), C + 5, M, C, tile, part.data_ptr(), _st())
        torch.cuda.synchronize()
        R.assert_tail(part, G * 2 * C, R.SENTINEL, "channel_stats part")
        R.assert_guard(xbuf, 2, C, R.SENTINEL, "channel_stats x")
        pg = part[:G * 2 * C].cpu().view(G, 2, C)
        for t in range(G):
            _check_red("channel_stats sum", dtname, ks[t], pg[t, 0], pref[t, 0], pmag[t, 0], ks[t])
            _check_red("channel_stats M2", dtname, ks[t], pg[t, 1], pref[t, 1], pmag[t, 1], ks[t] + 3)
        # the finalize on these partials against the full-M statistics
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        dgam, dbet, rm, rv = (t.to(DEV) for t in (gam, bet, rm0, rv0))
        nbt = torch.full((1,), 41, dtype=torch.int64, device=DEV)
        outs = torch.full((4, C), R.NAN, device=DEV)
        lib.bn_finalize(part.data_ptr(), C, G, M, tile, dgam.data_ptr(), dbet.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                        nbt.data_ptr(), mom, eps, *(outs[i].data_ptr() for i in range(4)), _st())
        torch.cuda.synchronize()
        assert int(nbt) == 42
        mean, var = R.batch_stats(x)
        fin = R.bn_finalize(mean, var, M, gam, bet, rm0, rv0, mom, eps)
        n = min(M, tile)
        xa = x.to(F64).abs().mean(0)
        # the mean: n adds per tile partial, the fp64 merge rounded once -> n + 1
        _check_red("bn_finalize mean", dtname, M, outs[0], mean, xa, n + 1)
        # the variance inherits (n + 3) roundings of the M2 partials, and the tile sums' error (n roundings of a
        # tile's mean |x|) through Chan's term cnt (mean_g - mean)^2, i.e. times 2 max_g |mean_g - mean|
        tmean = torch.stack([x[t * tile:(t + 1) * tile].to(F64).mean(0) for t in range(G)])
        vmag = var + 2 * (tmean - mean).abs().max(0).values * xa
        d_inv = 0.5 * fin["invstd"] / (var + eps)  # |d invstd / d var|
        _check_red("bn_finalize invstd", dtname, M, outs[1], fin["invstd"], d_inv * vmag + fin["invstd"] / (n + 4),
                   n + 4)
        unb = M / (M - 1) if M > 1 else 1.0
        _check_red("bn_finalize running_mean", dtname, M, rm, fin["rmean"], (1 - mom) * rm0.to(F64).abs() + mom * xa,
                   n + 2)
        _check_red("bn_finalize running_var", dtname, M, rv, fin["rvar"],
                   (1 - mom) * rv0.to(F64).abs() + mom * unb * vmag, n + 4)


# ------------------------------------------------------------------------------------------------
# bn_eval_coeffs, bn_fold
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("C", [1, 7, 64, 300])
def test_bn_eval_coeffs_and_fold(C, with_bias):
    from unetseg_hip.lib import lib
    g = _gen("eval", C)
    gam, bet, rm = (torch.randn(C, generator=g) for _ in range(3))
    rv, cb = torch.rand(C, generator=g) + 0.05, torch.randn(C, generator=g)
    d = [t.to(DEV) for t in (gam, bet, rm, rv, cb)]
    eps = 1e-5
    sc, sh, mag = R.bn_eval_coeffs(gam, bet, rm, rv, eps)
    out = torch.full((2, C + 64), R.SENTINEL, device=DEV)
    lib.bn_eval_coeffs(C, *(t.data_ptr() for t in d[:4]), eps, out[0].data_ptr(), out[1].data_ptr(), _st())
    torch.cuda.synchronize()
    _check("bn_eval_coeffs scale", "fp32", out[0, :C], sc, sc.abs(), torch.float32, 4)
    _check("bn_eval_coeffs shift", "fp32", out[1, :C], sh, mag, torch.float32, 8)
    R.assert_tail(out[0], C, R.SENTINEL, "scale")
    R.assert_tail(out[1], C, R.SENTINEL, "shift")
    sc, sh, mag = R.bn_eval_coeffs(gam, bet, rm, rv, eps, cb if with_bias else None)
    fold = torch.full((2, C + 64), R.SENTINEL, device=DEV)
    lib.bn_fold(C, *(t.data_ptr() for t in d[:4]), eps, d[4].data_ptr() if with_bias else 0, fold[0].data_ptr(),
                fold[1].data_ptr(), _st())
    torch.cuda.synchronize()
    _check("bn_fold kscale", "fp32", fold[0, :C], sc, sc.abs(), torch.float32, 4)
    _check("bn_fold bias", "fp32", fold[1, :C], sh, mag, torch.float32, 8)
    R.assert_tail(fold[0], C, R.SENTINEL, "kscale")
    R.assert_tail(fold[1], C, R.SENTINEL, "bias")
    if not with_bias:  # elem.hip: the same float expressions in both kernels
        assert torch.equal(fold[:, :C].view(torch.int32), out[:, :C].view(torch.int32))


# ------------------------------------------------------------------------------------------------
# unetseg_add
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 1031])
@pytest.mark.parametrize("cmul", [1, 3, 8])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_add_into_slice(dtname, cmul, M):
    """out += x with both sides channel slices: the result adds into what `out` held (copy_into and
    bn_relu_prefix rely on it), the neighbouring channels stay"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cmul * V
    g = _gen("add", dtname, C, M)
    x, o0 = _rnd(g, (M, C), tdt), _rnd(g, (M, C), tdt)
    xbuf, xv = _put(x, C + 3 * V, V)
    obuf, ov = _put(o0, C + 4 * V, 2 * V)
    lib.add(dt, xv.data_ptr(), C + 3 * V, ov.data_ptr(), C + 4 * V, M, C, _st())
    torch.cuda.synchronize()
    v, m = R.add(x, o0)
    _check("add", dtname, ov, v, m, tdt, 1)
    assert float((ov.cpu().to(F64) - x.to(F64)).abs().max()) > 0.1 or M * C < 16, "the result ignores what out held"
    R.assert_guard(obuf, 2 * V, C, R.SENTINEL, "add out")
    R.assert_guard(xbuf, V, C, R.SENTINEL, "add x")
    assert torch.equal(R._bits(xv.cpu()), R._bits(x)), "add changed its input"
