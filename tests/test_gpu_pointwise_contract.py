"""GPU: per-element contract of the narrow 1x1 head kernels (pw_small_*, pw_head_*), the attention gate (attn_*),
global average pooling (gap_*) and the input packers (csrc/pointwise.hip, the strided half of csrc/cls_head.hip)
against the float64 references of tests/nhwc_ref.py.  The contract is stated in include/unetseg_hip.h ("the
pointwise contract"); DESIGN.md section 4c holds the case table and the measured tables.

Every kernel is called through the C ABI and judged alone, element by element, by

    |got - ref| <= ulp_store(ref) + 1.01 k 2^-24 mag        (nhwc_ref.assert_elementwise)

with k counted beside each check.  Every case runs twice on the same values: packed (ld == C) and strided, where
each NHWC operand is a channel slice of its own wider buffer (operand i: c0 = (1 + i) V, ld = C + (3 + i) V, so
no two strides agree and none is C).  The two runs must agree bit for bit inside the slices; the channels beside
a slice, one guard pixel before and after every NHWC operand and 64 elements past the end of every planar or
partial array must keep their fill.  Outputs that are written start as NaN, accumulated ones from random data.

Pixel counts M = 1, 5, 127, 128, 129 (three images of 43 pixels) and 389: every tile of the small-head and
attention kernels is 128 pixels there (asserted through the tile queries), so these are one ragged tile, a
full one, a full one and one pixel, and three full ones and five pixels -- the last tile, the last group of
four pixel passes and, for the planar outputs, a tile that spans images.  The larger tiles only change one
kernel argument and stay with tests/test_gpu_c4c5.py.
"""
import math
import zlib

import pytest
import torch

import nhwc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
F32 = torch.float32
TAIL = 64
#: (M, images): the planar outputs are [N][K][M / N]
PIXELS = [(1, 1), (5, 1), (127, 1), (128, 1), (129, 3), (389, 1)]
WORST = {}  # (operation, dtype) -> largest |got - ref| / bound seen in this module
ANY = {}  # (reduction, dtype, n) -> the same at the any-order k, printed at the end: the source of RED_MEASURED
ALPHA = {}  # dtype -> largest error of alpha in fp32 ulps, printed at the end: the source of ALPHA_ULPS_MEASURED

#: Worst |got - ref| / bound of the fp32 reductions over a tile's n pixels at their any-order k, measured on an
#: MI355X against the float64 reference per (reduction, dtype, n) -- the convention of test_gpu_elem_contract.py:
#: _check_red asserts the any-order bound and, where the entry is below 1/50, the bound with k = 8 x ratio x k_any.
RED_MEASURED = {
    ('attn_bwd2 part_b', 'bf16', 1): 0.1581,
    ('attn_bwd2 part_b', 'bf16', 5): 0.07207,
    ('attn_bwd2 part_b', 'bf16', 127): 0.002951,
    ('attn_bwd2 part_b', 'bf16', 128): 0.01059,
    ('attn_bwd2 part_b', 'fp32', 1): 0.2543,
    ('attn_bwd2 part_b', 'fp32', 5): 0.1002,
    ('attn_bwd2 part_b', 'fp32', 127): 0.01216,
    ('attn_bwd2 part_b', 'fp32', 128): 0.00654,
    ('attn_bwd2 part_w', 'bf16', 1): 0.2469,
    ('attn_bwd2 part_w', 'bf16', 5): 0.215,
    ('attn_bwd2 part_w', 'bf16', 127): 0.01601,
    ('attn_bwd2 part_w', 'bf16', 128): 0.02517,
    ('attn_bwd2 part_w', 'fp32', 1): 0.3698,
    ('attn_bwd2 part_w', 'fp32', 5): 0.1525,
    ('attn_bwd2 part_w', 'fp32', 127): 0.02041,
    ('attn_bwd2 part_w', 'fp32', 128): 0.02271,
    ('pw_head_bwd part_b', 'bf16', 1): 0,
    ('pw_head_bwd part_b', 'bf16', 5): 0.1849,
    ('pw_head_bwd part_b', 'bf16', 127): 0.009424,
    ('pw_head_bwd part_b', 'bf16', 128): 0.009225,
    ('pw_head_bwd part_b', 'bf16', 129): 0.007356,
    ('pw_head_bwd part_b', 'bf16', 389): 0.004451,
    ('pw_head_bwd part_b', 'fp32', 1): 0,
    ('pw_head_bwd part_b', 'fp32', 5): 0.1961,
    ('pw_head_bwd part_b', 'fp32', 127): 0.007544,
    ('pw_head_bwd part_b', 'fp32', 128): 0.006522,
    ('pw_head_bwd part_b', 'fp32', 129): 0.009445,
    ('pw_head_bwd part_b', 'fp32', 389): 0.00321,
    ('pw_head_bwd part_w', 'bf16', 1): 0.2475,
    ('pw_head_bwd part_w', 'bf16', 5): 0.3151,
    ('pw_head_bwd part_w', 'bf16', 127): 0.03513,
    ('pw_head_bwd part_w', 'bf16', 128): 0.02304,
    ('pw_head_bwd part_w', 'bf16', 129): 0.02662,
    ('pw_head_bwd part_w', 'bf16', 389): 0.008122,
    ('pw_head_bwd part_w', 'fp32', 1): 0.2482,
    ('pw_head_bwd part_w', 'fp32', 5): 0.312,
    ('pw_head_bwd part_w', 'fp32', 127): 0.02392,
    ('pw_head_bwd part_w', 'fp32', 128): 0.02533,
    ('pw_head_bwd part_w', 'fp32', 129): 0.02697,
    ('pw_head_bwd part_w', 'fp32', 389): 0.00936,
    ('pw_small_bwd part_b', 'bf16', 1): 0,
    ('pw_small_bwd part_b', 'bf16', 5): 0.2213,
    ('pw_small_bwd part_b', 'bf16', 127): 0.002927,
    ('pw_small_bwd part_b', 'bf16', 128): 0.005833,
    ('pw_small_bwd part_b', 'fp32', 1): 0,
    ('pw_small_bwd part_b', 'fp32', 5): 0.3233,
    ('pw_small_bwd part_b', 'fp32', 127): 0.00722,
    ('pw_small_bwd part_b', 'fp32', 128): 0.008443,
    ('pw_small_bwd part_w', 'bf16', 1): 0.2448,
    ('pw_small_bwd part_w', 'bf16', 5): 0.2925,
    ('pw_small_bwd part_w', 'bf16', 127): 0.02637,
    ('pw_small_bwd part_w', 'bf16', 128): 0.03218,
    ('pw_small_bwd part_w', 'fp32', 1): 0.2464,
    ('pw_small_bwd part_w', 'fp32', 5): 0.3485,
    ('pw_small_bwd part_w', 'fp32', 127): 0.02405,
    ('pw_small_bwd part_w', 'fp32', 128): 0.02515,
    ('pw_small_bwd_relu part_b', 'bf16', 1): 0,
    ('pw_small_bwd_relu part_b', 'bf16', 5): 0.1417,
    ('pw_small_bwd_relu part_b', 'bf16', 127): 0.005298,
    ('pw_small_bwd_relu part_b', 'bf16', 128): 0.0113,
    ('pw_small_bwd_relu part_d', 'bf16', 1): 0,
    ('pw_small_bwd_relu part_d', 'bf16', 5): 0,
    ('pw_small_bwd_relu part_d', 'bf16', 127): 0.001542,
    ('pw_small_bwd_relu part_d', 'bf16', 128): 0.002132,
    ('pw_small_bwd_relu part_w', 'bf16', 1): 0.362,
    ('pw_small_bwd_relu part_w', 'bf16', 5): 0.2959,
    ('pw_small_bwd_relu part_w', 'bf16', 127): 0.02044,
    ('pw_small_bwd_relu part_w', 'bf16', 128): 0.03149,
}

#: largest error of alpha = 1 / (1 + expf(-z)) against the float64 sigmoid of the same (exactly formed) z, in fp32
#: ulps, measured on an MI355X (bf16 cases 1.723, fp32 cases 1.544: the same fp32 arithmetic on other psi);
#: test_attn_apply asserts twice that, rounded up to a whole ulp: 4 ulps, 4.8e-7 relative
ALPHA_ULPS_MEASURED = 1.723
ALPHA_ULPS = math.ceil(2 * ALPHA_ULPS_MEASURED)


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
    for dt, u in sorted(ALPHA.items()):
        print(f"\nalpha ulps   {dt}: {u:.4g}", end="")
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


class Op:
    """An NHWC operand [M][C] on the GPU with one guard pixel on either side: packed (ld == C) or, strided, the
    channel slice [c0, c0 + C) of a buffer of pixel stride ld, c0 = (1 + i) V and ld = C + (3 + i) V for operand
    number i.  t: its content (an input, or the start of an accumulated output), or None for an output that is
    written (NaN everywhere)."""

    def __init__(self, t, strided, i, shape=None, dtype=None):
        M, C = shape if t is None else t.shape
        tdt = dtype if t is None else t.dtype
        V = R.VEC[tdt]
        self.ld, self.c0 = (C + (3 + i) * V, (1 + i) * V) if strided else (C, 0)
        self.C, self.fill = C, (R.NAN if t is None else R.SENTINEL)
        self.buf = torch.full((M + 2, self.ld), self.fill, dtype=tdt, device=DEV)
        self.v = self.buf[1:M + 1, self.c0:self.c0 + C]
        if t is not None:
            self.v.copy_(t)
        self.ptr = self.v.data_ptr()

    def get(self):
        return self.v.cpu()

    def guard(self, what):
        """the channels beside the slice and the guard pixels keep their fill, bit for bit"""
        R.assert_guard(self.buf[1:-1], self.c0, self.C, self.fill, what)
        R.assert_guard(self.buf[[0, -1]], 0, 0, self.fill, what + " (the pixel before / after the tensor)")


class Flat:
    """a dense fp32 (or storage-type) output of n elements, NaN, with TAIL elements behind it that must stay NaN"""

    def __init__(self, n, dtype=F32):
        self.n = n
        self.buf = torch.full((n + TAIL,), R.NAN, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr()

    def get(self, *shape):
        return self.buf[:self.n].cpu().reshape(*shape)

    def guard(self, what):
        R.assert_tail(self.buf, self.n, R.NAN, what)


def _dev(t):
    return t.to(DEV).contiguous()


def _note(op, dtname, ratio):
    WORST[(op, dtname)] = max(WORST.get((op, dtname), 0.0), ratio)
    return ratio


def _check(op, dtname, got, ref, mag, store, k):
    r = _note(op, dtname, R.assert_elementwise(got, ref, mag, store, k, what=f"{op} {dtname}"))
    print(f"ratio {op} {dtname} k={k:.4g}: {r:.4g}")
    return r


def _check_red(op, dtname, n, got, ref, mag, k_any):
    """an fp32 reduction of n addends: the any-order bound, then the measured-ratio bound where RED_MEASURED has one"""
    r = R.assert_elementwise(got, ref, mag, F32, k_any, what=f"{op} {dtname} n={n} (any order)")
    key = (op, dtname, n)
    ANY[key] = max(ANY.get(key, 0.0), r)
    print(f"ratio {op} {dtname} n={n} any-order k={k_any}: {r:.4g}")
    k = R.k_measured(k_any, RED_MEASURED.get(key))
    if k != k_any:
        _check(f"{op} n={n}", dtname, got, ref, mag, F32, k)
    else:
        _note(f"{op} n={n}", dtname, r)


def _same(a, b, what):
    """the packed and the strided run agree bit for bit"""
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(R._bits(a[k]), R._bits(b[k])), f"{what}: {k} differs between the packed and the strided run"


def _twice(run, what):
    a, b = run(False), run(True)
    _same(a, b, what)
    return a


def _tiles128(M):
    """every tile of the small-head / attention kernels is 128 pixels at these M"""
    from unetseg_hip.lib import lib
    G = (M + 127) // 128
    assert lib.pw_small_tile(M) == 128 and lib.pw_small_tiles(M) == G and lib.attn_bwd1_tiles(M) == G
    assert lib.pw_head_tiles(M) == 1  # the C-way head's partial tile is 2048 pixels: one tile, n = M
    return G


def _per_tile(op, dtname, ns, got, ref, mag, k_of_n):
    """got / ref / mag [..., G]: each partial slot against the float64 sum over that tile's pixels"""
    for gi, n in enumerate(ns):
        _check_red(op, dtname, n, got[..., gi], ref[..., gi], mag[..., gi], k_of_n(n))


# ------------------------------------------------------------------------------------------------
# pw_small_fwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stats,bias", [(1, 0, 1), (1, 1, 1), (2, 0, 1), (2, 0, 0)])
@pytest.mark.parametrize("cvn", [1, 8, 64])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pw_small_fwd(dtname, cvn, k, stats, bias):
    """C/V = 8 without statistics is the DPP branch, with them the generic one; C/V = 1 puts 64 pixels in a wave,
    C/V = 64 one"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cvn * V
    for M, N in PIXELS:
        G, HW = _tiles128(M), M // N
        g = _gen("pw_small_fwd", dtname, C, k, M)
        x = _rnd(g, (M, C), tdt)
        w = (torch.randn(k, C, generator=g) / math.sqrt(C)).to(F32)
        b = (torch.randn(k, generator=g) * 0.1).to(F32) if bias else None
        wd, bd = _dev(w), (_dev(b) if bias else None)

        def run(strided):
            xo = Op(x, strided, 0)
            y, st = Flat(M * k), Flat(2 * G)
            lib.pw_small_fwd(dt, xo.ptr, xo.ld, M, HW, C, k, wd.data_ptr(), bd.data_ptr() if bias else 0, y.ptr,
                             st.ptr if stats else 0, _st())
            torch.cuda.synchronize()
            xo.guard("pw_small_fwd x")
            y.guard("pw_small_fwd y")
            st.guard("pw_small_fwd stats")
            out = dict(y=y.get(N, k, HW))
            if stats:
                out["stats"] = st.get(G, 2)
            else:
                assert bool(torch.isnan(st.buf).all()), "stats written without a stats pointer"
            return out

        o = _twice(run, f"pw_small_fwd M={M}")
        ref, mag = R.pw_fwd(x, w, b, N)
        # k: C addends, their products rounded, the bias add
        _check("pw_small_fwd y", dtname, o["y"], ref, mag, F32, C + 2)
        if stats:
            # from the stored fp32 psi, accumulated in double (mean and deviations too), cast once: the cast's
            # ulp and the n (+ 3) double roundings
            part, pmag, ns = R.tile_stats(o["y"].reshape(-1), 128)
            _check("pw_small_fwd stats sum", dtname, o["stats"][:, 0], part[:, 0], pmag[:, 0], F32, 128 * R.K_DOUBLE)
            _check("pw_small_fwd stats M2", dtname, o["stats"][:, 1], part[:, 1], pmag[:, 1], F32, 131 * R.K_DOUBLE)


# ------------------------------------------------------------------------------------------------
# pw_small_bwd, pw_head_bwd (the same arguments)
# ------------------------------------------------------------------------------------------------
def _bwd_case(entry, dtname, C, k, mode, tile):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    fn = getattr(lib, entry)
    for M, N in PIXELS:
        _tiles128(M)
        HW = M // N
        ns = [b - a for a, b in R.tile_ranges(M, tile)]
        G = len(ns)
        g = _gen(entry, dtname, C, k, M)
        x = _rnd(g, (M, C), tdt)
        w = (torch.randn(k, C, generator=g) / math.sqrt(C)).to(F32)
        dy = torch.randn(N, k, HW, generator=g).to(F32)
        dx0 = _rnd(g, (M, C), tdt) if mode == "acc" else None
        wd, dyd = _dev(w), _dev(dy)

        def run(strided):
            xo = Op(x, strided, 0)
            dxo = Op(dx0, strided, 1, (M, C), tdt)
            pw, pb = Flat(k * C * G), Flat(k * G)
            fn(dt, dyd.data_ptr(), xo.ptr, xo.ld, M, HW, C, k, wd.data_ptr(), 0 if mode == "nodx" else dxo.ptr,
               0 if mode == "nodx" else dxo.ld, int(mode == "acc"), pw.ptr, pb.ptr, _st())
            torch.cuda.synchronize()
            xo.guard(f"{entry} x")
            dxo.guard(f"{entry} dx")
            pw.guard(f"{entry} part_w")
            pb.guard(f"{entry} part_b")
            if mode == "nodx":
                assert bool(torch.isnan(dxo.buf).all()), "dx == NULL, yet the buffer behind it was written"
            return dict(dx=dxo.get(), part_w=pw.get(k, C, G), part_b=pb.get(k, G))

        o = _twice(run, f"{entry} M={M}")
        ref = R.pw_bwd(dy, x, w, dx0, tile)
        assert ref["n"] == ns
        if mode != "nodx":
            # k: K addends, their products rounded (a fused multiply-add saves that one), the add onto dx0
            _check(f"{entry} dx {mode}", dtname, o["dx"], ref["dx"], ref["dx_mag"], tdt, k + 1 + (mode == "acc"))
        # per tile: n addends, their products rounded / n addends
        _per_tile(f"{entry} part_w", dtname, ns, o["part_w"], ref["part_w"], ref["part_w_mag"], lambda n: n + 1)
        _per_tile(f"{entry} part_b", dtname, ns, o["part_b"], ref["part_b"], ref["part_b_mag"], lambda n: n)


@pytest.mark.parametrize("mode", ["write", "acc", "nodx"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("cvn", [1, 8, 256])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pw_small_bwd(dtname, cvn, k, mode):
    """C/V = 1: 256 pixel rows per block; 8: 32; 256: one row, every thread a channel vector"""
    _bwd_case("pw_small_bwd", dtname, cvn * _dt(dtname)[2], k, mode, 128)


@pytest.mark.parametrize("mode", ["write", "acc", "nodx"])
@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("C", [8, 64, 256])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pw_head_bwd(dtname, C, k, mode):
    """C = 8 / 64 / 256: 32 / 4 / 1 pixel rows per block; one 2048-pixel tile, so n = M"""
    _bwd_case("pw_head_bwd", dtname, C, k, mode, 2048)


# ------------------------------------------------------------------------------------------------
# pw_small_bwd_relu
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("C", [8, 64, 2048])
def test_pw_small_bwd_relu(C, k):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt("bf16")
    for M, N in PIXELS:
        G, HW = _tiles128(M), M // N
        ns = [b - a for a, b in R.tile_ranges(M, 128)]
        g = _gen("pw_small_bwd_relu", C, k, M)
        x = torch.relu(torch.randn(M, C, generator=g)).to(tdt)
        # +0, -0 and the smallest normal bf16, in the first and in the last pixel
        for p in {0, M - 1}:
            x[p, 1], x[p, 2], x[p, 3] = 0.0, -0.0, 2.0 ** -126
        assert bool(torch.signbit(x[0, 2])) and float(x[0, 3]) > 0
        w = (torch.randn(k, C, generator=g) / math.sqrt(C)).to(F32)
        dy = torch.randn(N, k, HW, generator=g).to(F32)
        wd, dyd = _dev(w), _dev(dy)

        def run(strided):
            xo = Op(x, strided, 0)
            dxo = Op(None, strided, 1, (M, C), tdt)
            pw, pb, pd = Flat(k * C * G), Flat(k * G), Flat(G * 2 * C)
            lib.pw_small_bwd_relu(dt, dyd.data_ptr(), xo.ptr, xo.ld, M, HW, C, k, wd.data_ptr(), dxo.ptr, dxo.ld,
                                  pw.ptr, pb.ptr, pd.ptr, _st())
            torch.cuda.synchronize()
            xo.guard("pw_small_bwd_relu x")
            dxo.guard("pw_small_bwd_relu dx")
            for f, name in ((pw, "part_w"), (pb, "part_b"), (pd, "part_d")):
                f.guard("pw_small_bwd_relu " + name)
            return dict(dx=dxo.get(), part_w=pw.get(k, C, G), part_b=pb.get(k, G), part_d=pd.get(G, 2, C))

        o = _twice(run, f"pw_small_bwd_relu M={M}")
        ref = R.pw_bwd_relu(dy, x, w, 128, tdt)
        # k as pw_small_bwd's dx: K addends, rounded products; exactly 0 where x <= 0 (+0 and -0 included)
        _check("pw_small_bwd_relu dx", "bf16", o["dx"], ref["dx_pre"], ref["dx_mag"], tdt, k + 1)
        dead = x.to(F64) <= 0
        assert bool((o["dx"].to(F64)[dead] == 0).all()), "dx is not 0 where x <= 0"
        _per_tile("pw_small_bwd_relu part_w", "bf16", ns, o["part_w"], ref["part_w"], ref["part_w_mag"], lambda n: n + 1)
        _per_tile("pw_small_bwd_relu part_b", "bf16", ns, o["part_b"], ref["part_b"], ref["part_b_mag"], lambda n: n)
        # slot 0: the column sums of the dx this call stored (bf16 values, summed in fp32: n addends); slot 1: 0
        s, m = R.tile_colsum(o["dx"], 128)
        _per_tile("pw_small_bwd_relu part_d", "bf16", ns, o["part_d"][:, 0].t(), s.t(), m.t(), lambda n: n)
        assert bool((o["part_d"][:, 1] == 0).all()), "part_d slot 1 is not 0"


# ------------------------------------------------------------------------------------------------
# pw_head_fwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,bias", [(1, 1), (3, 1), (3, 0), (32, 1)])
@pytest.mark.parametrize("C", [8, 64, 256])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pw_head_fwd(dtname, C, k, bias):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    for M, N in PIXELS:
        HW = M // N
        g = _gen("pw_head_fwd", dtname, C, k, M)
        x = _rnd(g, (M, C), tdt)
        w = (torch.randn(k, C, generator=g) / math.sqrt(C)).to(F32)
        b = (torch.randn(k, generator=g) * 0.1).to(F32) if bias else None
        wd, bd = _dev(w), (_dev(b) if bias else None)

        def run(strided):
            xo = Op(x, strided, 0)
            y = Flat(M * k)
            lib.pw_head_fwd(dt, xo.ptr, xo.ld, M, HW, C, k, wd.data_ptr(), bd.data_ptr() if bias else 0, y.ptr, _st())
            torch.cuda.synchronize()
            xo.guard("pw_head_fwd x")
            y.guard("pw_head_fwd y")
            return dict(y=y.get(N, k, HW))

        o = _twice(run, f"pw_head_fwd M={M}")
        ref, mag = R.pw_fwd(x, w, b, N)
        # k: C addends, their products rounded, the bias add
        _check("pw_head_fwd y", dtname, o["y"], ref, mag, F32, C + 2)


# ------------------------------------------------------------------------------------------------
# attention gate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cvn", [1, 8, 64])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_attn_apply(dtname, cvn):
    """alpha against the float64 sigmoid in fp32 ulps: psi is a multiple of 2^-10 below 8 in magnitude, sc = 0.75
    and sh = 0.25, so z = psi sc + sh is exact in fp32 (15 significant bits, fused or not) and the error is that of
    expf, 1 + e and the division alone"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cvn * V
    sc, sh = torch.tensor([0.75]), torch.tensor([0.25])
    scd, shd = _dev(sc), _dev(sh)
    for M, N in PIXELS:
        g = _gen("attn_apply", dtname, C, M)
        skip = _rnd(g, (M, C), tdt)
        psi = (torch.round(torch.randn(M, generator=g) * 1.5 * 1024) / 1024).clamp(-7.5, 7.5).to(F32)
        psid = _dev(psi)

        def run(strided):
            so = Op(skip, strided, 0)
            go = Op(None, strided, 1, (M, C), tdt)
            al = Flat(M)
            lib.attn_apply(dt, so.ptr, so.ld, psid.data_ptr(), scd.data_ptr(), shd.data_ptr(), al.ptr, go.ptr, go.ld, M, C,
                           _st())
            torch.cuda.synchronize()
            so.guard("attn_apply skip")
            go.guard("attn_apply gated")
            al.guard("attn_apply alpha")
            return dict(alpha=al.get(M), gated=go.get())

        o = _twice(run, f"attn_apply M={M}")
        aref, z, zmag = R.attn_alpha(psi, sc, sh)
        assert torch.equal(z.to(F32).to(F64), z), "z is not exact in fp32"
        ulps = float(((o["alpha"].to(F64) - aref).abs() / R.ulp_store(aref, F32)).max())
        ALPHA[dtname] = max(ALPHA.get(dtname, 0.0), ulps)
        print(f"alpha {dtname} M={M}: {ulps:.4g} ulps")
        # no wider than the 2e-6 relative tests/test_gpu_c4c5.py holds alpha to
        assert ALPHA_ULPS * 2.0 ** -23 <= 2e-6
        assert ulps <= ALPHA_ULPS, f"alpha: {ulps} ulps from the float64 sigmoid (bound {ALPHA_ULPS})"
        # gated from the alpha this call stored: k = 1, the product
        ref, mag = R.attn_apply(skip, o["alpha"])
        _check("attn_apply gated", dtname, o["gated"], ref, mag, tdt, 1)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("cvn", [1, 8, 64, 128])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_attn_bwd1(dtname, cvn, acc):
    """C/V = 128: two channel chunks per lane (nchunk = 2), the one-pixel-group loop"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cvn * V
    for M, N in PIXELS:
        G1 = _tiles128(M)
        g = _gen("attn_bwd1", dtname, C, M)
        dg, skip = _rnd(g, (M, C), tdt), _rnd(g, (M, C), tdt)
        ds0 = _rnd(g, (M, C), tdt) if acc else None
        psi = torch.randn(M, generator=g).to(F32)
        alpha = torch.sigmoid(torch.randn(M, generator=g) * 1.5).to(F32)
        mean, inv = torch.tensor([0.1], dtype=F32), torch.tensor([1.3], dtype=F32)
        d = [_dev(t) for t in (alpha, psi, mean, inv)]

        def run(strided):
            go, so = Op(dg, strided, 0), Op(skip, strided, 1)
            do = Op(ds0, strided, 2, (M, C), tdt)
            db, part = Flat(M), Flat(2 * G1)
            lib.attn_bwd1(dt, go.ptr, go.ld, so.ptr, so.ld, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                          d[3].data_ptr(), do.ptr, do.ld, acc, db.ptr, M, C, part.ptr, _st())
            torch.cuda.synchronize()
            for o_, name in ((go, "dg"), (so, "skip"), (do, "dskip"), (db, "dpsibn"), (part, "part")):
                o_.guard("attn_bwd1 " + name)
            return dict(dskip=do.get(), dpsibn=db.get(M), part=part.get(2, G1))

        o = _twice(run, f"attn_bwd1 M={M}")
        ref = R.attn_bwd1(dg, skip, alpha, ds0)
        # k: the product with alpha, and the add onto the old value
        _check(f"attn_bwd1 dskip acc={acc}", dtname, o["dskip"], ref["dskip"], ref["dskip_mag"], tdt, 1 + acc)
        # k: C addends, their products rounded, * alpha, 1 - alpha, * (1 - alpha)
        _check("attn_bwd1 dpsibn", dtname, o["dpsibn"], ref["dpsibn"], ref["dpsibn_mag"], F32, C + 4)
        # from the stored dpsibn, accumulated in double, cast once: the cast's ulp and at most 128 double
        # roundings; the second sum forms psi - mean in fp32: one fp32 rounding in the summand
        part, pmag, ns = R.attn_bwd1_part(o["dpsibn"], psi, mean, inv)
        _check("attn_bwd1 part sum", dtname, o["part"][0], part[0], pmag[0], F32, 128 * R.K_DOUBLE)
        _check("attn_bwd1 part sum xhat", dtname, o["part"][1], part[1], pmag[1], F32, 1 + 130 * R.K_DOUBLE)


@pytest.mark.parametrize("cvn", [1, 8, 256])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_attn_bwd2(dtname, cvn):
    """C/V = 1: 256 pixel rows per block (the four-pixel main loop never runs at a 128-pixel tile); 8: 32 rows, one
    round of four; 256: one row, 32 rounds of four and the tail"""
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    C = cvn * V
    for M, N in PIXELS:
        G = _tiles128(M)
        g = _gen("attn_bwd2", dtname, C, M)
        f = torch.relu(torch.randn(M, C, generator=g)).to(tdt)
        for p in {0, M - 1}:
            f[p, 0], f[p, V - 1] = 0.0, -0.0
        w = (torch.randn(C, generator=g) / math.sqrt(C)).to(F32)
        dpsibn = (torch.randn(M, generator=g) * 0.1).to(F32)
        psi = torch.randn(M, generator=g).to(F32)
        mean, inv = torch.tensor([0.1], dtype=F32), torch.tensor([1.3], dtype=F32)
        coef = torch.tensor([1.7, 0.05, -0.3, 0, 0, 0], dtype=F32)
        d = [_dev(t) for t in (dpsibn, psi, mean, inv, coef, w)]

        def run(strided):
            fo = Op(f, strided, 0)
            zo = Op(None, strided, 1, (M, C), tdt)
            pw, pb = Flat(C * G), Flat(G)
            lib.attn_bwd2(dt, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), fo.ptr,
                          fo.ld, d[5].data_ptr(), zo.ptr, zo.ld, M, C, pw.ptr, pb.ptr, _st())
            torch.cuda.synchronize()
            for o_, name in ((fo, "f"), (zo, "dzf"), (pw, "part_w"), (pb, "part_b")):
                o_.guard("attn_bwd2 " + name)
            return dict(dzf=zo.get(), part_w=pw.get(C, G), part_b=pb.get(G))

        o = _twice(run, f"attn_bwd2 M={M}")
        ref = R.attn_bwd2(dpsibn, psi, mean, inv, coef, f, w, 128)
        # k: dpsi's five roundings (nhwc_ref.K_ATTN_DPSI), the product with wpsi; exactly 0 where f <= 0
        _check("attn_bwd2 dzf", dtname, o["dzf"], ref["dzf"], ref["dzf_mag"], tdt, R.K_ATTN_DPSI + 1)
        assert bool((o["dzf"].to(F64)[f.to(F64) <= 0] == 0).all()), "dzf is not 0 where f <= 0"
        # per tile: n addends (fused multiply-adds), each carrying dpsi's five roundings
        _per_tile("attn_bwd2 part_w", dtname, ref["n"], o["part_w"], ref["part_w"], ref["part_w_mag"],
                  lambda n: n + R.K_ATTN_DPSI)
        _per_tile("attn_bwd2 part_b", dtname, ref["n"], o["part_b"], ref["part_b"], ref["part_b_mag"],
                  lambda n: n + R.K_ATTN_DPSI)


# ------------------------------------------------------------------------------------------------
# global average pooling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8, 2048])
@pytest.mark.parametrize("HW", [1, 7, 300])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_gap(dtname, B, HW, C):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    g = _gen("gap", dtname, B, HW, C)
    x = _rnd(g, (B * HW, C), tdt)
    dg = torch.randn(B, C, generator=g).to(F32)
    dgd = _dev(dg)

    def fwd(strided):
        xo = Op(x, strided, 0)
        go = Flat(B * C)
        lib.gap_fwd(dt, xo.ptr, xo.ld, B, HW, C, go.ptr, _st())
        torch.cuda.synchronize()
        xo.guard("gap_fwd x")
        go.guard("gap_fwd g")
        return dict(g=go.get(B, C))

    o = _twice(fwd, "gap_fwd")
    ref, mag = R.gap_fwd(x.reshape(B, HW, C))
    # summed and divided in double, cast once: the cast's ulp and HW + 1 double roundings
    _check("gap_fwd", dtname, o["g"], ref, mag, F32, (HW + 1) * R.K_DOUBLE)
    for acc in (0, 1):
        dx0 = _rnd(g, (B * HW, C), tdt) if acc else None

        def bwd(strided):
            do = Op(dx0, strided, 1, (B * HW, C), tdt)
            lib.gap_bwd(dt, dgd.data_ptr(), B, HW, C, do.ptr, do.ld, acc, _st())
            torch.cuda.synchronize()
            do.guard("gap_bwd dx")
            return dict(dx=do.get())

        o = _twice(bwd, "gap_bwd")
        ref, mag = R.gap_bwd(dg, HW, dx0.reshape(B, HW, C) if acc else None)
        # k: the division, and the add onto the old value
        _check(f"gap_bwd acc={acc}", dtname, o["dx"].reshape(B, HW, C), ref, mag, tdt, 1 + acc)


# ------------------------------------------------------------------------------------------------
# input packing (dense operands: no strided run; exact)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["c", 8, 16])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("dtname", ["bf16", "fp32"])
def test_pack_input(dtname, c, pad):
    from unetseg_hip.lib import lib
    dt, tdt, V = _dt(dtname)
    cpad = c if pad == "c" else pad
    N, H, W = 2, 3, 5
    x = torch.randn(N, c, H, W, generator=_gen("pack_input", c, cpad))
    xd = _dev(x)
    y = Flat(N * H * W * cpad, tdt)
    lib.pack_input(dt, xd.data_ptr(), N, c, H, W, cpad, y.ptr, _st())
    torch.cuda.synchronize()
    y.guard("pack_input y")
    assert torch.equal(R._bits(y.get(N, H, W, cpad)), R._bits(R.pack_input(x, cpad, tdt)))


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", [1, 5, 37])
@pytest.mark.parametrize("c", [1, 3, 8])
def test_pack_input_stem(c, W, H):
    """the image column at +3, the 3 left and 5 right border columns and the channels >= c zero"""
    from unetseg_hip.lib import lib
    N = 2
    x = torch.randn(N, c, H, W, generator=_gen("pack_input_stem", c, W, H))
    xd = _dev(x)
    y = Flat(N * H * (W + 8) * 8, torch.bfloat16)
    lib.pack_input_stem(xd.data_ptr(), N, c, H, W, y.ptr, _st())
    torch.cuda.synchronize()
    y.guard("pack_input_stem xp")
    got = y.get(N, H, W + 8, 8)
    assert torch.equal(R._bits(got), R._bits(R.pack_input_stem(x)))
    assert bool((R._bits(got[:, :, :3]) == 0).all()) and bool((R._bits(got[:, :, 3 + W:]) == 0).all())
    assert bool((R._bits(got[..., c:]) == 0).all())
