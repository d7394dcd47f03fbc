"""CPU: the references, data makers and case tables of tests/conv_generic_cases.py (the contract tests of the
generic conv kernels, tests/test_gpu_conv_generic.py).

  * the im2col references equal F.conv2d in float64 and its autograd for every case, all three directions
    (R != S, pad != R // 2 and stride 2 included), and their magnitudes are the same contraction over absolute
    values;
  * the exactness budget: with the integer ranges of the exact mode no partial sum of any case reaches 2^24,
    nor does a BN partial sum of 128 stored rows -- the condition that makes that mode independent of the
    summation order;
  * every one-hot maker yields exactly one non-zero per output channel, odd and with the top mantissa bit set;
  * with the library built: the host-only queries name the generic kernels for every case in both dtypes, for
    every parity class, with packed and with padded strides, and the listed split-K slab counts hold.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_generic_cases as cg

F64 = torch.float64
SHAPES = sorted(set(cg.all_shapes().values()))


def _id(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------------
# references against PyTorch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_references_equal_conv2d(shape):
    N, H, W, C1, C2, K, R, S, stride, pad = shape
    C = C1 + C2
    P, Q = cg.out_hw(H, W, R, S, stride, pad)
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, C, H, W, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(K, C, R, S, generator=g, dtype=F64, requires_grad=True)
    b, e = torch.randn(K, generator=g, dtype=F64), torch.randn(K, generator=g, dtype=F64)
    dy = torch.randn(N, K, P, Q, generator=g, dtype=F64)
    dx0 = torch.randn(N, C, H, W, generator=g, dtype=F64)
    y = F.conv2d(x, w, None, stride, pad)
    assert y.shape == (N, K, P, Q)
    y.backward(dy)

    def close(a, ref, what):
        assert a.shape == ref.shape, what
        assert float((a - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), what

    xd, wd = x.detach(), w.detach()
    v, m = cg.ref_fwd(xd, wd, stride, pad)
    close(v, y.detach(), "forward")
    close(m, F.conv2d(xd.abs(), wd.abs(), None, stride, pad), "forward magnitude")
    v, m = cg.ref_fwd(xd, wd, stride, pad, bias=b, escale=e, relu=True)
    close(v, torch.relu(y.detach() * e.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)), "forward, affine + ReLU")
    close(m, F.conv2d(xd.abs(), wd.abs(), None, stride, pad) * e.abs().view(1, -1, 1, 1) + b.abs().view(1, -1, 1, 1),
          "forward magnitude, affine")
    v, m = cg.ref_dgrad(dy, wd, H, W, stride, pad)
    close(v, x.grad, "data gradient")
    v1, m1 = cg.ref_dgrad(dy, wd, H, W, stride, pad, dx0)
    close(v1, x.grad + dx0, "data gradient, accumulated")
    close(m1, m + dx0.abs(), "data gradient magnitude, accumulated")
    v, m = cg.ref_wgrad(xd, dy, R, S, stride, pad)
    close(v, w.grad, "weight gradient")
    # the magnitudes of the gradients: the same autograd over absolute values
    xa, wa = xd.abs().requires_grad_(), wd.abs().requires_grad_()
    F.conv2d(xa, wa, None, stride, pad).backward(dy.abs())
    close(cg.ref_dgrad(dy, wd, H, W, stride, pad)[1], xa.grad, "data gradient magnitude")
    close(m, wa.grad, "weight gradient magnitude")


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_product_counts(shape):
    """products(): the contraction over ones counts the taps inside the image; its maximum is the L of the k rule"""
    N, H, W, C1, C2, K, R, S, stride, pad = shape
    C = C1 + C2
    P, Q = cg.out_hw(H, W, R, S, stride, pad)
    assert cg.max_products("fwd", shape) <= R * S * C
    assert cg.max_products("dgrad", shape) <= -(-R // stride) * -(-S // stride) * K
    assert cg.max_products("wgrad", shape) <= N * P * Q
    if pad == 0:
        assert float(cg.products("fwd", shape).min()) == R * S * C
        assert cg.max_products("wgrad", shape) == N * P * Q


def test_listed_geometry():
    """what the case table says each shape reaches"""
    mp = cg.max_products
    assert cg.out_hw(6, 7, 1, 3, 1, 1) == (8, 7)  # F_1x3: taller than the input
    # D_s2_odd: parity classes of 4 / 2 / 2 / 1 taps of 32 channels
    cnt = cg.products("dgrad", cg.case_shape("D_s2_odd", "fp32"))[0, 0]
    assert {float(cnt[h, w]) for h in (2, 3) for w in (2, 3)} == {32.0, 64.0, 128.0}
    # D_1x1s2: three of the four parity classes have no tap
    cnt = cg.products("dgrad", cg.case_shape("D_1x1s2", "fp32"))[0, 0]
    assert float(cnt[0, 0]) == 16 and float(cnt[0, 1]) == float(cnt[1, 0]) == float(cnt[1, 1]) == 0
    # D_uncovered: row 7 (and column 9) is reached by no output, the rest is
    cnt = cg.products("dgrad", cg.case_shape("D_uncovered", "fp32"))[0, 0]
    assert float(cnt[7].max()) == 0 and float(cnt[:, 9].max()) == 0 and float(cnt[:7, :9].min()) > 0
    assert mp("fwd", cg.case_shape("F_7x7", "fp32")) == 49 * 8
    # W_empty_slabs: 513 K steps in either dtype
    for dtname, bk in (("fp32", 16), ("bf16", 32)):
        N, H, W = cg.case_shape("W_empty_slabs", dtname)[:3]
        assert -(-N * H * W // bk) == 513
        assert cg.generic_splits(dtname, 8, 8, N * H * W) == 64 and -(-513 // 64) * 57 == 513


# ------------------------------------------------------------------------------------------------
# exactness budget
# ------------------------------------------------------------------------------------------------
def _budgets():
    for cid, (_, ep) in cg.FWD_CASES.items():
        for dtname in cg.STORE:
            yield cid, cg.exact_budget("fwd", cg.case_shape(cid, dtname), bias=ep.get("bias", False))
    for cid in cg.AFFINE_CASES:
        yield cid, cg.exact_budget("fwd", cg.case_shape(cid, "fp32"), affine=True)
    for cid in cg.DGRAD_CASES:
        yield cid, cg.exact_budget("dgrad", cg.case_shape(cid, "fp32"), accumulate=True)
    for cid in cg.WGRAD_CASES:
        for dtname in cg.STORE:
            yield cid, cg.exact_budget("wgrad", cg.case_shape(cid, dtname), accumulate=True)


def test_exactness_budget():
    for cid, b in _budgets():
        assert 0 < b["partial"] < 2 ** 24, (cid, b)
        assert b["stats"] < 2 ** 24, (cid, b)
    # the one-hot products: two 12-bit (8-bit) factors fit fp32's 24-bit significand
    assert (2 ** 12 - 1) ** 2 < 2 ** 24 and (2 ** 8 - 1) ** 2 + cg.ACC_MAX < 2 ** 24


def test_exact_mode_data_in_range():
    for cid in cg.DGRAD_CASES:
        for dtname, store in cg.STORE.items():
            d = cg.make_data(cid, "dgrad", cg.case_shape(cid, dtname), dtname, "exact", bias=True, affine=True)
            for name, m in (("x", 3), ("w", 3), ("dy", 3), ("bias", 3), ("escale", 3), ("dx0", 8)):
                t = d[name]
                assert float(t.abs().max()) <= m and torch.equal(t, t.round()), (cid, name)
                assert torch.equal(t.to(store).to(F64), t), (cid, name)


# ------------------------------------------------------------------------------------------------
# one-hot makers
# ------------------------------------------------------------------------------------------------
def _full_odd(v, bits):
    a = v.abs()
    return bool(((a % 2 == 1) & (a >= 2 ** (bits - 1)) & (a < 2 ** bits)).all())


@pytest.mark.parametrize("dtname", list(cg.STORE))
def test_onehot_makers(dtname):
    bits = 12 if dtname == "fp32" else 8
    store = cg.STORE[dtname]
    for cid in cg.FWD_CASES:
        shape = cg.case_shape(cid, dtname)
        d = cg.make_data(cid, "fwd", shape, dtname, "onehot")
        K = shape[5]
        nz = (d["w"] != 0).reshape(K, -1).sum(1)
        assert torch.equal(nz, torch.ones(K, dtype=nz.dtype)), cid
        assert _full_odd(d["w"][d["w"] != 0], bits) and _full_odd(d["x"], bits), cid
        assert d["bias"] is None
        assert torch.equal(d["x"].to(store).to(F64), d["x"]) and torch.equal(d["w"].to(store).to(F64), d["w"])
        # the first and the last K position are addressed (the K-loop tail)
        flat = d["w"].permute(0, 2, 3, 1).reshape(K, -1)
        assert flat[0, 0] != 0 and flat[-1, -1] != 0, cid
    for cid in cg.DGRAD_CASES:
        shape = cg.case_shape(cid, dtname)
        d = cg.make_data(cid, "dgrad", shape, dtname, "onehot")
        C = shape[3] + shape[4]
        nz = (d["w"] != 0).permute(1, 0, 2, 3).reshape(C, -1).sum(1)
        assert torch.equal(nz, torch.ones(C, dtype=nz.dtype)), cid
        assert _full_odd(d["w"][d["w"] != 0], bits) and _full_odd(d["dy"], bits), cid
    for cid in cg.WGRAD_CASES:
        shape = cg.case_shape(cid, dtname)
        d = cg.make_data(cid, "wgrad", shape, dtname, "onehot")
        K = shape[5]
        nz = (d["dy"] != 0).permute(1, 0, 2, 3).reshape(K, -1).sum(1)
        assert torch.equal(nz, torch.ones(K, dtype=nz.dtype)), cid
        assert _full_odd(d["dy"][d["dy"] != 0], bits) and _full_odd(d["x"], bits), cid
        # every weight-gradient element is then at most one product
        assert float(cg.ref_wgrad((d["x"] != 0).to(F64), (d["dy"] != 0).to(F64), *shape[6:])[0].max()) == 1


def test_layouts():
    tails = set()
    for (cid, dtname), shape in cg.all_shapes().items():
        direction = "dgrad" if cid in cg.DGRAD_CASES else "fwd"
        chs = cg.operand_channels(direction, shape)
        tail = cid in cg.TAIL_CASES
        lay = cg.layout(chs, tail)
        assert len({ld for ld, _ in lay}) == len(lay) and len({c0 for _, c0 in lay}) == len(lay), (cid, lay)
        for C, (ld, c0) in zip(chs, lay):
            assert c0 > 0 and c0 % 8 == 0 and ld % 8 == 0 and c0 + C <= ld, (cid, lay)
            assert (c0 + C == ld) == tail, (cid, lay)
        if tail:
            tails.add(cid[0])
    assert tails == {"F", "D", "W"} and cg.TAIL_CASES & set(cg.AFFINE_CASES)


# ------------------------------------------------------------------------------------------------
# dispatch (host-only queries of the built library)
# ------------------------------------------------------------------------------------------------
@pytest.fixture()
def lib():
    from unetseg_hip import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    from unetseg_hip import lib as L
    return L


def _layouts(direction, shape, cid):
    chs = cg.operand_channels(direction, shape)
    return [cg.packed_layout(chs), cg.layout(chs, cid in cg.TAIL_CASES), cg.layout(chs, True)]


@pytest.mark.parametrize("dtname", list(cg.STORE))
def test_forward_cases_select_generic(lib, dtname):
    dt = lib.DT_BF16 if dtname == "bf16" else lib.DT_F32
    for cid in cg.FWD_CASES:
        N, H, W, C1, C2, K, R, S, stride, pad = shape = cg.case_shape(cid, dtname)
        lays = _layouts("fwd", shape, cid)
        if cid == "F_dense_inplace":
            lays.append([(160, 0), (160, 96)])
        for lay in lays:
            got = lib.fwd_config(dt, C1, lay[0][0], C2, lay[1][0] if C2 else 0, N, H, W, K, R, S, stride, pad)
            assert got == "generic", (cid, dtname, lay, got)
            tile = lib.lib.conv2d_fwd_tile_m(dt, C1, lay[0][0], C2, lay[1][0] if C2 else 0, N, H, W, K, R, S, stride, pad)
            assert tile == cg.TILE_M, (cid, dtname, tile)


@pytest.mark.parametrize("dtname", list(cg.STORE))
def test_dgrad_cases_select_generic(lib, dtname):
    dt = lib.DT_BF16 if dtname == "bf16" else lib.DT_F32
    for cid in cg.DGRAD_CASES:
        N, H, W, C1, C2, K, R, S, stride, pad = shape = cg.case_shape(cid, dtname)
        P, Q = cg.out_hw(H, W, R, S, stride, pad)
        for lay in _layouts("dgrad", shape, cid):
            got = lib.dgrad_config(dt, lay[0][0], N, P, Q, K, C1, R, S, stride, pad, lay[1][0], H, W)
            assert got == ["generic"] * stride * stride, (cid, dtname, lay, got)


@pytest.mark.parametrize("dtname", list(cg.STORE))
def test_wgrad_cases_select_generic(lib, dtname, monkeypatch):
    dt = lib.DT_BF16 if dtname == "bf16" else lib.DT_F32
    for cid, (_, opt) in cg.WGRAD_CASES.items():
        N, H, W, C1, C2, K, R, S, stride, pad = shape = cg.case_shape(cid, dtname)
        P, Q = cg.out_hw(H, W, R, S, stride, pad)
        with monkeypatch.context() as mp:
            for name, val in opt.get("env", {}).get(dtname, {}).items():
                mp.setenv(name, val)
            for lay in _layouts("wgrad", shape, cid):
                kern, splits, _ = lib.wgrad_config(dt, C1, lay[0][0], C2, lay[1][0] if C2 else 0, N, H, W, lay[-1][0], K, R,
                                                   S, stride, pad)
                assert kern == "wgrad_generic", (cid, dtname, lay, kern)
                assert splits == cg.generic_splits(dtname, K, R * S * (C1 + C2), N * P * Q), (cid, dtname, splits)
                if "splits" in opt:
                    assert splits == opt["splits"][dtname], (cid, dtname, splits)
                ws = lib.lib.conv2d_wgrad_workspace(dt, N, P, Q, K, C1 + C2, R, S)
                assert ws >= splits * K * R * S * (C1 + C2) * 4, (cid, dtname, ws)
