"""CPU: the data makers, expected results, exactness budget and configuration coverage of the bit-exact tests of
the fast conv kernels (tests/conv_fast_exact_cases.py, run on the GPU by tests/test_gpu_conv_fast_exact.py).

  * budget: for every case, from its actual data in float64, the sum of the absolute values of the terms of every
    asserted quantity stays below 2^24 (in units of the quantity's quantum), so fp32 accumulation in any order
    -- any tile, slab or persistent-block schedule -- is exact.  Prints the largest figure per direction;
  * data makers: integer ranges, one non-zero per one-hot row, positions 0 and last used, the C1 boundary weights;
  * expected results against F.conv2d and its autograd at 1e-12, on both contraction paths of the helper;
  * coverage: from the host-only queries, the cases reach every configuration key strided_keys() reaches, minus
    the stem keys (needs the built library, as tests/test_conv_strided_cover_cpu.py).
"""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_fast_exact_cases as fx
import conv_generic_cases as cg

F64 = torch.float64
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, (v, cid) in sorted(WORST.items()):
        print(f"\nlargest budget figure  {k:<8s} {v:>10.0f} = 2^{torch.log2(torch.tensor(v)).item():.2f}  ({cid})", end="")
    print()


def _note(kind, v, cid):
    if v > WORST.get(kind, (0, ""))[0]:
        WORST[kind] = (v, cid)


def _all_cases():
    tcs = fx.strided()
    cases = [(cid, c[0], c[1]) for cid, c in tcs.STRIDED_CASES.items()]
    cases += [(f"first3x3_{d}", d, s) for d, s in tcs.FIRST3X3_CASES]
    return cases


_SEEN = {}


@pytest.mark.parametrize("cid,direction,shape", _all_cases(), ids=[c[0] for c in _all_cases()])
def test_exact_budget(cid, direction, shape):
    key = (direction, shape, repr(fx.NARROW.get(cid)))
    if key not in _SEEN:  # cases that differ only in their environment share data and figures
        d = fx.make_data(direction, shape, "exact", fx.NARROW.get(cid))
        worst = {}
        rules = (False, True) if direction == "dgrad" else (True,)
        for two in rules:
            for k, v in fx.budget(direction, shape, d, fx.expect(direction, shape, d, two)).items():
                worst[k] = max(worst.get(k, 0.0), v)
        _SEEN[key] = worst
    for k, v in _SEEN[key].items():
        assert v < fx.LIMIT, f"{cid}: {k} sums |terms| to {v:.0f} >= 2^24: narrow the case in NARROW"
        _note({"y": "fwd", "stats": "fwd", "dw": "wgrad"}.get(k, "dgrad") + ("" if k in ("y", "dw", "dx") else " sums"), v, cid)


def test_exact_budget_padk_head():
    for K, C1, H, W in fx.PADK_CASES:
        d = fx.padk_data(K, C1, H, W)
        dw = 2.0 * float((d["dy"].abs().t() @ d["x"].abs()).max())
        dx = float((d["dy"][:, :K].abs() @ d["w"].abs() + d["x"].abs()).max())
        assert dw < fx.LIMIT and dx < fx.LIMIT, (K, C1, H, W, dw, dx)
        _note("wgrad", dw, f"padk K{K} C{C1}")
    shape = fx.HEAD_SHAPE
    d = fx.make_data("fwd_relu", shape, "exact")
    y = fx.expect("fwd_relu", shape, d)["y"].to(F64)
    assert fx.budget("fwd_relu", shape, d, None)["y"] < fx.LIMIT
    for head_k, _ in fx.HEAD_CASES:
        hd = fx.head_data(head_k)
        fig = float((y.abs() @ hd["hw"].abs().t() + hd["hb"].abs()).max())
        assert fig < fx.LIMIT, (head_k, fig)
        _note("head", fig, f"head_k {head_k}")


def test_onehot_budget_is_one_product():
    """a 8-bit odd times a 8-bit odd: below 2^16, twice it (the accumulated weight gradient) below 2^17"""
    v = cg._odd(fx._g("t", (1,)), (4096,), 8)
    assert float(v.abs().max()) <= 255 and float(v.abs().min()) >= 129 and bool((v % 2 != 0).all())


# ------------------------------------------------------------------------------------------------
# data makers
# ------------------------------------------------------------------------------------------------
SMALL = {"fwd_all": (1, 5, 6, 8, 8, 16, 3, 1), "fwd_bnrelu_in": (1, 5, 6, 16, 0, 16, 1, 1), "dgrad": (1, 6, 7, 16, 0, 8, 3, 2),
         "post1": (1, 5, 6, 16, 0, 8, 3, 1), "post2": (1, 5, 6, 16, 0, 8, 3, 1), "post4": (1, 5, 6, 16, 0, 8, 3, 1),
         "post3": (1, 5, 6, 16, 0, 8, 1, 1), "post3_y2": (1, 5, 6, 16, 0, 8, 1, 1), "wgrad": (2, 6, 7, 8, 8, 16, 3, 2),
         "wgrad_bnrelu_in": (1, 5, 6, 16, 0, 8, 1, 1), "fwd_stats": (1, 5, 6, 8, 0, 16, 3, 1), "fwd_relu": (1, 5, 6, 8, 0, 16, 3, 1)}


def test_exact_ranges():
    shape = (1, 9, 8, 64, 64, 128, 3, 1)
    for direction in ("fwd_all", "post3_y2", "wgrad"):
        d = fx.make_data(direction, shape, "exact")
        for name in ("x", "w", "dy", "bias", "sc", "sh", "z", "y2"):
            if name in d:
                t = d[name]
                assert bool((t == t.round()).all()) and float(t.abs().max()) == 3 and float(t.min()) == -3, name
        if "g0" in d:
            assert bool((d["g0"] == d["g0"].round()).all()) and float(d["g0"].max()) == 8 and float(d["g0"].min()) == -8
            assert set(d["mu"].tolist()) <= {-1.0, 0.0, 1.0} and set(d["inv"].tolist()) <= {0.5, 1.0, 2.0}
            assert set(d["mu2"].tolist()) <= {-1.0, 0.0, 1.0} and set(d["inv2"].tolist()) <= {0.5, 1.0, 2.0}
            assert d["mbits"].dtype == torch.uint8 and len(set(d["mbits"].tolist())) > 100
    d1 = fx.make_data("fwd_all", shape, "exact", dict(w=1))
    assert float(d1["w"].abs().max()) == 1 and float(d1["x"].abs().max()) == 3
    # the zero of the BN-ReLU mask argument and of the ReLU output occurs often
    d = fx.make_data("post2", shape, "exact")
    arg = d["z"] * d["sc"][:128] + d["sh"][:128]
    assert float((arg == 0).double().mean()) > 0.05 and float((torch.relu(d["z"]) == 0).double().mean()) > 0.5


def test_onehot_rows():
    for direction, shape in (("fwd_all", (1, 9, 8, 64, 64, 128, 5, 1)), ("fwd_stats", (1, 9, 8, 2048, 0, 128, 1, 1)),
                             ("dgrad", (1, 24, 24, 64, 64, 64, 3, 2)), ("wgrad", (2, 15, 17, 64, 64, 128, 3, 1)),
                             ("fwd_bnrelu_in", (1, 9, 8, 320, 0, 128, 1, 1))):
        N, H, W, C1, C2, K, R_, s = shape
        cin = C1 + C2
        d = fx.make_data(direction, shape, "onehot")
        q = fx.query_class(direction)
        assert float(d["bias"].abs().max()) == 0 and bool((d["sc"] == 1).all()) and bool((d["sh"] == 0).all())
        for name in ("x", "dy", "w"):
            nz = d[name][d[name] != 0].abs()
            if nz.numel():
                assert float(nz.min()) >= 129 and float(nz.max()) <= 255 and bool((nz % 2 == 1).all()), name
        if q == "wgrad":
            assert bool(((d["dy"] != 0).sum((0, 2, 3)) == 1).all())
            flat = (d["dy"].permute(1, 0, 2, 3).reshape(K, -1) != 0).double().argmax(1)
            assert int(flat[0]) == 0 and int(flat[-1]) == d["dy"].numel() // K - 1
            continue
        w = d["w"].permute(0, 2, 3, 1) if q != "dgrad" else d["w"].permute(1, 2, 3, 0)  # [out][R][S][in]
        w = w.reshape(w.shape[0], -1)
        assert bool(((w != 0).sum(1) == 1).all()), direction
        pos = (w != 0).double().argmax(1)
        assert int(pos[0]) == 0 and int(pos[-1]) == w.shape[1] - 1, (direction, pos[0], pos[-1])
        if q == "fwd" and C2:  # the source boundary
            assert int((d["w"][1, C1 - 1] != 0).sum()) == 1 and int((d["w"][2, C1] != 0).sum()) == 1


# ------------------------------------------------------------------------------------------------
# expected results against PyTorch
# ------------------------------------------------------------------------------------------------
def test_contraction_paths_agree():
    for s, R_ in ((1, 3), (2, 3), (1, 1), (1, 5)):
        g = fx._g("paths", (s, R_))
        x, w = torch.randn(2, 8, 9, 11, generator=g, dtype=F64), torch.randn(6, 8, R_, R_, generator=g, dtype=F64)
        pad = R_ // 2
        y = F.conv2d(x, w, None, s, pad)
        dy = torch.randn(y.shape, generator=g, dtype=F64)
        assert float((fx.conv(x, w, s, pad) - cg._fwd(x, w, s, pad)).abs().max()) < 1e-12
        assert float((fx.conv_t(dy, w, 9, 11, s, pad) - cg._dgrad(dy, w, 9, 11, s, pad)).abs().max()) < 1e-12


@pytest.mark.parametrize("direction", list(SMALL))
def test_expect_against_autograd(direction):
    shape = SMALL[direction]
    N, H, W, C1, C2, K, R_, s = shape
    cin, pad, M = C1 + C2, R_ // 2, N * H * W
    d = fx.make_data(direction, shape, "exact")
    q = fx.query_class(direction)
    ex = fx.expect(direction, shape, d, two_round=True)
    x = d["x"].clone().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    xin = x
    if "bnrelu_in" in direction:
        xin = torch.relu(x * d["sc"][:C1].view(1, -1, 1, 1) + d["sh"][:C1].view(1, -1, 1, 1))
    y = F.conv2d(xin, w, None, s, pad)
    if direction in ("fwd_relu", "fwd_all"):
        y = torch.relu(y + d["bias"].view(1, -1, 1, 1))
    if q in ("fwd", "bnin"):
        assert float((ex["y"].to(F64) - fx.rows(y.detach())).abs().max()) < 1e-12  # |y| < 256: the rounding is exact
        return
    if q == "wgrad":
        xin.retain_grad()
        y.backward(d["dy"])
        assert float((ex["dw0"].to(F64) - w.grad).abs().max()) < 1e-12
        assert float((ex["dw1"].to(F64) - 2 * w.grad).abs().max()) < 1e-12
        return
    y.backward(d["dy"])
    dgrad = fx.rows(x.grad)  # small shapes: |dgrad| < 256, so both roundings are exact
    assert float(dgrad.abs().max()) < 256
    g0, z = d["g0"].reshape(M, cin), d["z"].reshape(M, cin)
    if direction == "dgrad":
        assert float((ex["dx0"].to(F64) - dgrad).abs().max()) < 1e-12
        assert float((ex["dx1"].to(F64) - (dgrad + g0)).abs().max()) < 1e-12
        return
    # the post-ops: autograd through the producer's activation
    zz = z.clone().requires_grad_(True)
    if direction == "post1":
        a, up = torch.relu(zz), dgrad
    elif direction == "post2":
        a, up = torch.relu(zz * d["sc"][:cin] + d["sh"][:cin]), dgrad
    else:
        bits = fx.unpack_bits(d["mbits"], M, cin)
        a, up = torch.where(bits, zz, torch.zeros((), dtype=F64)), (dgrad if direction == "post4" else dgrad + g0)
    a.backward(up)
    want = zz.grad
    if direction == "post2":  # d relu(z sc + sh) / dz carries sc; the kernel's d is the gradient at the BN output
        want = torch.where((z * d["sc"][:cin] + d["sh"][:cin]) > 0, dgrad, torch.zeros((), dtype=F64))
        assert float((zz.grad - want * d["sc"][:cin]).abs().max()) < 1e-12
    assert float((ex["dx"].to(F64) - want).abs().max()) < 1e-12
    assert float((ex["part"][0] - want.sum(0)).abs().max()) < 1e-12
    if direction != "post1" and direction != "post4":
        assert float((ex["part"][1] - (want * (z - d["mu"][:cin]) * d["inv"][:cin]).sum(0)).abs().max()) < 1e-12
    if direction == "post3_y2":
        xh2 = (d["y2"].reshape(M, cin) - d["mu2"][:cin]) * d["inv2"][:cin]
        assert float((ex["part"][2] - (want * xh2).sum(0)).abs().max()) < 1e-12


def test_accumulate_rules_differ_where_the_gradient_rounds():
    """|dgrad| > 256 with an odd low part: bf16_rn(dgrad + old) != bf16_rn(bf16_rn(dgrad) + old) somewhere, so a
    kernel that takes the other family's order fails; and the rule per configuration name"""
    shape = (1, 16, 32, 64, 0, 64, 3, 1)
    d = fx.make_data("dgrad", shape, "exact")
    one, two = fx.expect("dgrad", shape, d, False), fx.expect("dgrad", shape, d, True)
    assert torch.equal(one["dx0"], two["dx0"])
    n = int((one["dx1"] != two["dx1"]).sum())
    assert n > 0, "no element tells the two orders apart"
    assert not fx.acc_two_roundings("dgrad:halo3")
    for name in ("tn128x64_1st", "ring256x128_hp", "multi64x128", "ring64x128_t9", "tn128x128_1step"):
        assert fx.acc_two_roundings("dgrad:" + name)
    assert torch.equal(fx.bf16_rn(torch.tensor([257.0, 258.0, 259.0, -0.0], dtype=F64)).to(F64),
                       torch.tensor([256.0, 258.0, 260.0, 0.0], dtype=F64))


def test_stats_rows():
    """consecutive rows for the TN tiles and gather rings; tile / 32 x 32 spatial blocks, row-major over (image,
    block row, block column), for halo3, first3x3 and the halo-A rings: a permutation either way"""
    assert torch.equal(fx.stats_rows("fwd:ring256x128_t9", 1, 130, 130, 256), torch.arange(16900))
    for key, tile in (("fwd:halo3", 256), ("fwd:first3x3", 256), ("fwd:ring128x128_halo", 128), ("fwd:ring256x64_hp", 256)):
        N, P, Q = 2, 16, 64
        r = fx.stats_rows(key, N, P, Q, tile)
        assert torch.equal(r.sort().values, torch.arange(N * P * Q))
        tr = tile // 32
        for g in (0, 1, 2, N * P * Q // tile - 1):
            nb_th, tw = divmod(g, Q // 32)
            want = torch.tensor([(nb_th * tr + i) * Q + tw * 32 + j for i in range(tr) for j in range(32)])
            assert torch.equal(r[g * tile:(g + 1) * tile], want), (key, g)


# ------------------------------------------------------------------------------------------------
# configuration coverage (host-only queries)
# ------------------------------------------------------------------------------------------------
def test_cases_cover_every_fast_configuration():
    from unetseg_hip import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    from unetseg_hip import introspect
    from unetseg_hip.lib import DT_BF16, fwd_config, stem_config
    tcs = fx.strided()
    got = set()
    for cid, (direction, shape, expect, env, _) in tcs.STRIDED_CASES.items():
        with tcs._environ(env):
            keys = tcs.case_keys(direction, shape, tcs.packed_layout(tcs.operand_channels(direction, shape)))
        assert keys == expect, (cid, keys)
        got.update(keys)
    for _, (N, H, W, C1, C2, K, R_, s) in tcs.FIRST3X3_CASES:
        got.add("fwd:" + fwd_config(DT_BF16, C1, 8, 0, 0, N, H, W, K, R_, R_, s, 1))
    stem = set()
    for N, H, tn, _ in tcs.STEM_CASES:
        with tcs._environ({"UNETSEG_STEM_TN": "1"} if tn else {}):
            stem.add("stem_fwd:" + stem_config(N, H, H, 64)[0])
            stem.add(introspect.call_configs(("stem_wgrad", N, H, H, 3, 0, 64, 7, 7, 2, 3, 8, 0))[0])
    want = tcs.strided_keys() - stem
    assert got == want, sorted(got ^ want)
    # every accumulated data gradient names a family the rule knows
    for k in got:
        if k.startswith("dgrad"):
            fx.acc_two_roundings(k)
