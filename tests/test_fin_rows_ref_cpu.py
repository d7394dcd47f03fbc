"""CPU: the float64 references of the row-partial finalize family (tests/fin_rows_ref.py) pinned to PyTorch, and
the data maker's stated condition: on every case id of tests/test_gpu_fin_rows_contract.py the bounds that file
asserts are reachable by a correct implementation, shown before a GPU is involved.

The references are fed float64 partials of float64 pixel data here (no fp32 rounding anywhere), so they must
agree with torch.nn.BatchNorm2d / autograd in float64 to 1e-12.
"""
import pytest
import torch

import fin_rows_cases as K
import fin_rows_ref as FR
import nhwc_ref as R

F64 = torch.float64
TOL = 1e-12


def _close(a, b, what):
    a, b = R.f64(a), R.f64(b)
    err = float(((a - b).abs() / (1 + b.abs())).max())
    assert err <= TOL, f"{what}: {err:.3e}"


def _stat_parts(x, tile):
    """float64 (sum, M2 about the row's mean) rows of x [M][C]"""
    part, _, _ = R.channel_stats(x, tile)
    return part


def _sum_parts(cols, tile):
    """cols: list of [M][C] -> float64 [G][len][C] row sums"""
    return torch.stack([R.tile_colsum(v, tile)[0] for v in cols], 1)


# ------------------------------------------------------------------------------------------------
# bn_finalize_rows against nn.BatchNorm2d (train mode, float64)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,tile", [(2, 3, 256), (37, 5, 16), (256, 4, 256), (1031, 7, 128), (4099, 3, 16)])
@pytest.mark.parametrize("momentum", [0.1, 0.37, None])
def test_bn_finalize_rows_is_batchnorm2d(M, C, tile, momentum):
    g = K.gen("cpu-fin", M, C, tile)
    x = 3.0 + 0.5 * torch.randn(M, C, generator=g, dtype=F64)
    bn = torch.nn.BatchNorm2d(C, eps=1e-5, momentum=momentum).to(F64).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y = bn(x.view(M, C, 1, 1)).view(M, C)
    # num_batches_tracked: one per training forward; momentum None is the cumulative average 1 / nbt, 1 at the
    # first step
    assert int(bn.num_batches_tracked) == 1
    ref = FR.bn_finalize_rows(_stat_parts(x, tile), M, tile, bn.weight, bn.bias, rm0, rv0,
                              1.0 if momentum is None else momentum, 1e-5)
    _close(ref["mean"], x.mean(0), "mean")
    _close(ref["var"], x.var(0, unbiased=False), "var")
    _close(x * ref["scale"] + ref["shift"], y, "scale / shift")
    _close((x - ref["mean"]) * ref["invstd"] * bn.weight + bn.bias, y, "mean / invstd")
    _close(ref["rmean"], bn.running_mean, "running_mean")
    _close(ref["rvar"], bn.running_var, "running_var")
    # a second step moves the counter once more, and the buffers from where the first left them
    bn(x.view(M, C, 1, 1))
    assert int(bn.num_batches_tracked) == 2
    if momentum is not None:
        ref2 = FR.bn_finalize_rows(_stat_parts(x, tile), M, tile, bn.weight, bn.bias, ref["rmean"], ref["rvar"],
                                   momentum, 1e-5)
        _close(ref2["rmean"], bn.running_mean, "running_mean, step 2")
        _close(ref2["rvar"], bn.running_var, "running_var, step 2")


def test_bn_finalize_rows_single_pixel():
    """M == 1: the mean is the pixel, the variance 0, and the running variance takes the biased one (BatchNorm2d
    refuses one value per channel in train mode)"""
    C = 5
    g = K.gen("cpu-fin-1")
    x = torch.randn(1, C, generator=g, dtype=F64)
    p = K.bn_params("cpu-fin-1", C)
    ref = FR.bn_finalize_rows(_stat_parts(x, 256), 1, 256, p["gamma"], p["beta"], p["rmean"], p["rvar"], 0.1, 1e-5)
    _close(ref["mean"], x[0], "mean")
    _close(ref["invstd"], torch.full((C,), 1e-5, dtype=F64) ** -0.5, "invstd")
    _close(ref["rvar"], 0.9 * p["rvar"].to(F64), "running_var")
    _close(ref["shift"], p["beta"].to(F64) - x[0] * ref["scale"], "shift")


# ------------------------------------------------------------------------------------------------
# bn_bwd_finalize_rows* against autograd and nhwc_ref.bn_bwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbranch", [1, 2])
@pytest.mark.parametrize("M,C,tile", [(37, 5, 16), (1031, 7, 128)])
def test_bn_bwd_finalize_rows_is_autograd(M, C, tile, nbranch):
    g = K.gen("cpu-bwd", M, C, tile, nbranch)
    y = [torch.randn(M, C, generator=g, dtype=F64) * 2 + 0.7 for _ in range(2)]
    st = [R.batch_stats(v) for v in y]
    mean = [s[0] for s in st]
    inv = [1 / torch.sqrt(s[1] + 1e-5) for s in st]
    xh = [(y[b] - mean[b]) * inv[b] for b in range(2)]
    dz = torch.randn(M, C, generator=g, dtype=F64)
    gam = [(torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_() for _ in range(2)]
    bet = [torch.randn(C, generator=g, dtype=F64).requires_grad_() for _ in range(2)]
    out = sum(gam[b] * xh[b] + bet[b] for b in range(nbranch))
    (out * dz).sum().backward()
    old = [torch.randn(C, generator=g, dtype=F64) for _ in range(4)]
    part = _sum_parts([dz] + [dz * xh[b] for b in range(nbranch)], tile)
    # fp32 coefficient inputs (coef[0] is their fp32 product), float64 everything else
    g32, i32 = [v.detach().to(torch.float32) for v in gam], [v.to(torch.float32) for v in inv]
    if nbranch == 1:
        ref = FR.bn_bwd_finalize_rows(part, M, g32[0], i32[0], old[0], old[1])
        same = FR.bn_bwd_finalize_rows_res(part, M, 1, g32[0], i32[0], old[0], old[1])
        for k in ("dgamma1", "dbeta1", "coef"):
            assert torch.equal(ref[k], same[k]), k
        assert ref["coef"].shape == (3, C)
    else:
        ref = FR.bn_bwd_finalize_rows_res(part, M, 2, g32[0], i32[0], old[0], old[1], g32[1], i32[1], old[2], old[3])
        assert ref["coef"].shape == (6, C)
    for b in range(nbranch):
        _close(ref[f"dgamma{b + 1}"], old[2 * b] + gam[b].grad, f"dgamma{b + 1}")
        _close(ref[f"dbeta{b + 1}"], old[2 * b + 1] + bet[b].grad, f"dbeta{b + 1}")
    # the coefficients of nhwc_ref.bn_bwd (the table the apply pass is tested with)
    nh = R.bn_bwd(dz, None, y[0], mean[0], inv[0], y[1] if nbranch == 2 else None, mean[1], inv[1], g32[0], g32[1], M,
                  want_dy=False)
    for b in range(nbranch):
        exact = g32[b].to(F64) * i32[b].to(F64)
        assert float((ref["coef"][3 * b] - exact).abs().max()) <= float((R.EPS32 * exact.abs()).max())
        assert torch.equal(ref["coef"][3 * b].to(torch.float32), g32[b] * i32[b])
        _close(ref["coef"][3 * b + 1], nh["coef"][3 * b + 1], f"coef[{3 * b + 1}]")
        _close(ref["coef"][3 * b + 2], nh["coef"][3 * b + 2], f"coef[{3 * b + 2}]")
    if nbranch == 2:  # both branches share the sum of dz
        assert torch.equal(ref["coef"][1], ref["coef"][4])
        _close(ref["dbeta2"] - old[3], ref["dbeta1"] - old[1], "dbeta2's sum")


# ------------------------------------------------------------------------------------------------
# the merges against the statistics of the concatenated rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,tile,last", [(1, 16, 5), (15, 16, 16), (16, 8, 1), (17, 16, 7), (65, 8, 8), (100, 4, 3)])
def test_merges_are_the_statistics_of_the_concatenated_rows(G, tile, last):
    C = 6
    M = (G - 1) * tile + last
    g = K.gen("cpu-merge", G, tile, last)
    x = torch.randn(M, C, generator=g, dtype=F64) * 0.5 + torch.tensor([0, 1, 30, -30, 2, -1], dtype=F64)
    part = _stat_parts(x, tile)
    out, mag, cnt2 = FR.merge_rows_chan(part, G, M, tile)
    want = _stat_parts(x, tile * FR.MERGE_R)
    assert out.shape == want.shape == ((G + 15) // 16, 2, C)
    _close(out, want, "Chan merge")
    assert cnt2.tolist() == [float(min(tile * 16, M - i * tile * 16)) for i in range(out.shape[0])]
    assert bool((mag >= out.abs() * (1 - 1e-12)).all())
    # merged rows feed bn_finalize with tile * 16: the same statistics
    p = K.bn_params("cpu-merge", C)
    a = FR.bn_finalize_rows(part, M, tile, p["gamma"], p["beta"], p["rmean"], p["rvar"], 0.1, 1e-5)
    b = FR.bn_finalize_rows(out, M, tile * 16, p["gamma"], p["beta"], p["rmean"], p["rvar"], 0.1, 1e-5)
    for k in FR.FIN_OUTPUTS:
        _close(b[k], a[k], f"finalize of merged rows, {k}")
    for nq in (2, 3):
        cols = [torch.randn(M, C, generator=g, dtype=F64) for _ in range(nq)]
        rows = _sum_parts(cols, tile)
        o, m = FR.merge_rows(rows, G, nq)
        _close(o, _sum_parts(cols, tile * FR.MERGE_R), f"plain merge nq={nq}")
        _close(o.sum(0), torch.stack([v.sum(0) for v in cols]), f"plain merge total nq={nq}")
        assert bool((m >= o.abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------------------------------------
# the data maker's condition: every GPU case id, its bound, two correct implementations
# ------------------------------------------------------------------------------------------------
def _f32(x):
    return x.to(torch.float32)


def _fin_float32(d):
    """bn_finalize with float64 kept for the row reductions alone (the sum, Chan's M2), every multiply and divide
    after them and the store in float32"""
    ref = d["ref"]
    M, mom, eps = ref["M"], ref["momentum"], ref["eps"]
    gam, bet, rm0, rv0 = (_f32(d[k]) for k in ("gamma", "beta", "rmean", "rvar"))
    mean, var = _f32(ref["sum"] / M), _f32(ref["m2"] / M)
    unb = _f32(ref["m2"] / (M - 1)) if M > 1 else var
    inv = _f32(1.0 / torch.sqrt(var.to(F64) + eps))
    # 1 - momentum is a subtraction: kept as the kernel has it, each product with it rounded once
    keep = lambda v: _f32((1.0 - mom) * v.to(F64)).to(F64)  # noqa: E731
    return dict(mean=mean, invstd=inv, scale=gam * inv, shift=_f32(bet.to(F64) - ((mean * gam) * inv).to(F64)),
                rmean=_f32(keep(rm0) + _f32(mom * mean.to(F64)).to(F64)),
                rvar=_f32(keep(rv0) + _f32(mom * unb.to(F64)).to(F64)))


def _bwd_float32(d, ref):
    """the backward finalizes: the fp64 sums cast to fp32, then the add and the divide in float32"""
    M32 = torch.tensor(float(ref["M"]), dtype=torch.float32)
    got, coef = {}, torch.zeros_like(ref["coef"], dtype=torch.float32)
    for b in range(ref["nb"]):
        got[f"dgamma{b + 1}"] = d["dg0"][b] + _f32(ref["sums"][1 + b])
        got[f"dbeta{b + 1}"] = d["db0"][b] + _f32(ref["sums"][0])
        coef[3 * b] = d["g"][b] * d["inv"][b]
        coef[3 * b + 1] = _f32(ref["sums"][0] / ref["M"])
        coef[3 * b + 2] = _f32(ref["sums"][1 + b] / ref["M"])
    got["coef"] = coef
    return got


def _bwd_float64(ref):
    got = {k: _f32(v) for k, v in ref.items() if k.startswith(("dgamma", "dbeta")) and not k.endswith("_mag")}
    got["coef"] = _f32(ref["coef"])
    return got


@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_bounds_reachable_bn_finalize(G, C):
    d = K.fin_case(G, C)
    ref = d["ref"]
    FR.check_bn_finalize({k: _f32(ref[k]) for k in FR.FIN_OUTPUTS}, ref, G, f"float64 G={G} C={C}")
    FR.check_bn_finalize(_fin_float32(d), ref, G, f"float32 G={G} C={C}")
    # the 30s are there: the largest |mean| / std of the case (C >= 3 holds all three ratios)
    if C >= 3:
        assert float((ref["mean"].abs() * ref["invstd"]).max()) > 25


def test_bounds_reachable_bn_finalize_single_pixel():
    d = K.stats_rows("one", 1, 5, 256, 1)
    p = K.bn_params("one", 5)
    d.update(p)
    d["ref"] = ref = FR.bn_finalize_rows(d["part"], 1, 256, p["gamma"], p["beta"], p["rmean"], p["rvar"], K.MOMENTUM, K.EPS)
    FR.check_bn_finalize({k: _f32(ref[k]) for k in FR.FIN_OUTPUTS}, ref, 1, "float64 M=1")
    FR.check_bn_finalize(_fin_float32(d), ref, 1, "float32 M=1")


@pytest.mark.parametrize("form", ["rows", "res1", "res2"])
@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_bounds_reachable_bn_bwd(G, C, form):
    nb = {"rows": None, "res1": 1, "res2": 2}[form]
    d = K.bwd_rows(form, G, C, 2 if nb is None else 1 + nb)
    ref = K.bwd_ref(d, nb)
    FR.check_bn_bwd(_bwd_float64(ref), ref, G, f"float64 {form} G={G} C={C}")
    FR.check_bn_bwd(_bwd_float32(d, ref), ref, G, f"float32 {form} G={G} C={C}")


@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_bounds_reachable_colsum_rows(G, C):
    d = K.bwd_rows("colsum", G, C, 2)
    for k in (0, 1):
        for acc in (0, 1):
            s = d["part"][:, k].to(F64).sum(0)
            got = d["db0"][0] + _f32(s) if acc else _f32(s)
            FR.check_colsum(got, d["part"][:, k], acc, d["db0"][0], f"colsum G={G} C={C} k={k} acc={acc}")


@pytest.mark.parametrize("G,C,tile,last", K.MERGE_CASES)
def test_bounds_reachable_merge(G, C, tile, last):
    d = K.stats_rows("merge", G, C, tile, last)
    ref, mag, _ = FR.merge_rows_chan(d["part"], G, d["M"], tile)
    FR.check_merge(_f32(ref), ref, mag, True, f"Chan G={G} C={C}")
    for nq in (2, 3):
        part = K.bwd_rows("merge", G, C, nq)["part"]
        ref, mag = FR.merge_rows(part, G, nq)
        FR.check_merge(_f32(ref), ref, mag, False, f"plain nq={nq} G={G} C={C}")


@pytest.mark.parametrize("G,C", K.CHAIN_CASES)
def test_bounds_reachable_chain(G, C):
    """merge -> finalize judged against the reference of the unmerged rows: the merged rows evaluated in float64
    and rounded to fp32 once, then each finalize in float64 and with its epilogue in float32"""
    d = K.fin_case(G, C)
    mref, cnt2, more = K.chain_more_stats(d["part"], G, d["M"], d["tile"], d["ref"])
    m = FR.bn_finalize_rows(_f32(mref), d["M"], d["tile"] * 16, d["gamma"], d["beta"], d["rmean"], d["rvar"], K.MOMENTUM,
                            K.EPS)
    FR.check_bn_finalize({k: _f32(m[k]) for k in FR.FIN_OUTPUTS}, d["ref"], G, f"chain float64 G={G} C={C}", more)
    FR.check_bn_finalize(_fin_float32(dict(d, ref=m)), d["ref"], G, f"chain float32 G={G} C={C}", more)
    for form, nb in (("rows", None), ("res1", 1), ("res2", 2)):
        nq = 2 if nb is None else 1 + nb
        b = K.bwd_rows(form, G, C, nq)
        ref = K.bwd_ref(b, nb)
        merged = K.bwd_ref(dict(b, part=_f32(FR.merge_rows(b["part"], G, nq)[0])), nb)
        more_s = K.chain_more_sums(b["part"], G, nq)
        FR.check_bn_bwd(_bwd_float64(merged), ref, G, f"chain float64 {form} G={G} C={C}", more_s)
        FR.check_bn_bwd(_bwd_float32(b, merged), ref, G, f"chain float32 {form} G={G} C={C}", more_s)


def test_case_tables_cover_the_issue():
    """every G meets at least two C, every C at least three G; the Chan form meets both tiles with a last row of 1,
    37 and tile pixels; the largest input is 4097 x 3 x 260 floats at the most"""
    for cases, Gs, Cs in ((K.FIN_CASES, K.FIN_G, K.FIN_C), ([c[:2] for c in K.MERGE_CASES], K.MERGE_G, K.MERGE_C)):
        assert {g for g, _ in cases} == set(Gs) and {c for _, c in cases} == set(Cs)
        for G in Gs:
            assert len({c for g, c in cases if g == G}) >= 2, G
        for C in Cs:
            assert len({g for g, c in cases if c == C}) >= 3, C
        assert max(g * c for g, c in cases) * 3 <= 4097 * 3 * 260
    seen = {(tile, "tile" if last == tile else last) for _, _, tile, last in K.MERGE_CASES}
    assert seen == {(t, l) for t in (128, 256) for l in (1, 37, "tile")}
    assert set(K.CHAIN_CASES) == {(g, c) for g, c in K.FIN_CASES if g in (2049, 4097)} and len(K.CHAIN_CASES) == 4
