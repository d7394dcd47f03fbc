"""GPU: float64 contract of the BatchNorm row-partial finalize kernels (csrc/elem.hip, csrc/fin_reduce.h) --
unetseg_bn_finalize, unetseg_bn_bwd_finalize_rows, unetseg_bn_bwd_finalize_rows_res, unetseg_fin_merge_rows,
unetseg_colsum_rows -- against the references of tests/fin_rows_ref.py, through the C ABI.

The reference reads the fp32 partial rows the kernel reads, so it is the exact function of those rows, and every
kernel accumulates in fp64 and rounds once: each output is held, element by element, to

    |got - ref| <= ulp_fp32(ref) + 1.01 k 2^-24 mag + G 2^-53 sum|part|

with k the fp32 roundings after the fp64 sums, counted beside each assertion in fin_rows_ref.check_* (k = 1 for
everything stored once, 2 for dgamma / dbeta added onto their old values, bit equality for the fp32 products
coef[0] / coef[3]).  Every output is exact-size inside a buffer with a sentinel tail that must survive bit for
bit; with nbranch == 1 the coefficient table is allocated with six rows and rows 3..5 keep the sentinel.  Every
kernel runs twice into different buffers and must repeat itself bit for bit (fixed-order sums).  The row and
channel counts sit on the switches of the launch geometry (tests/fin_rows_cases.py); the data makes a merge that
is not Chan's, or not in fp64, fail (|mean| / std up to 30), and the same bounds are shown reachable on every
case in tests/test_fin_rows_ref_cpu.py.  The largest |got - ref| / bound per (kernel, output, wave form) is
printed at the end; DESIGN.md (section 4a.1) holds the table measured on an MI355X.
"""
import types

import pytest
import torch

import fin_rows_cases as K
import fin_rows_ref as FR
import nhwc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
PAD = 64
NAN = float("nan")
WORST = {}  # (kernel, output, wave form) -> largest |got - ref| / bound seen in this module


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()
    yield
    for (kern, out, form), r in sorted(WORST.items()):
        print(f"\nworst ratio  {kern:<28s} {out:<8s} {form:<5s} {r:.4g}", end="")
    print()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _form(G):
    """the wave form the launch picks (fin_reduce.h fin_waves)"""
    return "one" if G <= 512 else "four"


def _note(kern, form, ratios):
    for out, r in ratios.items():
        WORST[(kern, out, form)] = max(WORST.get((kern, out, form), 0.0), r)
    print(f"ratio {kern} {form}: " + " ".join(f"{o}={r:.3g}" for o, r in ratios.items()))


def _out(n, init=None):
    """an exact-size output of n floats inside a buffer with a sentinel tail: NaN where the kernel writes, `init`
    (the old values) where it accumulates"""
    buf = torch.full((n + PAD,), R.SENTINEL, device=DEV)
    buf[:n] = NAN if init is None else init.to(DEV)
    return buf


def _bits(bufs):
    return [b.view(torch.int32).cpu() if b.dtype == torch.float32 else b.cpu() for b in bufs]


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(_bits(a), _bits(b))):
        assert torch.equal(x, y), f"{what}: output buffer {i} differs between two runs on the same input"


# ------------------------------------------------------------------------------------------------
# unetseg_bn_finalize
# ------------------------------------------------------------------------------------------------
def _finalize(part, C, G, M, tile, d, running=True, nbt0=K.NBT0):
    """one launch -> (got: name -> fp32 [C] on the CPU, every buffer); the tails and the counter asserted here"""
    from unetseg_hip.lib import lib
    gam, bet = d["gamma"].to(DEV), d["beta"].to(DEV)
    o = [_out(C) for _ in range(4)]
    rm, rv = _out(C, d["rmean"]), _out(C, d["rvar"])
    nbt = torch.full((1 + PAD,), 777, dtype=torch.int64, device=DEV)
    nbt[0] = nbt0
    run = (rm.data_ptr(), rv.data_ptr(), nbt.data_ptr()) if running else (0, 0, 0)
    lib.bn_finalize(part.data_ptr(), C, G, M, tile, gam.data_ptr(), bet.data_ptr(), *run, K.MOMENTUM, K.EPS,
                    *(t.data_ptr() for t in o), _st())
    torch.cuda.synchronize()
    for t, n in zip(o + [rm, rv], FR.FIN_OUTPUTS):
        R.assert_tail(t, C, R.SENTINEL, f"bn_finalize {n}")
    # incremented once: not once per channel, block or wave
    assert nbt.cpu().tolist() == [nbt0 + 1 if running else nbt0] + [777] * PAD
    got = {n: t[:C].cpu() for n, t in zip(FR.FIN_OUTPUTS, o)}
    if running:
        got.update(rmean=rm[:C].cpu(), rvar=rv[:C].cpu())
    else:  # the running statistics are not touched
        assert torch.equal(rm[:C].cpu(), d["rmean"]) and torch.equal(rv[:C].cpu(), d["rvar"])
    assert torch.equal(gam.cpu(), d["gamma"]) and torch.equal(bet.cpu(), d["beta"])
    return got, o + [rm, rv, nbt]


@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_bn_finalize(G, C):
    d = K.fin_case(G, C)
    part = d["part"].to(DEV)
    got, bufs = _finalize(part, C, G, d["M"], d["tile"], d)
    _note("bn_finalize", _form(G), FR.check_bn_finalize(got, d["ref"], G, f"bn_finalize G={G} C={C}"))
    _, again = _finalize(part, C, G, d["M"], d["tile"], d)
    _same_bits(bufs, again, "bn_finalize")
    # without running statistics: the four coefficient vectors are the same bits, nothing else is written
    _, bufs0 = _finalize(part, C, G, d["M"], d["tile"], d, running=False)
    _same_bits(bufs[:4], bufs0[:4], "bn_finalize without running statistics")
    assert torch.equal(part.cpu(), d["part"]), "bn_finalize changed its partials"


def test_bn_finalize_single_pixel():
    """M = 1, G = 1: variance 0, the running variance takes the biased one"""
    C = 5
    d = K.stats_rows("one", 1, C, 256, 1)
    d.update(K.bn_params("one", C))
    ref = FR.bn_finalize_rows(d["part"], 1, 256, d["gamma"], d["beta"], d["rmean"], d["rvar"], K.MOMENTUM, K.EPS)
    got, _ = _finalize(d["part"].to(DEV), C, 1, 1, 256, d)
    _note("bn_finalize M=1", "one", FR.check_bn_finalize(got, ref, 1, "bn_finalize M=1"))


# ------------------------------------------------------------------------------------------------
# unetseg_bn_bwd_finalize_rows, unetseg_bn_bwd_finalize_rows_res, unetseg_colsum_rows
# ------------------------------------------------------------------------------------------------
FORMS = {"rows": None, "res1": 1, "res2": 2}


def _bwd(form, part, C, G, d):
    """one launch of the plain or the residual form -> (got, every buffer).  The coefficient table always has six
    rows; the rows the form does not own keep the sentinel.  nbranch == 1 passes 0 for the second branch."""
    from unetseg_hip.lib import lib
    nb = FORMS[form]
    nbr = nb or 1
    g, inv = [t.to(DEV) for t in d["g"]], [t.to(DEV) for t in d["inv"]]
    dg, db = [_out(C, t) for t in d["dg0"]], [_out(C, t) for t in d["db0"]]
    coef = _out(6 * C)
    coef[3 * nbr * C:6 * C] = R.SENTINEL
    if nb is None:
        lib.bn_bwd_finalize_rows(part.data_ptr(), C, G, d["M"], g[0].data_ptr(), inv[0].data_ptr(), dg[0].data_ptr(),
                                 db[0].data_ptr(), coef.data_ptr(), _st())
    else:
        b2 = (g[1].data_ptr(), inv[1].data_ptr(), dg[1].data_ptr(), db[1].data_ptr()) if nb == 2 else (0, 0, 0, 0)
        lib.bn_bwd_finalize_rows_res(part.data_ptr(), C, G, d["M"], nb, g[0].data_ptr(), inv[0].data_ptr(),
                                     dg[0].data_ptr(), db[0].data_ptr(), *b2, coef.data_ptr(), _st())
    torch.cuda.synchronize()
    R.assert_tail(coef, 3 * nbr * C, R.SENTINEL, f"{form} coef (rows past {3 * nbr} included)")
    got = dict(coef=coef[:3 * nbr * C].cpu().view(3 * nbr, C))
    for b in range(2):
        R.assert_tail(dg[b], C, R.SENTINEL, f"{form} dgamma{b + 1}")
        R.assert_tail(db[b], C, R.SENTINEL, f"{form} dbeta{b + 1}")
        if b < nbr:
            got[f"dgamma{b + 1}"], got[f"dbeta{b + 1}"] = dg[b][:C].cpu(), db[b][:C].cpu()
        else:  # the branch the call does not have keeps its old values
            assert torch.equal(dg[b][:C].cpu(), d["dg0"][b]) and torch.equal(db[b][:C].cpu(), d["db0"][b])
    for b in range(2):
        assert torch.equal(g[b].cpu(), d["g"][b]) and torch.equal(inv[b].cpu(), d["inv"][b])
    return got, dg + db + [coef]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_bn_bwd_finalize(G, C, form):
    nb = FORMS[form]
    d = K.bwd_rows(form, G, C, 2 if nb is None else 1 + nb)
    ref = K.bwd_ref(d, nb)
    part = d["part"].to(DEV)
    got, bufs = _bwd(form, part, C, G, d)
    _note(f"bn_bwd_finalize_{form}", _form(G), FR.check_bn_bwd(got, ref, G, f"{form} G={G} C={C}"))
    if nb == 2:  # both branches from the same sum of dz
        assert torch.equal(got["coef"][4].view(torch.int32), got["coef"][1].view(torch.int32))
    _, again = _bwd(form, part, C, G, d)
    _same_bits(bufs, again, form)
    assert torch.equal(part.cpu(), d["part"]), f"{form} changed its partials"


@pytest.mark.parametrize("G,C", K.FIN_CASES)
def test_colsum_rows(G, C):
    from unetseg_hip.lib import lib
    d = K.bwd_rows("colsum", G, C, 2)
    part = d["part"].to(DEV)
    for k in (0, 1):
        for acc in (0, 1):
            outs = [_out(C, d["db0"][0]) for _ in range(2)]
            for o in outs:
                lib.colsum_rows(part.data_ptr(), C, G, k, o.data_ptr(), acc, _st())
            torch.cuda.synchronize()
            R.assert_tail(outs[0], C, R.SENTINEL, "colsum_rows out")
            r = FR.check_colsum(outs[0][:C], d["part"][:, k], acc, d["db0"][0], f"colsum_rows G={G} C={C} k={k} acc={acc}")
            _note("colsum_rows", _form(G), {f"acc{acc}": r})
            _same_bits(outs[:1], outs[1:], "colsum_rows")


# ------------------------------------------------------------------------------------------------
# unetseg_fin_merge_rows
# ------------------------------------------------------------------------------------------------
def _merge(part, C, G, M, tile, nq):
    from unetseg_hip.lib import lib
    G2 = (G + FR.MERGE_R - 1) // FR.MERGE_R
    outs = [_out(G2 * nq * C) for _ in range(2)]
    for o in outs:
        lib.fin_merge_rows(part.data_ptr(), C, G, M, tile, nq, o.data_ptr(), _st())
    torch.cuda.synchronize()
    R.assert_tail(outs[0], G2 * nq * C, R.SENTINEL, "fin_merge_rows out")
    _same_bits(outs[:1], outs[1:], "fin_merge_rows")
    return outs[0], G2


@pytest.mark.parametrize("G,C,tile,last", K.MERGE_CASES)
def test_fin_merge_rows(G, C, tile, last):
    d = K.stats_rows("merge", G, C, tile, last)
    part = d["part"].to(DEV)
    out, G2 = _merge(part, C, G, d["M"], tile, 2)
    ref, mag, _ = FR.merge_rows_chan(d["part"], G, d["M"], tile)
    r = FR.check_merge(out[:G2 * 2 * C].cpu().view(G2, 2, C), ref, mag, True, f"Chan merge G={G} C={C} tile={tile}")
    _note("fin_merge_rows", "-", {"chan": r})
    assert torch.equal(part.cpu(), d["part"])
    for nq in (2, 3):
        rows = K.bwd_rows("merge", G, C, nq)["part"]
        out, G2 = _merge(rows.to(DEV), C, G, 0, 0, nq)
        ref, mag = FR.merge_rows(rows, G, nq)
        r = FR.check_merge(out[:G2 * nq * C].cpu().view(G2, nq, C), ref, mag, False, f"plain merge nq={nq} G={G} C={C}")
        _note("fin_merge_rows", "-", {f"plain{nq}": r})


# ------------------------------------------------------------------------------------------------
# the chain: merge -> finalize, judged against the reference of the unmerged rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,C", K.CHAIN_CASES)
def test_chain_merge_bn_finalize(G, C):
    d = K.fin_case(G, C)
    _, _, more = K.chain_more_stats(d["part"], G, d["M"], d["tile"], d["ref"])
    merged, G2 = _merge(d["part"].to(DEV), C, G, d["M"], d["tile"], 2)
    got, _ = _finalize(merged, C, G2, d["M"], d["tile"] * FR.MERGE_R, d)
    _note("merge -> bn_finalize", _form(G2), FR.check_bn_finalize(got, d["ref"], G, f"chain G={G} C={C}", more))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("G,C", K.CHAIN_CASES)
def test_chain_merge_bn_bwd_finalize(G, C, form):
    nb = FORMS[form]
    nq = 2 if nb is None else 1 + nb
    d = K.bwd_rows(form, G, C, nq)
    ref = K.bwd_ref(d, nb)
    merged, G2 = _merge(d["part"].to(DEV), C, G, 0, 0, nq)
    got, _ = _bwd(form, merged, C, G2, d)
    _note(f"merge -> bn_bwd_finalize_{form}", _form(G2),
          FR.check_bn_bwd(got, ref, G, f"chain {form} G={G} C={C}", K.chain_more_sums(d["part"], G, nq)))


def test_merge_rows_picks_the_merged_path_above_the_threshold(monkeypatch):
    """ops._merge_rows: the rows as they are up to FIN_MERGE_MIN, merged 16 to 1 with tile * 16 above it"""
    from unetseg_hip import ops
    ctx = types.SimpleNamespace(f32=lambda *s: torch.empty(s, dtype=torch.float32, device=DEV), stream=_st())
    monkeypatch.setattr(ops, "FIN_MERGE", True)
    C, tile = 3, 16
    for thr in (ops.FIN_MERGE_MIN, 40):
        monkeypatch.setattr(ops, "FIN_MERGE_MIN", thr)
        for G in (thr - 1, thr, thr + 1, thr + 17):
            d = K.stats_rows("ops", G, C, tile, 5)
            part = d["part"].to(DEV)
            out, rows, t = ops._merge_rows(ctx, part, C, G, 2, d["M"], tile)
            torch.cuda.synchronize()
            if G <= thr:
                assert out is part and (rows, t) == (G, tile), (thr, G)
                continue
            assert (rows, t) == ((G + 15) // 16, tile * 16) and tuple(out.shape) == (rows, 2, C), (thr, G)
            ref, mag, _ = FR.merge_rows_chan(d["part"], G, d["M"], tile)
            FR.check_merge(out.cpu(), ref, mag, True, f"ops._merge_rows G={G}")
            rows3 = K.bwd_rows("ops", G, C, 3)["part"]
            out3, n3, t3 = ops._merge_rows(ctx, rows3.to(DEV), C, G, 3)
            torch.cuda.synchronize()
            assert (n3, t3) == ((G + 15) // 16, 0)
            ref3, mag3 = FR.merge_rows(rows3, G, 3)
            FR.check_merge(out3.cpu(), ref3, mag3, False, f"ops._merge_rows plain G={G}")
