"""Float64 references of the row-partial finalize family (csrc/elem.hip, csrc/fin_reduce.h): unetseg_bn_finalize,
unetseg_bn_bwd_finalize_rows, unetseg_bn_bwd_finalize_rows_res, unetseg_fin_merge_rows and unetseg_colsum_rows,
and the bounds their contract tests assert (tests/test_gpu_fin_rows_contract.py on the GPU; the references are
pinned to PyTorch, and the bounds shown reachable, on the CPU in tests/test_fin_rows_ref_cpu.py).

Written from the text of include/unetseg_hip.h in torch float64, in the style of tests/nhwc_ref.py, whose contract
helpers it reuses; nothing here imports the library or touches a GPU.

The *input* of every reference is the fp32 partial rows part[G][nq][C] themselves, exactly the bytes a kernel
reads, so the reference is the exact function of those rows and the only errors a kernel may add are its own:
the fp64 row sums (at most G 2^-53 sum|part|, added to every bound explicitly) and the fp32 roundings k after
them, in the form of nhwc_ref:

    |got - ref| <= ulp_fp32(ref) + 1.01 k 2^-24 mag + (fp64 term)

Each reference returns next to a value its magnitude, the float64 sum of the absolute values of the terms added.
"""
import torch

from nhwc_ref import EPS32, F64, SENTINEL, assert_elementwise, assert_tail, bound, f64, k_measured, ulp_store  # noqa: F401

EPS64 = 2.0 ** -53  # one float64 rounding, relative
MERGE_R = 16  # rows unetseg_fin_merge_rows merges into one


def _f32(x):
    """x (float64) rounded to fp32 once, back in float64"""
    return x.to(torch.float32).to(F64)


def row_counts(G, M, tile):
    """pixels of row g: min(tile, M - g tile), float64 [G]"""
    g = torch.arange(G, dtype=F64)
    cnt = torch.minimum(torch.full_like(g, float(tile)), float(M) - g * tile)
    assert float(cnt.min()) >= 1, (G, M, tile)
    return cnt


# ------------------------------------------------------------------------------------------------
# unetseg_bn_finalize
# ------------------------------------------------------------------------------------------------
FIN_OUTPUTS = ("mean", "invstd", "scale", "shift", "rmean", "rvar")


def bn_finalize_rows(part, M, tile, gamma, beta, rmean, rvar, momentum, eps):
    """part [G][2][C] = (sum, M2 about the row's mean) of min(tile, M - g tile) pixels per row; Chan's merge of
    the rows -> dict of mean, invstd, scale = gamma invstd, shift = beta - mean gamma invstd and the running
    statistics after one momentum step (unbiased variance; the biased one with M == 1), each with `<name>_mag`.
    Also the merge's own quantities: sum, sum_abs = sum_g |sum_g|, m2, var, and m2_mag = sum_g (M2_g + cnt_g
    (|mean_g| + |mean|)^2), which bounds the terms of a float64 evaluation (the difference mean_g - mean
    cancels)."""
    part, gamma, beta = f64(part), f64(gamma), f64(beta)
    G, two, C = part.shape
    assert two == 2
    cnt = row_counts(G, M, tile)[:, None]
    assert float(cnt.sum()) == M, (G, M, tile)
    s, q = part[:, 0], part[:, 1]
    tot = s.sum(0)
    mean = tot / M
    mg = s / cnt
    m2 = (q + cnt * (mg - mean) ** 2).sum(0)
    var = m2 / M
    inv = 1.0 / torch.sqrt(var + eps)
    unb = m2 / (M - 1) if M > 1 else var
    out = dict(sum=tot, sum_abs=s.abs().sum(0), m2=m2, var=var, unb=unb,
               m2_mag=(q.abs() + cnt * (mg.abs() + mean.abs()) ** 2).sum(0),
               mean=mean, mean_mag=s.abs().sum(0) / M, invstd=inv, invstd_mag=inv.abs(),
               scale=gamma * inv, scale_mag=(gamma * inv).abs(),
               shift=beta - mean * gamma * inv, shift_mag=beta.abs() + (mean * gamma * inv).abs(),
               gamma=gamma, M=M, momentum=momentum, eps=eps)
    if rmean is not None:
        rm0, rv0 = f64(rmean), f64(rvar)
        out.update(rmean=(1 - momentum) * rm0 + momentum * mean,
                   rmean_mag=((1 - momentum) * rm0).abs() + (momentum * mean).abs(),
                   rvar=(1 - momentum) * rv0 + momentum * unb,
                   rvar_mag=((1 - momentum) * rv0).abs() + (momentum * unb).abs())
    return out


def chan_spread(s, cnt, mean, ds, dq):
    """Rows (s, q) with counts cnt [G][1] merged about `mean`: how far perturbations |delta s_g| <= ds, |delta q_g|
    <= dq [G][C] move the total sum and the merged M2 -> (d_sum, d_m2) [C].  M2 = sum_g q_g + cnt_g (s_g / cnt_g -
    mean)^2 and sum_g cnt_g (s_g / cnt_g - mean) = 0, so to first order the shift of the mean drops out and
    delta M2 = sum_g delta q_g + 2 (s_g / cnt_g - mean) delta s_g."""
    return ds.sum(0), dq.sum(0) + (2 * (s / cnt - mean).abs() * ds).sum(0)


def bn_finalize_spread(ref, d_sum, d_m2):
    """first-order reach of |delta sum| <= d_sum, |delta M2| <= d_m2 on every output of bn_finalize_rows (times 1.01
    for the second order)"""
    M, mom, gam = ref["M"], ref["momentum"], ref["gamma"].abs()
    d_mean, d_var = d_sum / M, d_m2 / M
    d_inv = 0.5 * ref["invstd"] / (ref["var"] + ref["eps"]) * d_var
    sp = dict(mean=d_mean, invstd=d_inv, scale=gam * d_inv,
              shift=gam * (ref["mean"].abs() * d_inv + ref["invstd"] * d_mean + d_inv * d_mean),
              rmean=mom * d_mean, rvar=mom * d_m2 / max(M - 1, 1))
    return {k: 1.01 * v for k, v in sp.items()}


def _with(mag, extra, k):
    """the magnitude that makes nhwc_ref.bound add `extra` (absolute) to ulp + 1.01 k 2^-24 mag"""
    return mag + extra / (1.01 * k * EPS32)


def check_bn_finalize(got, ref, G, what, more=None):
    """got: name -> fp32 [C] for the names of FIN_OUTPUTS present.  Every output is formed in double and cast once
    (bn_finalize_kernel, elem.hip), so k = 1, the store, for each; mag as the issue sets it: |ref| for mean, invstd
    and scale, the terms added for shift and the running statistics.  The fp64 row sums enter through
    bn_finalize_spread: G 2^-53 sum|sum_g| on the sum, (G + 8) 2^-53 m2_mag on M2 (the + 8: the divide, subtract,
    square and multiply of each term).  `more`: (d_sum, d_m2) on top, for rows that were rounded on the way.
    -> name -> largest |got - ref| / bound"""
    d_sum, d_m2 = G * EPS64 * ref["sum_abs"], (G + 8) * EPS64 * ref["m2_mag"]
    if more is not None:
        d_sum, d_m2 = d_sum + more[0], d_m2 + more[1]
    sp = bn_finalize_spread(ref, d_sum, d_m2)
    mags = dict(
        mean=ref["mean"].abs(),  # k = 1: mean_out[c] = (float)mean, elem.hip:83
        invstd=ref["invstd_mag"],  # k = 1: invstd_out[c] = (float)inv, inv a double, elem.hip:82-84
        scale=ref["scale_mag"],  # k = 1: (float)(gam * inv), the product in double from the fp32 gam, elem.hip:85
        shift=ref["shift_mag"],  # k = 1: (float)(bet - mean * gam * inv) in double, elem.hip:87
        rmean=ref.get("rmean_mag"),  # k = 1: (float)((1.0 - momentum) * rm0 + momentum * mean), elem.hip:90
        rvar=ref.get("rvar_mag"))  # k = 1: (float)((1.0 - momentum) * rv0 + momentum * unb), elem.hip:91
    return {n: assert_elementwise(got[n], ref[n], _with(mags[n], sp[n], 1), torch.float32, 1, what=f"{what} {n}")
            for n in FIN_OUTPUTS if n in got}


# ------------------------------------------------------------------------------------------------
# unetseg_bn_bwd_finalize_rows, unetseg_bn_bwd_finalize_rows_res
# ------------------------------------------------------------------------------------------------
def _bn_bwd(part, M, branches):
    """part [G][1 + nb][C] = (sum dz, sum dz xhat_1 [, sum dz xhat_2]); branches: [(g, inv, dg0, db0)] * nb"""
    part = f64(part)
    G, nq, C = part.shape
    nb = len(branches)
    assert nq == 1 + nb
    sums, sabs = part.sum(0), part.abs().sum(0)
    coef = torch.zeros(3 * nb, C, dtype=F64)
    out = dict(sums=sums, sums_abs=sabs, M=M, nb=nb)
    for b, (g, inv, dg0, db0) in enumerate(branches):
        # k = g inv is the fp32 product of the fp32 inputs; both branches take dbeta and coef[1] / coef[4] from the
        # same sum of dz
        coef[3 * b] = (g.detach().cpu().to(torch.float32) * inv.detach().cpu().to(torch.float32)).to(F64)
        coef[3 * b + 1] = sums[0] / M
        coef[3 * b + 2] = sums[1 + b] / M
        dg0, db0 = f64(dg0), f64(db0)
        out[f"dgamma{b + 1}"], out[f"dgamma{b + 1}_mag"] = dg0 + sums[1 + b], dg0.abs() + sums[1 + b].abs()
        out[f"dbeta{b + 1}"], out[f"dbeta{b + 1}_mag"] = db0 + sums[0], db0.abs() + sums[0].abs()
        out[f"q{b + 1}"] = 1 + b
    out["coef"] = coef
    return out


def bn_bwd_finalize_rows(part, M, g1, inv1, dg0, db0):
    """part [G][2][C] = (sum dz, sum dz xhat) -> dict: dgamma1 = dg0 + sum_g part[g][1], dbeta1 = db0 + sum_g
    part[g][0] (mag |old| + |sum|), coef [3][C] = (g1 inv1 as the fp32 product, sum dz / M, sum dz xhat / M), sums
    and sums_abs [2][C]"""
    return _bn_bwd(part, M, [(g1, inv1, dg0, db0)])


def bn_bwd_finalize_rows_res(part, M, nbranch, g1, inv1, dg1_0, db1_0, g2=None, inv2=None, dg2_0=None, db2_0=None):
    """part [G][1 + nbranch][C] = (sum dz, sum dz xhat1 [, sum dz xhat2]) -> bn_bwd_finalize_rows's dict, with
    nbranch == 2 also dgamma2 (from part[.][2]), dbeta2 (from the same sum of dz as dbeta1) and coef rows 3..5 =
    (g2 inv2, sum dz / M, sum dz xhat2 / M)"""
    br = [(g1, inv1, dg1_0, db1_0)] + ([(g2, inv2, dg2_0, db2_0)] if nbranch == 2 else [])
    return _bn_bwd(part, M, br)


def check_bn_bwd(got, ref, G, what, more=None):
    """got: dgamma1, dbeta1 [, dgamma2, dbeta2] [C] and coef [3 nb][C] (fp32).  more: [1 + nb][C] absolute error the
    sums carry on top (rows rounded on the way).  -> name -> largest |got - ref| / bound"""
    M = ref["M"]
    d = G * EPS64 * ref["sums_abs"]
    if more is not None:
        d = d + more
    r = {}
    for b in range(ref["nb"]):
        q = 1 + b
        # k = 2: the cast of the fp64 sum, the add onto the old value (elem.hip:501-502, 532-533, 538-539)
        for name, j in ((f"dgamma{b + 1}", q), (f"dbeta{b + 1}", 0)):
            r[name] = assert_elementwise(got[name], ref[name], _with(ref[name + "_mag"], d[j], 2), torch.float32, 2,
                                         what=f"{what} {name}")
        # coef[0], coef[3]: the fp32 product of the fp32 inputs, bit for bit (elem.hip:496, 521, 526)
        g0, w0 = got["coef"][3 * b].detach().cpu().to(torch.float32), ref["coef"][3 * b].to(torch.float32)
        assert torch.equal(g0.view(torch.int32), w0.view(torch.int32)), f"{what} coef[{3 * b}] is not fl(g * inv)"
        # k = 1: (float)(sum / (double)M) (elem.hip:504-505, 535-536, 541-542)
        for row, j in ((3 * b + 1, 0), (3 * b + 2, q)):
            c = ref["coef"][row]
            r[f"coef{row}"] = assert_elementwise(got["coef"][row], c, _with(c.abs(), d[j] / M, 1), torch.float32, 1,
                                                 what=f"{what} coef[{row}]")
    return r


# ------------------------------------------------------------------------------------------------
# unetseg_fin_merge_rows, unetseg_colsum_rows
# ------------------------------------------------------------------------------------------------
def _groups(part, G, R):
    """[G][nq][C] -> [G2][R][nq][C] zero-padded, and the bool [G2][R] of the rows that exist"""
    part = f64(part)
    assert part.shape[0] == G
    G2 = (G + R - 1) // R
    pad = torch.zeros((G2 * R,) + tuple(part.shape[1:]), dtype=F64)
    pad[:G] = part
    live = (torch.arange(G2 * R) < G).view(G2, R)
    return pad.view((G2, R) + tuple(part.shape[1:])), live


def merge_rows(part, G, nq, R=MERGE_R):
    """plain float64 sums of each group of R consecutive rows -> (out [ceil(G/R)][nq][C], mag = the sums of |.|)"""
    assert part.shape[1] == nq
    grp, _ = _groups(part, G, R)
    return grp.sum(1), grp.abs().sum(1)


def merge_rows_chan(part, G, M, tile, R=MERGE_R):
    """(sum, M2 about the merged mean) of each group of R rows of `tile` pixels, the last row min(tile, M - g tile)
    -> (out [ceil(G/R)][2][C], mag [..][2][C], cnt2 [ceil(G/R)] the merged rows' pixel counts); mag as
    bn_finalize_rows's sum_abs and m2_mag"""
    grp, live = _groups(part, G, R)
    G2 = grp.shape[0]
    cnt = torch.ones(G2 * R, dtype=F64)
    cnt[:G] = row_counts(G, M, tile)
    cnt = cnt.view(G2, R, 1)
    lv = live.view(G2, R, 1).to(F64)
    s, q = grp[:, :, 0], grp[:, :, 1]
    n = (cnt * lv).sum(1)
    tot = s.sum(1)
    mean = (tot / n).unsqueeze(1)
    mg = s / cnt
    m2 = (lv * (q + cnt * (mg - mean) ** 2)).sum(1)
    mag2 = (lv * (q.abs() + cnt * (mg.abs() + mean.abs()) ** 2)).sum(1)
    return torch.stack([tot, m2], 1), torch.stack([s.abs().sum(1), mag2], 1), n[:, 0]


def check_merge(got, ref, mag, chan, what, R=MERGE_R):
    """merged rows [G2][nq][C]: k = 1, the cast of the fp64 value (elem.hip:615-616, 624), mag = |ref|; the fp64 term
    R 2^-53 mag (+ 8 for the Chan terms' own operations)"""
    e = ((R + 8) if chan else R) * EPS64 * mag
    return assert_elementwise(got, ref, _with(ref.abs(), e, 1), torch.float32, 1, what=what)


def check_colsum(got, part_k, accumulate, out0, what):
    """out[c] (+)= sum_g part_k[g][c]: k = 2 (the cast, the add; elem.hip:561), mag = |old| + |sum|"""
    part_k = f64(part_k)
    G = part_k.shape[0]
    v = part_k.sum(0)
    m = v.abs()
    if accumulate:
        v, m = v + f64(out0), m + f64(out0).abs()
    return assert_elementwise(got, v, _with(m, G * EPS64 * part_k.abs().sum(0), 2), torch.float32, 2, what=what)
