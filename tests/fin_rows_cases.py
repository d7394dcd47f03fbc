"""Cases and data of the row-partial finalize contract (tests/test_gpu_fin_rows_contract.py), shared with the CPU
file that proves the bounds reachable on every one of them (tests/test_fin_rows_ref_cpu.py).  CPU only, seeded
per case id, built in float64.

Row counts, from the switches of csrc/fin_reduce.h (kFinRPL = 8 rows per lane per round, one wave per channel up
to G = 512, four waves above): 1, 2, 7 (fewer rows than lanes); 63, 64, 65 (one wave's lanes); 511, 512 (the
last one-wave size, exactly one full round of 8 x 64); 513 (the first four-wave size); 2047, 2048, 2049 (one full
four-wave round of 8 x 256, then the second round, where bn_finalize's pass 2 re-reads the rows); 4097 (three
rounds, the last nearly empty).  Channel counts 1, 3, 4, 5, 64, 67, 260: the one-wave form's blocks of four
channels with their c >= C exits, odd counts in the one-block-per-channel form.  Every G meets two or three C,
every C at least three G.
"""
import zlib

import torch

import fin_rows_ref as FR

F64 = torch.float64

FIN_G = (1, 2, 7, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
FIN_C = (1, 3, 4, 5, 64, 67, 260)
FIN_CASES = [(1, 1), (1, 5), (2, 3), (2, 64), (7, 4), (7, 260), (63, 5), (63, 67), (64, 1), (64, 260), (65, 3),
             (65, 64), (511, 4), (511, 67), (512, 5), (512, 64), (513, 1), (513, 260), (2047, 3), (2047, 4),
             (2048, 5), (2048, 67), (2049, 1), (2049, 64), (4097, 3), (4097, 67)]
CHAIN_CASES = [(G, C) for G, C in FIN_CASES if G in (2049, 4097)]

MERGE_G = (1, 15, 16, 17, 63, 64, 65, 601, 1009)
MERGE_C = (1, 63, 64, 65, 130)
_MERGE_GC = [(1, 1), (1, 64), (15, 63), (15, 130), (16, 64), (16, 65), (17, 1), (17, 130), (63, 63), (63, 65), (64, 64),
             (64, 1), (65, 65), (65, 130), (601, 63), (601, 130), (1009, 1), (1009, 65)]


def _chan_geometry(i, G):
    """tile in {128, 256} (128 at the two largest G: the pixel data stays small) and a last row of 1, 37 or tile
    pixels, cycled over the cases so that all six combinations occur"""
    tile = 128 if G >= 601 else (128, 256)[i % 2]
    return tile, (1, 37, tile)[i % 3]


#: (G, C, tile, last row's pixels) of the Chan form; the plain forms run nq = 2 and nq = 3 at every (G, C)
MERGE_CASES = [(G, C) + _chan_geometry(i, G) for i, (G, C) in enumerate(_MERGE_GC)]

MOMENTUM = float(torch.tensor(0.1, dtype=torch.float32))  # the fp32 values the C ABI's float arguments hold
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
NBT0 = 41


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def stats_geometry(G):
    """(tile, last row's pixels) of a bn_finalize case: 256-pixel rows while the pixel data stays small, 16-pixel
    rows above; the last row ragged"""
    return (256, 37) if G <= 65 else (16, 5)


def stats_rows(seed, G, C, tile, last):
    """Statistics rows from real pixel data x = mu_c + sigma_c randn, mu_c / sigma_c spread over {0, 1, 30} across
    the channels (either sign): a merge that is not Chan's, or one in fp32, fails on the 30s.  The partials (sum,
    M2 about the row's mean) are formed in float64 and rounded to fp32.
    -> dict: part fp32 [G][2][C], M, x (float64 [M][C])"""
    g = gen("stats", seed, G, C, tile, last)
    M = (G - 1) * tile + last
    c = torch.arange(C)
    ratio = torch.tensor([0.0, 1.0, 30.0], dtype=F64)[(c + G) % 3] * torch.where((c // 3) % 2 == 0, 1.0, -1.0).to(F64)
    sigma = 0.5 + torch.rand(C, generator=g, dtype=F64)
    x = ratio * sigma + sigma * torch.randn(M, C, generator=g, dtype=F64)
    part = torch.zeros(G, 2, C, dtype=F64)
    if G > 1:
        t = x[:(G - 1) * tile].view(G - 1, tile, C)
        part[:G - 1, 0] = t.sum(1)
        part[:G - 1, 1] = ((t - t.mean(1, keepdim=True)) ** 2).sum(1)
    t = x[(G - 1) * tile:]
    part[G - 1, 0] = t.sum(0)
    part[G - 1, 1] = ((t - t.mean(0, keepdim=True)) ** 2).sum(0)
    return dict(part=part.to(torch.float32), M=M, x=x)


def bn_params(seed, C):
    """gamma, beta and non-zero running statistics (fp32)"""
    g = gen("bn", seed, C)
    return dict(gamma=(torch.rand(C, generator=g) + 0.5), beta=torch.randn(C, generator=g),
                rmean=torch.randn(C, generator=g), rvar=torch.rand(C, generator=g) + 0.5)


def bwd_rows(seed, G, C, nq):
    """Backward rows: randn plus a per-channel offset in {0, +0.5, -0.5} (the sums are not all cancellation), the
    branch coefficients and non-zero old dgamma / dbeta.
    -> dict: part fp32 [G][nq][C], M, g / inv / dg0 / db0: two fp32 [C] each (one per branch)"""
    g = gen("bwd", seed, G, C, nq)
    off = torch.tensor([0.0, 0.5, -0.5])[(torch.arange(C) + G) % 3]
    part = torch.randn(G, nq, C, generator=g) + off
    r = lambda lo: [torch.rand(C, generator=g) + lo for _ in range(2)]  # noqa: E731
    n = lambda: [torch.randn(C, generator=g) for _ in range(2)]  # noqa: E731
    return dict(part=part, M=G * 128 - 3, g=r(0.5), inv=r(0.5), dg0=n(), db0=n())


def fin_case(G, C):
    """One bn_finalize case: the rows, the parameters and the float64 reference.

    beta is placed so that shift = beta - t, t = mean gamma invstd, is a sum without cancellation and |beta| >=
    2 |t|.  The bound of shift has k = 1 (the kernel forms t in double): with u = 2^-24 and ulp(shift) > u |shift|
    it is ulp + 1.01 u (|beta| + |t|).  An implementation that rounds every multiply and divide to fp32 carries on
    t the roundings of mean (u), mean gamma (u), invstd (u / 2 from the variance, u its own) and the last product
    (u), and half an ulp of the store: 4.5 u |t| + ulp / 2, within the bound once 1.51 (|beta| + |t|) >= 4.5 |t|,
    |beta| >= 1.98 |t|.  With beta = randn the channels of |mean| / std = 30 leave such an implementation a few
    per cent outside (the condition tests/test_fin_rows_ref_cpu.py checks on every case); the kernel's own bound
    does not depend on the choice."""
    tile, last = stats_geometry(G)
    d = stats_rows("fin", G, C, tile, last)
    d.update(bn_params(("fin", G), C), tile=tile)
    t = FR.bn_finalize_rows(d["part"], d["M"], tile, d["gamma"], d["beta"], None, None, MOMENTUM, EPS)["shift_mag"] - \
        d["beta"].to(F64).abs()
    sign = torch.where(d["part"][:, 0].to(F64).sum(0) * d["gamma"].to(F64) < 0, 1.0, -1.0).to(F64)
    d["beta"] = (sign * (d["beta"].to(F64).abs() + 2.0 * t)).to(torch.float32)
    d["ref"] =FR.bn_finalize_rows(d["part"], d["M"], tile, d["gamma"], d["beta"], d["rmean"], d["rvar"], MOMENTUM,
                                   EPS)
    return d


def bwd_ref(d, nbranch=None):
    """the reference of a bwd_rows dict: the plain form (nbranch None) or the residual form"""
    a = (d["g"][0], d["inv"][0], d["dg0"][0], d["db0"][0])
    if nbranch is None:
        return FR.bn_bwd_finalize_rows(d["part"], d["M"], *a)
    b = (d["g"][1], d["inv"][1], d["dg0"][1], d["db0"][1]) if nbranch == 2 else ()
    return FR.bn_bwd_finalize_rows_res(d["part"], d["M"], nbranch, *a, *b)


def chain_more_stats(part, G, M, tile, ref):
    """The merged statistics rows are rounded to fp32 before bn_finalize reads them: one rounding per merged value,
    2^-24 |value|, carried to the sum and to M2 by chan_spread -> (merged reference rows, their counts, (d_sum,
    d_m2) for check_bn_finalize)"""
    mref, _, cnt2 = FR.merge_rows_chan(part, G, M, tile)
    s2, q2 = mref[:, 0], mref[:, 1]
    return mref, cnt2, FR.chan_spread(s2, cnt2[:, None], ref["mean"], FR.EPS32 * s2.abs(), FR.EPS32 * q2.abs())


def chain_more_sums(part, G, nq):
    """the same for the plain merge: 2^-24 sum_g2 |merged value| per quantity, [nq][C]"""
    mref, _ = FR.merge_rows(part, G, nq)
    return FR.EPS32 * mref.abs().sum(0)
