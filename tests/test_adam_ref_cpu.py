"""CPU proof of tests/adam_ref.py: the fp32 emulation of adam_kernel's operation order stays inside the derived
per-element bounds against the float64 reference, contracted or not, and every listed mutant of it leaves them
on the same inputs -- so the bounds the GPU contract tests apply are neither too tight for correct fp32
arithmetic nor loose enough to admit a wrong Adam."""
import itertools

import pytest
import torch

import adam_ref as A

N = 10007
LR, EPS = 1e-3, 1e-8
STEPS = (1, 2, 100000)
WDS = (0.0, 1e-4)
SCALES = (None, 65536.0, 3.0)
BETAS = ((0.9, 0.999), (0.5, 0.9))


def _case(step, wd, scale, betas, seed=11):
    p, g, m, v = A.make_inputs(N, seed, wd, scale)
    ref = A.adam_ref(p, g, m, v, step, LR, betas[0], betas[1], EPS, wd, scale)
    return (p, g, m, v), ref


def _emulate(inp, step, wd, scale, betas, **kw):
    return A.adam_emulate_fp32(*inp, step, LR, betas[0], betas[1], EPS, wd, scale, **kw)


def test_reference_is_torch_adam():
    """adam_ref is torch.optim.Adam (coupled L2 decay), three steps from zero moments, in float64"""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(501, generator=g)
    pt = p0.clone().to(torch.float64).requires_grad_(True)
    b1, b2, wd = A.f32(0.9), A.f32(0.999), A.f32(1e-4)
    opt = torch.optim.Adam([pt], lr=A.f32(LR), betas=(b1, b2), eps=A.f32(EPS), weight_decay=wd)
    p, m, v = p0.to(torch.float64), torch.zeros(501, dtype=torch.float64), torch.zeros(501, dtype=torch.float64)
    for step in range(1, 4):
        gr = torch.randn(501, generator=g)
        pt.grad = gr.to(torch.float64)
        opt.step()
        r = A.adam_ref(p, gr, m, v, step, LR, 0.9, 0.999, EPS, 1e-4)
        p, m, v = r.p, r.m, r.v
    # the reference rounds the two bias coefficients to fp32 as the kernels do: 2^-24 relative on the update
    torch.testing.assert_close(p, pt.detach(), rtol=0, atol=4 * A.U * A.f32(LR) * 4)
    st = opt.state[pt]
    # double rounding noise only (m is a difference of O(1) terms: absolute, a few 2^-53)
    torch.testing.assert_close(m, st["exp_avg"], rtol=0, atol=1e-14)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=0)


def test_grad_scale_divides():
    p, g, m, v = A.make_inputs(300, 5, 0.0, 8.0)
    a = A.adam_ref(p, g, m, v, 2, LR, 0.9, 0.999, EPS, 0.0, 8.0)
    b = A.adam_ref(p, g / 8.0, m, v, 2, LR, 0.9, 0.999, EPS, 0.0, None)
    for x, y in ((a.p, b.p), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(x, y)


def test_inputs_hold_the_edge_blocks():
    p, g, m, v = A.make_inputs(N, 11, 1e-4, 3.0)
    kind = A.block_kind(N)
    assert (kind == 1).sum() > 1000 and (kind == 2).sum() > 1000
    z = kind == 1
    assert not g[z].any() and not m[z].any() and not v[z].any()
    assert (v >= 0).all() and (m[kind == 0] != 0).all() and (v[kind == 0] > 0).all()
    gr = g.double() / A.f32(3.0) + A.f32(1e-4) * p.double()
    c = kind == 2
    assert ((m.double() - gr).abs()[c] <= 4.5 * 2.0 ** -23 * gr.abs()[c]).all()
    for t in (p, g):  # about six decades
        a = t[kind == 0].abs()
        assert a.quantile(0.99) / a.quantile(0.01) > 1e5


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("step", STEPS)
def test_emulation_inside_bounds(step, contract):
    worst = [0.0, 0.0, 0.0]
    for wd, scale, betas in itertools.product(WDS, SCALES, BETAS):
        inp, ref = _case(step, wd, scale, betas)
        got = _emulate(inp, step, wd, scale, betas, contract=contract)
        r = A.ratios(*got, ref)
        assert all(x <= 1.0 for x in r), (step, wd, scale, betas, contract, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
        if wd == 0.0:  # the zero block: no gradient, no moments, no decay -> the parameter does not move
            z = A.block_kind(N) == 1
            assert torch.equal(got[0][z], inp[0][z]) and not got[1][z].any() and not got[2][z].any()
    print(f"step {step} contract {contract}: worst |err| / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    # a bound the correct arithmetic does not come near would be too loose to mean much
    assert min(worst) > 0.02, worst


# the steps at which each mutant differs from Adam at all: at t = 100000 both bias coefficients are exactly 1 in
# fp32 (0.999^100000 ~ e^-100), so the three bias mutants ARE the kernel there
MUTANT_STEPS = {
    "eps_in_sqrt": STEPS, "bc2_no_sqrt": (1, 2), "no_bias_correction": (1, 2), "decoupled_wd": STEPS,
    "wd_after_moments": STEPS, "scale_multiplied": STEPS, "betas_swapped_in_v": STEPS,
}


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutants_leave_the_bounds(mutant, contract):
    assert set(MUTANT_STEPS) == set(A.MUTANTS)
    wd = 1e-4  # the decay mutants need a decay; the others are judged at the same one
    scales = (65536.0, 3.0) if mutant == "scale_multiplied" else SCALES
    for step, scale, betas in itertools.product(MUTANT_STEPS[mutant], scales, BETAS):
        inp, ref = _case(step, wd, scale, betas)
        got = _emulate(inp, step, wd, scale, betas, contract=contract, mutant=mutant)
        r = A.ratios(*got, ref)
        assert not all(x <= 1.0 for x in r), f"{mutant} passes at step {step} scale {scale} betas {betas}: {r}"
    if mutant in ("bc2_no_sqrt", "no_bias_correction"):
        inp, ref = _case(100000, wd, None, BETAS[0])
        a = _emulate(inp, 100000, wd, None, BETAS[0], contract=contract, mutant=mutant)
        b = _emulate(inp, 100000, wd, None, BETAS[0], contract=contract)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_dev_vs_host_bound_covers_one_ulp_coefficients():
    """adam_dev against adam: moving each fp32 bias coefficient by one ulp either way stays inside
    dev_vs_host_bound, and leaves m' and v' bit-identical"""
    import numpy as np
    step, wd, scale, betas = 2, 1e-4, 3.0, BETAS[0]
    inp, ref = _case(step, wd, scale, betas)
    base = _emulate(inp, step, wd, scale, betas)
    bc = A.bias_coeffs(*betas, step)
    orig = A.bias_coeffs
    try:
        for d1, d2 in itertools.product((-1, 1), (-1, 1)):
            moved = (float(np.nextafter(np.float32(bc[0]), np.float32(d1 * 4))),
                     float(np.nextafter(np.float32(bc[1]), np.float32(d2 * 4))))
            A.bias_coeffs = lambda *a, _m=moved: _m
            got = _emulate(inp, step, wd, scale, betas)
            assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])
            err = (got[0].double() - base[0].double()).abs()
            assert (err <= A.dev_vs_host_bound(ref.p, ref.delta)).all()
    finally:
        A.bias_coeffs = orig
