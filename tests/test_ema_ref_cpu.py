"""CPU proof of tests/ema_ref.py: the fp32 emulation of the fused Adam + EMA kernel's operation order stays inside the
derived per-element bound against the float64 reference, contracted or not; every listed mutant of the average
leaves it on the same inputs; the warm-up rule, on both sides of its crossover; and the host's 1 - d_t
(unetseg_hip.arena.ema_one_minus_decay, what FusedAdam hands unetseg_adam_ema) is the reference's."""
import itertools

import pytest
import torch

import adam_ref as A
import ema_ref as E

N = 10007
LR, EPS = 1e-3, 1e-8
BETAS = (0.9, 0.999)
STEPS = (1, 1000)
WDS = (0.0, 1e-4)
SCALES = (None, 65536.0)
DECAYS = (0.9, 0.999)


def _case(step, wd, scale, decay, warmup, seed=11):
    inp = A.make_inputs(N, seed, wd, scale) + (E.make_ema(N, seed, wd, scale),)
    omd = E.one_minus_decay(decay, warmup, step)
    return inp, E.ema_ref(*inp, step, LR, *BETAS, EPS, wd, omd, scale)


def _emulate(inp, step, wd, scale, decay, warmup, **kw):
    return E.ema_emulate_fp32(*inp, step, LR, *BETAS, EPS, wd, decay, warmup, scale, **kw)


def test_average_inputs_hold_the_edge_cases():
    p = A.make_inputs(N, 11, 1e-4, None)[0]
    e = E.make_ema(N, 11, 1e-4, None)
    z = A.block_kind(N) == 1
    assert torch.equal(e[z], p[z]) and z.sum() > 1000
    rel = ((e.double() - p.double()).abs() / p.double().abs())[~z]
    assert (rel > 1.0).sum() > 500 and (rel < 1e-3).sum() > 500


def test_reference_is_the_textbook_average():
    """e' = d e + (1 - d) p' in float64, with d = 1 - omd"""
    inp, ref = _case(1000, 1e-4, None, 0.999, False)
    d = 1.0 - ref.omd
    torch.testing.assert_close(ref.ema, d * ref.ema_in + ref.omd * ref.p, rtol=1e-14, atol=1e-300)


@pytest.mark.parametrize("t,want", [(1, 2.0 / 11.0), (2, 3.0 / 12.0), (8989, 8990.0 / 8999.0), (8991, None),
                                    (9990, None), (100000, None)])
def test_warmup_rule(t, want):
    """decay 0.999: (1 + t) / (10 + t) below the crossover t = 8990, the decay (as fp32) above it; at 8990 itself
    the two agree to 1.3e-8, the distance of float32(0.999) from 0.999"""
    d = E.decay_at(0.999, True, t)
    assert d == (A.f32(0.999) if want is None else want)
    assert E.decay_at(0.999, False, t) == A.f32(0.999)
    assert (t < 8990) == (d < A.f32(0.999))
    assert abs(E.decay_at(0.999, True, 8990) - 0.999) < 2e-8
    assert E.one_minus_decay(0.999, True, t) == A.f32(1.0 - d)


@pytest.mark.parametrize("t", [1, 2, 12, 8989, 8990, 8991, 9990, 100000])
def test_host_rule_is_the_reference(t):
    from unetseg_hip.arena import ema_one_minus_decay
    for decay, warmup in itertools.product(DECAYS + (0.0,), (True, False)):
        assert A.f32(ema_one_minus_decay(decay, warmup, t)) == E.one_minus_decay(decay, warmup, t)


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("step", STEPS)
def test_emulation_inside_bound(step, contract):
    worst = 0.0
    for wd, scale, decay, warmup in itertools.product(WDS, SCALES, DECAYS, (True, False)):
        inp, ref = _case(step, wd, scale, decay, warmup)
        got = _emulate(inp, step, wd, scale, decay, warmup, contract=contract)
        assert all(x <= 1.0 for x in A.ratios(*got[:3], ref))
        r = E.ratio(got[3], ref.ema, E.ema_bound(ref))
        assert r <= 1.0, (step, wd, scale, decay, warmup, contract, r)
        worst = max(worst, r)
        if wd == 0.0:  # the zero block: p' = p = e, so the average does not move
            z = A.block_kind(N) == 1
            assert torch.equal(got[3][z], inp[4][z])
    print(f"step {step} contract {contract}: worst |err| / bound of the average {worst:.3f}")
    assert worst > 0.02, worst  # a bound the correct arithmetic does not come near would mean little


def test_one_ulp_on_the_device_coefficient_is_inside_the_bound():
    """unetseg_adam_ema_dev forms 1 - d_t on the device: one fp32 ulp either way stays inside the bound"""
    import numpy as np
    step, wd, scale, decay = 2, 1e-4, None, 0.999
    inp, ref = _case(step, wd, scale, decay, True)
    pn = A.adam_emulate_fp32(*inp[:4], step, LR, *BETAS, EPS, wd, scale)[0]
    e = inp[4]
    for way in (-4.0, 4.0):
        omd = torch.tensor(float(np.nextafter(np.float32(ref.omd), np.float32(way))), dtype=torch.float32)
        assert float(omd) != ref.omd
        assert E.ratio(e + omd * (pn - e), ref.ema, E.ema_bound(ref)) <= 1.0


# (step, warmup) at which each mutant differs from the kernel: the two warm-up mutants at t = 1, where the ramp
# (2 / 11) is far from either decay
MUTANT_CASES = {
    "decay_swapped": list(itertools.product(STEPS, (True, False))), "old_p": list(itertools.product(STEPS, (True, False))),
    "overwrite": list(itertools.product(STEPS, (True, False))), "warmup_ignored": [(1, True)], "warmup_forced": [(1, False)],
}


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_mutants_leave_the_bound(mutant, contract):
    assert set(MUTANT_CASES) == set(E.MUTANTS)
    for (step, warmup), wd, scale, decay in itertools.product(MUTANT_CASES[mutant], WDS, SCALES, DECAYS):
        inp, ref = _case(step, wd, scale, decay, warmup)
        got = _emulate(inp, step, wd, scale, decay, warmup, contract=contract, mutant=mutant)
        assert all(x <= 1.0 for x in A.ratios(*got[:3], ref))  # the Adam part is the kernel's
        r = E.ratio(got[3], ref.ema, E.ema_bound(ref))
        assert r > 1.0, f"{mutant} passes at step {step} warmup {warmup} wd {wd} scale {scale} decay {decay}: {r}"
