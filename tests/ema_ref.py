"""Float64 reference of the fused Adam + weight-EMA step (csrc/optim.hip: unetseg_adam_ema, unetseg_adam_ema_dev),
its per-element fp32 error bound, the warm-up rule, an fp32 emulation of the kernel's operation order with the
mutants the bound must reject, and the seeded average the CPU proof (test_ema_ref_cpu.py) and the GPU tests
(test_gpu_ema.py) share.

The operation is adam_ref.adam_ref followed by

    e' = e + (1 - d_t) (p' - e)            d_t = min(d, (1 + t) / (10 + t)) under warm-up, d otherwise

with t the step being taken and d the decay as fp32.  The reference takes 1 - d_t as the kernel receives it: formed
in double, rounded to fp32 once, widened back.
"""
import functools
import math

import torch

import adam_ref as A
from adam_ref import F32, F64, U, f32

# fp32 roundings of the EMA line: the difference p' - e, the product with 1 - d_t, the sum (the last two are one
# under FMA contraction); every intermediate is at most |e| + |p'| since 1 - d_t <= 1.  The count is doubled once,
# which also covers one ulp (2 U) on the 1 - d_t the capturable kernel forms on the device.
K_E = 2 * 3


def decay_at(decay, warmup, t):
    """d_t in double, from the decay as fp32"""
    d = f32(decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def one_minus_decay(decay, warmup, t):
    """1 - d_t as the kernel receives it (fp32, widened to double)"""
    return f32(1.0 - decay_at(decay, warmup, t))


def ema_ref(p, g, m, v, e, step, lr, b1, b2, eps, wd, omd, grad_scale=None):
    """adam_ref's namespace with ema (the new average), ema_in and omd added.  omd: 1 - d_t (rounded to fp32 here,
    a no-op on a value from one_minus_decay)."""
    r = A.adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale)
    r.omd = f32(omd)
    r.ema_in = e.detach().cpu().to(F64)
    r.ema = r.ema_in + r.omd * (r.p - r.ema_in)
    return r


def ema_update_ref(e, p_new, omd):
    """the EMA line alone in float64, from a given new parameter (the optimizer-level tests: p' is the kernel's)"""
    e, p_new = e.detach().cpu().to(F64), p_new.detach().cpu().to(F64)
    return e + f32(omd) * (p_new - e)


def ema_bound(ref):
    """bound(e') = K_E U (|e| + |p'|) + (1 - d) bound(p')"""
    return own_bound(ref.ema_in, ref.p) + ref.omd * A.adam_bounds(ref)[0]


def own_bound(e, p_new):
    """the EMA line's own roundings, K_E U (|e| + |p'|): the whole bound when p' is given exactly"""
    return K_E * U * (e.detach().cpu().to(F64).abs() + p_new.detach().cpu().to(F64).abs())


def ratio(got, want, bound):
    """largest |got - want| / bound (0/0 counts as 0, x/0 as inf; NaN propagates)"""
    err = (got.detach().cpu().to(F64) - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# fp32 emulation of the EMA line on top of adam_ref.adam_emulate_fp32, and its mutants
# ------------------------------------------------------------------------------------------------
MUTANTS = ("decay_swapped", "old_p", "warmup_ignored", "warmup_forced", "overwrite")


def ema_emulate_fp32(p, g, m, v, e, step, lr, b1, b2, eps, wd, decay, warmup, grad_scale=None, contract=False,
                     mutant=None):
    """the fused kernel's expression in fp32 -> (p', m', v', e').  contract=True fuses each product with the sum
    that follows it; mutant names one wrong implementation of the average."""
    assert mutant is None or mutant in MUTANTS, mutant
    pn, mv, vv = A.adam_emulate_fp32(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale, contract=contract)
    if mutant == "warmup_ignored":
        warmup = False
    if mutant == "warmup_forced":
        warmup = True
    omd = torch.tensor(one_minus_decay(decay, warmup, step), dtype=F32)
    if mutant == "decay_swapped":
        omd = torch.tensor(1.0, dtype=F32) - omd
    e = e.detach().cpu().to(F32)
    src = p.detach().cpu().to(F32) if mutant == "old_p" else pn
    if mutant == "overwrite":
        return pn, mv, vv, pn.clone()
    d = src - e
    en = (omd.to(F64) * d.to(F64) + e.to(F64)).to(F32) if contract else e + omd * d
    return pn, mv, vv, en


# ------------------------------------------------------------------------------------------------
# seeded average
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _ema(n, seed, wd, grad_scale):
    p = A.make_inputs(n, seed, wd, grad_scale)[0]
    gen = torch.Generator().manual_seed(seed + 7919)
    rel = torch.randn(n, generator=gen, dtype=F64) * 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 4 - 4)
    e = (p.to(F64) * (1.0 + rel)).to(F32)
    own = torch.arange(n) % 5 == 0  # every fifth element: an average unrelated to the parameter
    far = (torch.randn(n, generator=gen, dtype=F64) * 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 6 - 4)).to(F32)
    e[own] = far[own]
    same = A.block_kind(n) == 1  # the zero block: the average equals the parameter (as before the first update)
    e[same] = p[same]
    return e


def make_ema(n, seed, wd=0.0, grad_scale=None):
    """fp32 CPU tensor: the average that goes with adam_ref.make_inputs(n, seed, wd, grad_scale) -- within a relative
    10^uniform(-4, 0) of p, every fifth element unrelated to p, and equal to p on the zero block (where, with
    wd = 0, neither the parameter nor the average may move).  Cached: callers must not modify it."""
    return _ema(int(n), int(seed), float(wd), None if grad_scale is None else float(grad_scale))
