"""Float64 reference of the fused Adam step (csrc/optim.hip), its per-element fp32 error bounds, an fp32
emulation of the kernel's operation order with the mutants the bounds must reject, and the seeded inputs the
CPU proof (test_adam_ref_cpu.py) and the GPU contract tests (test_gpu_adam_contract.py) share.

The operation is torch.optim.Adam with coupled L2 weight decay (train.py:62-78):

    gr    = g / grad_scale + wd p             (grad_scale: the loss scale the gradient carries; GradScaler's unscale)
    m'    = m + (1 - b1) (gr - m)
    v'    = b2 v + (1 - b2) gr^2
    denom = sqrt(v') / sqrt(1 - b2^t) + eps
    p'    = p - (lr / (1 - b1^t)) m' / denom

The reference takes every hyperparameter as the kernel receives it -- rounded to fp32, then widened to double
(1 - float32(0.999) is 1.3e-5 away from 0.001: parameter quantisation, not arithmetic error) -- and the two bias
coefficients bc1 = 1 - b1^t and sqrt(1 - b2^t) computed in double and rounded to fp32, as both kernels do.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24  # fp32 unit roundoff: one rounding to nearest moves a value by at most U |value|
F64 = torch.float64
F32 = torch.float32

# fp32 roundings of adam_kernel, per path (the K of each bound is the count doubled once for margin)
KG = 4   # gr: 1/grad_scale, g * inv_scale, wd * p, the sum                      (the last two are one under FMA)
KM = 8   # m': the four of gr, gr - m, 1 - b1, the product, the sum                (the last two are one under FMA)
KV5 = 5  # v' without gr's error: v * b2, 1 - b2, (1 - b2) * gr, * gr, the sum
KD = 10  # the update without the errors of m' and v': sqrt, / bc2_sqrt, + eps, lr / bc1, m' / denom, the product
#          (6 roundings) and one ulp = 2 U on each of the two fp32 bias coefficients (4)
K_M = 2 * KM               # 16
K_V = 2 * (KV5 + 2 * KG)   # 26: gr enters squared, so its relative error counts twice
K_P = 2 * KD + K_V // 2    # 33: v' enters under a square root, so its relative error counts half


def f32(x):
    """a Python number as the kernel receives it: rounded to fp32, widened back to double"""
    return float(np.float32(x))


def bias_coeffs(b1, b2, step):
    """(bc1, bc2_sqrt) as unetseg_adam forms them: double arithmetic on the fp32 betas, rounded to fp32"""
    b1, b2 = f32(b1), f32(b2)
    return f32(1.0 - b1 ** step), f32(math.sqrt(1.0 - b2 ** step))


def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale=None):
    """One Adam step in float64.  p, g, m, v: fp32 (or float64) CPU tensors holding fp32 values; returns the
    new p, m, v, the update delta = p' - p and the intermediates the bounds need: gr, gr_abs = |g / scale| +
    |wd p| (the magnitude gr's roundings act on; equal to |gr| unless the two terms cancel), denom, and the
    scalars q = lr / bc1, c1 = 1 - b1, c2 = 1 - b2."""
    assert step >= 1
    p, g, m, v = (t.detach().cpu().to(F64) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    bc1, bc2s = bias_coeffs(b1, b2, step)
    gs = g if grad_scale is None else g / f32(grad_scale)
    gr = gs + wd * p if wd != 0.0 else gs
    gr_abs = gs.abs() + abs(wd) * p.abs()
    c1, c2 = 1.0 - b1, 1.0 - b2
    m2 = m + c1 * (gr - m)
    v2 = v * b2 + c2 * gr * gr
    denom = v2.sqrt() / bc2s + eps
    q = lr / bc1
    delta = -q * (m2 / denom)
    return SimpleNamespace(p=p + delta, m=m2, v=v2, delta=delta, gr=gr, gr_abs=gr_abs, denom=denom, q=q, c1=c1,
                           c2=c2, m_in=m, p_in=p)


def adam_bounds(ref):
    """Per-element bounds (bound_p, bound_m, bound_v) on |kernel - reference| for fp32 arithmetic in
    adam_kernel's order, to first order in U, every count doubled once.  Each fp32 rounding moves its result by
    at most U |result|; FMA contraction of a product and the sum that follows removes one rounding, so the
    uncontracted count covers either choice.

    gr    KG = 4 roundings (1 / grad_scale, g * inv_scale, wd * p, the sum; the reciprocal is exact for a
          power of two and counted all the same), each acting on a value no larger than
          gr_abs = |g / scale| + |wd p|:                           err(gr) <= KG U gr_abs.
          gr_abs is |gr| unless the gradient and the decay term have opposite signs; the cancellation the sum
          can then suffer is the data's, not the kernel's, and is why the bounds carry gr_abs and not |gr|.
    m'    gr - m, 1 - b1 (exact for b1 >= 0.5, counted), the product and the sum: 4 more, every intermediate
          (gr - m, (1 - b1)(gr - m), m') no larger than |m| + gr_abs since 1 - b1 <= 1:
                                     bound(m') = K_M U (|m| + gr_abs),           K_M = 2 (KG + 4) = 16.
    v'    v * b2, 1 - b2, (1 - b2) * gr, * gr, the sum: 5 roundings of non-negative terms, so 5 U v' (no
          cancellation); gr enters squared, (1 - b2) 2 |gr| err(gr):
                                     bound(v') = 2 U (5 v' + 2 KG (1 - b2) |gr| gr_abs)
          which is K_V U v' with K_V = 2 (5 + 2 KG) = 26 wherever gr_abs = |gr| (always when wd = 0).
    p'    the final subtraction rounds once, U |p'|.  The update delta = -(lr / bc1) m' / denom carries, relative
          to |delta|: sqrt, / bc2_sqrt, + eps (denom's terms are non-negative), lr / bc1, m' / denom and the
          product, 6 roundings; one ulp (2 U) on each fp32 bias coefficient, since the device pow may differ
          from the host's in the last double bit: KD = 10; and half the relative error of v' (it sits under
          the square root).  The error of m' passes through scaled by (lr / bc1) / denom:
              bound(p') = U |p'| + (2 KD U + bound(v') / (2 v')) |delta| + (lr / bc1) bound(m') / denom
          i.e. U |p'| + K_P U |delta| + (lr / bc1) bound(m') / denom with K_P = 2 KD + K_V / 2 = 33 wherever
          gr_abs = |gr|.
    No element is excluded: where v' = 0 (zero gradient, zero v) bound(v') is 0 and its term drops out."""
    bm = K_M * U * (ref.m_in.abs() + ref.gr_abs)
    bv = 2.0 * U * (KV5 * ref.v + 2.0 * KG * ref.c2 * ref.gr.abs() * ref.gr_abs)
    rel_v = torch.where(ref.v > 0, bv / (2.0 * ref.v.clamp_min(1e-300)), torch.zeros_like(bv))
    bp = U * ref.p.abs() + (2.0 * KD * U + rel_v) * ref.delta.abs() + ref.q * bm / ref.denom
    return bp, bm, bv


def dev_vs_host_bound(p_new, delta):
    """|p'(adam_dev) - p'(adam)| for equal inputs when each bias coefficient may differ by one ulp (2 U) and
    nothing else: lr / bc1 differs by 2 U plus its two roundings (4 U); sqrt(v') / bc2_sqrt likewise, + eps two
    more (6 U); m' / denom 8 U; the product 4 + 8 + 2 = 14 U of |delta|; the final subtraction rounds once on
    either side, 2 U |p'|.  m' and v' do not read the coefficients: they are bit-identical."""
    return 2.0 * U * p_new.abs() + 14.0 * U * delta.abs()


def ratios(got_p, got_m, got_v, ref):
    """largest |got - ref| / bound per output (0/0 counts as 0, x/0 as inf)"""
    out = []
    for got, want, bound in zip((got_p, got_m, got_v), (ref.p, ref.m, ref.v), adam_bounds(ref)):
        err = (got.detach().cpu().to(F64) - want).abs()
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
        r = torch.where(err == 0, torch.zeros_like(r), r)  # NaN in got propagates: max() is then NaN
        out.append(float(r.max()) if r.numel() else 0.0)
    return tuple(out)


# ------------------------------------------------------------------------------------------------
# fp32 emulation of adam_kernel (torch on the CPU: every fp32 tensor op rounds once), and its mutants
# ------------------------------------------------------------------------------------------------
MUTANTS = ("eps_in_sqrt", "bc2_no_sqrt", "no_bias_correction", "decoupled_wd", "wd_after_moments", "scale_multiplied",
           "betas_swapped_in_v")


def _s(x):
    return torch.tensor(x, dtype=F32)


def _fma(a, b, c):
    """fl32(a * b + c): the product of two fp32 values is exact in double"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def adam_emulate_fp32(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale=None, contract=False, mutant=None):
    """adam_kernel's expression, operation by operation, in fp32 -> (p', m', v').  contract=True fuses each
    product with the sum that follows it, as the compiler may; mutant names one wrong implementation."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, g, m, v = (t.detach().cpu().to(F32) for t in (p, g, m, v))
    lr, beta1, beta2, eps, wd = _s(lr), _s(b1), _s(b2), _s(eps), _s(wd)
    bc1, bc2s = (_s(x) for x in bias_coeffs(b1, b2, step))
    if mutant == "bc2_no_sqrt":
        bc2s = _s(1.0 - f32(b2) ** step)
    if mutant == "no_bias_correction":
        bc1, bc2s = _s(1.0), _s(1.0)
    one = _s(1.0)
    if grad_scale is None:
        gr = g.clone()
    elif mutant == "scale_multiplied":
        gr = g * _s(grad_scale)
    else:
        gr = g * (one / _s(grad_scale))
    decay_in_grad = float(wd) != 0.0 and mutant not in ("decoupled_wd", "wd_after_moments")
    if decay_in_grad:
        gr = _fma(wd, p, gr) if contract else gr + wd * p
    c1, c2 = one - beta1, one - beta2
    d = gr - m
    mv = _fma(c1, d, m) if contract else m + c1 * d
    if mutant == "betas_swapped_in_v":
        vv = _fma(c1 * gr, gr, v * beta1) if contract else v * beta1 + c1 * gr * gr
    else:
        vv = _fma(c2 * gr, gr, v * beta2) if contract else v * beta2 + c2 * gr * gr
    if mutant == "eps_in_sqrt":
        denom = (vv + eps).sqrt() / bc2s
    else:
        denom = vv.sqrt() / bc2s + eps
    q = lr / bc1
    num = mv
    pv = p
    if mutant == "wd_after_moments":
        num = mv + wd * p
    if mutant == "decoupled_wd":
        pv = p - (lr * wd) * p
    r = num / denom
    pn = _fma(-q, r, pv) if contract else pv - q * r
    return pn, mv, vv


# ------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------
CHUNK = 16  # elements per special block; blocks repeat every 8 chunks so every size past 96 holds both kinds


def block_kind(n):
    """per element: 0 ordinary, 1 the zero block (g = m = v = 0), 2 the cancellation block (m within a few
    ulp of gr)"""
    c = (torch.arange(n) // CHUNK) % 8
    return torch.where(c == 3, 1, torch.where(c == 5, 2, 0))


@functools.lru_cache(maxsize=8)
def _inputs(n, seed, wd, grad_scale):
    gen = torch.Generator().manual_seed(seed)

    def spread():
        return torch.randn(n, generator=gen, dtype=F64) * 10.0 ** (torch.rand(n, generator=gen, dtype=F64) * 6 - 4)

    p = spread().to(F32)
    g_true = spread()
    m = spread().to(F32)
    v = (spread() ** 2).to(F32)
    scale = 1.0 if grad_scale is None else f32(grad_scale)
    g = (g_true * scale).to(F32)  # the gradient as a scaled loss leaves it: g / scale spans the six decades
    kind = block_kind(n)
    zero, cancel = kind == 1, kind == 2
    g[zero] = 0.0
    m[zero] = 0.0
    v[zero] = 0.0
    gr = g.to(F64) / scale + f32(wd) * p.to(F64)
    k = torch.randint(-3, 4, (n,), generator=gen).to(F64)
    m[cancel] = (gr * (1.0 + k * 2.0 ** -23)).to(F32)[cancel]
    return p, g, m, v


def make_inputs(n, seed, wd=0.0, grad_scale=None):
    """(p, g, m, v) fp32 CPU tensors: magnitudes randn * 10^uniform(-4, 2) (v its square, so v >= 0), non-zero
    starting moments, a block of exact zeros in g, m and v (the update must be exactly 0 when wd = 0) and a
    block whose m sits within 3 ulp of gr (cancellation in gr - m).  The stored gradient is the true one times
    grad_scale.  Cached: callers must not modify what they get."""
    return _inputs(int(n), int(seed), float(wd), None if grad_scale is None else float(grad_scale))
