"""Inputs of the soft-skeleton / soft-clDice comparisons, shared by tests/test_cldice_cpu.py (which asserts the
conditions under which a comparison means something, on the CPU) and tests/test_gpu_cldice.py (which runs them).

Skeleton cases feed fp32 probability maps sigmoid(z), z uniform in [-2, 2], straight to the kernels, so min / max
selection happens on identical values (a wider z leaves s_j within rounding of 1 somewhere at seven levels on
every seed, and the relu of d_j (1 - s_{j-1}) is then undecided).  Shapes: single pixels and lines, 2x5x9,
3x13x66 (three column tiles, the last one 2 wide), and the 32 x 32 tile plus 1 and plus 3 in both dimensions (the second: a remainder as wide as the
forward's halo).  iters 0, 1, 3, 7, and 12 > min(H, W) on 2x5x9 (every shape below 8 has iters above its size too).

Loss cases draw z uniform in [-4, 4] (nch 2: o0 = 2 randn, o1 = o0 + z in fp32, so |fl32(o1 - o0)| <= 6) and targets
from a few strokes one to three pixels wide; with `ignore` a tenth of the pixels is ignored.

The seeds were picked on the CPU so that the conditions of test_cldice_cpu.py hold; SEED_SHIFT lists the cases
whose first seed did not.
"""
import functools

import numpy as np

import cldice_ref as R

IGN = 255
TILE = 32
SKEL_SHAPES = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 5, 9), (3, 13, 66), (1, TILE + 1, TILE + 1), (1, TILE + 3, TILE + 3)]
SKEL_CASES = [(s, k) for s in SKEL_SHAPES for k in (0, 1, 3, 7)] + [((2, 5, 9), 12)]

LOSS_SHAPES = [(1, 1, 1), (2, 5, 9), (3, 13, 66), (2, TILE + 3, TILE + 1)]
# (shape, nch, ignore, iters, kind); kind: "mixed", or the whole batch "ignored" / "background" / "foreground"
LOSS_CASES = ([(s, nch, ign, 3, "mixed") for s in LOSS_SHAPES for nch in (1, 2) for ign in (False, True)]
              + [((2, 5, 9), 2, False, 1, "mixed"), ((3, 13, 66), 1, True, 0, "mixed")]
              + [((2, 13, 21), 2, True, 3, "ignored"), ((2, 13, 21), 2, False, 3, "background"),
                 ((2, 13, 21), 1, False, 3, "foreground"), ((2, 13, 21), 1, True, 3, "foreground")])

#: case -> added to its seed (found with `python tests/cldice_cases.py`)
SEED_SHIFT = {
    ("skel", (3, 13, 66), 7): 1,
    ("loss", (3, 13, 66), 1, False, 3, "mixed"): 1,
    ("loss", (2, 35, 33), 1, False, 3, "mixed"): 1,
}


def conditions_hold(levels, x, margin=0.0):
    """no relu argument of the float64 reference in (0, 2^-18), pairwise distinct non-zero inputs per image, and
    every window's extreme apart from the window's next value by more than `margin`, relatively"""
    a = R.relu_arguments(levels)
    if ((a > 0) & (a < 2.0 ** -18)).any():
        return False
    if not all(np.unique(img[img != 0]).size == (img != 0).sum() for img in x):
        return False
    return R.selection_margin(levels) > margin


def _skel_inputs(shape, iters, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-2.0, 2.0, shape)
    x = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    return x, g


def _skel_seed(shape, iters):
    N, H, W = shape
    return 100000 * N + 1000 * H + 10 * W + 7 * iters + SEED_SHIFT.get(("skel", shape, iters), 0)


@functools.lru_cache(maxsize=None)
def skel_case(shape, iters):
    """inputs and float64 reference of one skeleton case, computed once and shared read-only"""
    x, g = _skel_inputs(shape, iters, _skel_seed(shape, iters))
    levels = R.skeleton_levels(x, iters)
    gx, A = R.skeleton_backward(levels, g)
    for a in (x, g, gx, A):
        a.setflags(write=False)
    return dict(shape=shape, iters=iters, x=x, g=g, levels=levels, skel=levels[-1]["s"], gx=gx, A=A)


def _targets(rng, shape, ignore, kind):
    B, H, W = shape
    t = np.zeros(shape, dtype=np.int64)
    if kind == "foreground":
        t[:] = 1
    elif kind == "mixed":
        for b in range(B):
            for _ in range(3):  # strokes: rows and columns one to three pixels wide
                w = int(rng.integers(1, 4))
                if rng.random() < 0.5:
                    r = int(rng.integers(0, H))
                    t[b, r:r + w, int(rng.integers(0, W)):] = 1
                else:
                    c = int(rng.integers(0, W))
                    t[b, :int(rng.integers(1, H + 1)), c:c + w] = 1
    if kind == "ignored":
        t[:] = IGN
    elif ignore:
        t[rng.random(shape) < 0.1] = IGN
    return t


def _loss_inputs(shape, nch, ignore, kind, seed):
    rng = np.random.default_rng(seed)
    B, H, W = shape
    z = rng.uniform(-4.0, 4.0, shape).astype(np.float32)
    if nch == 2:
        o0 = (2 * rng.standard_normal(shape)).astype(np.float32)
        out = np.stack([o0, o0 + z], 1)
    else:
        out = z[:, None]
    return np.ascontiguousarray(out, dtype=np.float32), _targets(rng, shape, ignore, kind)


def _loss_seed(shape, nch, ignore, iters, kind):
    B, H, W = shape
    return (100000 * B + 1000 * H + 10 * W + nch + (5 if ignore else 0) + 7 * iters + len(kind)
            + SEED_SHIFT.get(("loss", shape, nch, ignore, iters, kind), 0))


#: the relative gap a window's extreme keeps from the next value: the fp32 p is within EPS_P u of the reference's
LOSS_MARGIN = 4 * R.EPS_P * R.U


@functools.lru_cache(maxsize=None)
def loss_case(shape, nch, ignore, iters, kind):
    out, t = _loss_inputs(shape, nch, ignore, kind, _loss_seed(shape, nch, ignore, iters, kind))
    ref = R.cldice(out, t, iters=iters, smooth=1.0, ignore=IGN if ignore else None)
    for a in (out, t, ref["gz"], ref["gz_bound"]):
        a.setflags(write=False)
    return dict(shape=shape, nch=nch, ign=IGN if ignore else None, iters=iters, kind=kind, out=out, t=t, **ref)


if __name__ == "__main__":  # prints the SEED_SHIFT entries the conditions need
    for shape, k in SKEL_CASES:
        for shift in range(200):
            SEED_SHIFT[("skel", shape, k)] = shift
            x, _ = _skel_inputs(shape, k, _skel_seed(shape, k))
            if conditions_hold(R.skeleton_levels(x, k), x):
                break
        if shift:
            print(f'    ("skel", {shape}, {k}): {shift},')
    for c in LOSS_CASES:
        shape, nch, ignore, k, kind = c
        for shift in range(200):
            SEED_SHIFT[("loss",) + c] = shift
            out, t = _loss_inputs(shape, nch, ignore, kind, _loss_seed(*c))
            ref = R.cldice(out, t, iters=k, ignore=IGN if ignore else None)
            if conditions_hold(ref["levels"], ref["p"], LOSS_MARGIN):
                break
        if shift:
            print(f'    ("loss", {shape}, {nch}, {ignore}, {k}, "{kind}"): {shift},')
