"""GPU: per-element contract of the two Adam kernels (csrc/optim.hip) against the float64 reference and the
derived fp32 bounds of tests/adam_ref.py (proved on the CPU by test_adam_ref_cpu.py).

unetseg_adam (host step / lr) and unetseg_adam_dev (device-resident lr and step count, the form a HIP graph
replays) are called through the C ABI on slices of larger allocations -- element offsets 0, 1 and 3, as the
overlapped update's bucket slices are -- with sentinel guards on both sides of each of the four arrays that must
survive bit for bit, as must the gradient.  p', m' and v' are each compared element by element, none excluded.
The sizes straddle one block (255, 256, 257), take several blocks (10007) and reach the grid-stride loop's
second iteration (16384 * 256 + 257: grid_for caps the grid at 16384 blocks, which every real model exceeds).
Each test prints the largest |got - ref| / bound per output; DESIGN.md holds the figures measured on an MI355X.
"""
import itertools

import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = -12345.678
LR, EPS = 1e-3, 1e-8
BIG = 16384 * 256 + 257
SIZES = (0, 1, 255, 256, 257, 10007, BIG)
DEV_SIZES = (1, 257, 10007, BIG)
OFFSETS = (0, 1, 3)
WDS = (0.0, 1e-4)
SCALES = (None, 65536.0, 3.0)
STEPS = (1, 2, 1000, 100000)
B_STD, B_ALT = (0.9, 0.999), (0.5, 0.9)
WORST = {}  # kernel -> [p, m, v] largest |got - ref| / bound seen in this module
BITWISE = {"cases": 0, "p_differ": 0, "elements": 0}  # adam_dev against adam


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()
    yield
    for k, r in sorted(WORST.items()):
        print(f"\nworst ratio  {k:<9s} p {r[0]:.4g}  m {r[1]:.4g}  v {r[2]:.4g}", end="")
    print(f"\nadam_dev vs adam: {BITWISE['cases']} cases, {BITWISE['p_differ']} with a differing p', "
          f"{BITWISE['elements']} differing elements")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32)


class Guarded:
    """a CPU tensor as a slice, `off` elements past the front guard, of a GPU allocation filled with a sentinel"""

    def __init__(self, t, off):
        n = t.numel()
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=t.dtype, device=DEV)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(t)
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def guards_intact(self):
        a, b = _bits(self.buf), _bits(self.before)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:])

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _scale_dev(scale):
    return None if scale is None else Guarded(torch.tensor([scale], dtype=torch.float32), 1)


def _launch(kernel, arrs, n, step, lr, betas, wd, scale):
    """one step of `kernel` ('adam' | 'adam_dev') on the guarded arrays; returns the C status"""
    from unetseg_hip.lib import lib
    P, G, M, V = arrs
    sc = _scale_dev(scale)
    sp = None if sc is None else sc.ptr()
    if kernel == "adam":
        rc = lib.adam(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, lr, betas[0], betas[1], EPS, wd, step, sp, _st())
    else:
        hyper = Guarded(torch.tensor([lr], dtype=torch.float32), 1)
        cnt = Guarded(torch.tensor([step - 1], dtype=torch.int32), 1)
        rc = lib.adam_dev(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, hyper.ptr(), cnt.ptr(), betas[0], betas[1], EPS, wd,
                          sp, _st())
        torch.cuda.synchronize()
        assert hyper.unchanged(), "adam_dev wrote hyper or its surroundings"
        assert cnt.guards_intact() and int(cnt.view.item()) == step, f"*step {int(cnt.view.item())} after step {step}"
    torch.cuda.synchronize()
    assert sc is None or sc.unchanged(), "grad_scale was written"
    return rc


def _run_case(kernel, n, off, step, wd, scale, betas, seed=11, lr=LR):
    inp = A.make_inputs(n, seed, wd, scale)
    arrs = [Guarded(t, off) for t in inp]
    assert _launch(kernel, arrs, n, step, lr, betas, wd, scale) == 0
    P, G, M, V = arrs
    what = f"{kernel} n={n} off={off} step={step} wd={wd} scale={scale} betas={betas}"
    for name, a in zip("pgmv", arrs):
        assert a.guards_intact(), f"{what}: guard of {name} overwritten"
    assert G.unchanged(), f"{what}: the gradient was written"
    got = tuple(a.view.cpu() for a in (P, M, V))
    ref = A.adam_ref(*inp, step, lr, betas[0], betas[1], EPS, wd, scale)
    r = A.ratios(*got, ref)
    print(f"ratio {what}: p {r[0]:.4g} m {r[1]:.4g} v {r[2]:.4g}")
    assert all(x <= 1.0 for x in r), f"{what}: |got - ref| / bound  p {r[0]:.4g}  m {r[1]:.4g}  v {r[2]:.4g}"
    if wd == 0.0:  # zero gradient, zero moments, no decay: the parameter must not move at all
        z = A.block_kind(n) == 1
        assert torch.equal(got[0][z], inp[0][z]), f"{what}: the zero block moved"
    w = WORST.setdefault(kernel, [0.0, 0.0, 0.0])
    for i in range(3):
        w[i] = max(w[i], r[i])
    return got, ref


def _hyper_cases(n, off):
    """(step, wd, scale, betas): the whole wd x grad_scale x step grid plus one (0.5, 0.9) case at the small sizes.
    The large size differs from 10007 only in reaching the grid-stride loop's second iteration, which no
    hyperparameter steers: its six wd x grad_scale combinations are dealt two to an offset, the steps cycled, so
    the three offsets together run every combination once and every step value at least once."""
    combos = list(itertools.product(WDS, SCALES))
    if n < BIG:
        return [(s, wd, sc, B_STD) for (wd, sc), s in itertools.product(combos, STEPS)] + [(2, 1e-4, 3.0, B_ALT)]
    k = 2 * OFFSETS.index(off)
    return [(STEPS[(k + i) % 4], wd, sc, B_STD) for i, (wd, sc) in enumerate(combos[k:k + 2])]


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", [s for s in SIZES if s > 0])
def test_adam_contract(n, off):
    for step, wd, scale, betas in _hyper_cases(n, off):
        _run_case("adam", n, off, step, wd, scale, betas)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", DEV_SIZES)
def test_adam_dev_contract(n, off):
    for step, wd, scale, betas in _hyper_cases(n, off):
        _run_case("adam_dev", n, off, step, wd, scale, betas)


@pytest.mark.parametrize("kernel", ["adam", "adam_dev"])
@pytest.mark.parametrize("off", OFFSETS)
def test_empty_arena_is_a_no_op(kernel, off):
    """n = 0: status 0 and nothing written (the guards meet where the array would be)"""
    e = torch.empty(0, dtype=torch.float32)
    arrs = [Guarded(e, off) for _ in range(4)]
    assert _launch(kernel, arrs, 0, 1, LR, B_STD, 1e-4, 3.0) == 0
    assert all(a.unchanged() for a in arrs)


def test_adam_refuses_step_zero():
    from unetseg_hip.lib import lib
    arrs = [Guarded(t, 1) for t in A.make_inputs(257, 11)]
    P, G, M, V = arrs
    with pytest.raises(RuntimeError, match="step must be >= 1"):
        lib.adam(P.ptr(), G.ptr(), M.ptr(), V.ptr(), 257, LR, 0.9, 0.999, EPS, 0.0, 0, None, _st())
    torch.cuda.synchronize()
    assert all(a.unchanged() for a in arrs)


@pytest.mark.parametrize("kernel", ["adam", "adam_dev"])
def test_refuses_null_and_negative(kernel):
    from unetseg_hip.lib import lib
    arrs = [Guarded(t, 0) for t in A.make_inputs(257, 11)]
    hyper = torch.full((1,), LR, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(ptrs, n):
        if kernel == "adam":
            return lib.adam(*ptrs, n, LR, 0.9, 0.999, EPS, 0.0, 1, None, _st())
        return lib.adam_dev(*ptrs, n, hyper.data_ptr(), cnt.data_ptr(), 0.9, 0.999, EPS, 0.0, None, _st())

    good = [a.ptr() for a in arrs]
    for i in range(4):
        with pytest.raises(RuntimeError, match="null pointer or negative size"):
            call(good[:i] + [None] + good[i + 1:], 257)
    with pytest.raises(RuntimeError, match="null pointer or negative size"):
        call(good, -1)
    torch.cuda.synchronize()
    assert all(a.unchanged() for a in arrs) and int(cnt.item()) == 0


@pytest.mark.parametrize("kernel", ["adam", "adam_dev"])
def test_trajectory_feeds_on_its_own_state(kernel):
    """4 steps on the kernel's own outputs, a fresh gradient each; every step is judged against the reference
    restarted from the kernel's previous state"""
    n, off, wd, scale = 10007, 1, 1e-4, 3.0
    inp = A.make_inputs(n, 21, wd, scale)
    arrs = [Guarded(t, off) for t in inp]
    P, G, M, V = arrs
    state = [t.clone() for t in inp]
    for step in range(1, 5):
        g = A.make_inputs(n, 21 + step, wd, scale)[1]
        G.view.copy_(g)
        g_bits = _bits(G.buf).clone()
        assert _launch(kernel, arrs, n, step, LR, B_STD, wd, scale) == 0
        assert all(a.guards_intact() for a in arrs) and torch.equal(_bits(G.buf), g_bits)
        ref = A.adam_ref(state[0], g, state[2], state[3], step, LR, *B_STD, EPS, wd, scale)
        got = tuple(a.view.cpu() for a in (P, M, V))
        r = A.ratios(*got, ref)
        print(f"ratio {kernel} trajectory step {step}: p {r[0]:.4g} m {r[1]:.4g} v {r[2]:.4g}")
        assert all(x <= 1.0 for x in r), (kernel, step, r)
        state = [got[0], g, got[1], got[2]]


@pytest.mark.parametrize("n,off,step,wd,scale,betas", [
    (1, 0, 1, 0.0, None, B_STD), (257, 1, 2, 1e-4, 65536.0, B_STD), (10007, 3, 1000, 1e-4, 3.0, B_STD),
    (10007, 1, 100000, 0.0, 3.0, B_STD), (10007, 0, 2, 1e-4, None, B_ALT), (BIG, 1, 2, 1e-4, 3.0, B_STD),
    (BIG, 3, 1000, 0.0, None, B_STD),
])
def test_adam_dev_against_adam(n, off, step, wd, scale, betas):
    """equal inputs: m' and v' never read the bias coefficients and are bit-identical; p' may differ by what one
    ulp on each device-computed coefficient allows (adam_ref.dev_vs_host_bound)"""
    a, ref = _run_case("adam", n, off, step, wd, scale, betas)
    b, _ = _run_case("adam_dev", n, off, step, wd, scale, betas)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "m' or v' differ between adam_dev and adam"
    err = (a[0].double() - b[0].double()).abs()
    differ = int((err != 0).sum())
    BITWISE["cases"] += 1
    BITWISE["p_differ"] += differ > 0
    BITWISE["elements"] += differ
    print(f"adam_dev vs adam n={n} step={step}: {differ} of {n} p' differ")
    assert (err <= A.dev_vs_host_bound(ref.p, ref.delta)).all()


def test_graph_replay_advances_step_and_rereads_lr():
    """a captured adam_dev launch pair replayed 5 times: every replay takes the gradient then in the buffer, uses
    *step + 1, advances *step by one and reads the lr then in hyper (changed between replays 2 and 3)"""
    from unetseg_hip.lib import lib
    n, off, wd, start = 10007, 1, 1e-4, 7
    inp = A.make_inputs(n, 31, wd)
    # one eager call on scratch buffers first, so nothing is loaded during the capture
    assert _launch("adam_dev", [Guarded(t, off) for t in inp], n, 1, LR, B_STD, wd, None) == 0
    arrs = [Guarded(t, off) for t in inp]
    P, G, M, V = arrs
    hyper = Guarded(torch.tensor([LR], dtype=torch.float32), 1)
    cnt = Guarded(torch.tensor([start], dtype=torch.int32), 1)

    def launch():
        lib.adam_dev(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, hyper.ptr(), cnt.ptr(), B_STD[0], B_STD[1], EPS, wd, None,
                     _st())

    # torch's side-stream warm-up on buffers of its own, as bench.py runs its warm-up steps
    warm = [Guarded(t, off) for t in inp]
    wcnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            lib.adam_dev(*(a.ptr() for a in warm), n, hyper.ptr(), wcnt.data_ptr(), B_STD[0], B_STD[1], EPS, wd, None,
                         _st())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    assert all(a.unchanged() for a in arrs), "the capture itself ran the update"
    assert cnt.unchanged() and hyper.unchanged(), "the capture itself advanced *step"
    state = [t.clone() for t in inp]
    lr = LR
    for k in range(1, 6):
        if k == 3:
            lr = 2.5e-4
            hyper.view.fill_(lr)
        g = A.make_inputs(n, 31 + k, wd)[1]
        G.view.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert int(cnt.view.item()) == start + k and cnt.guards_intact()
        assert all(a.guards_intact() for a in arrs) and torch.equal(G.view.cpu(), g)
        got = tuple(a.view.cpu() for a in (P, M, V))
        ref = A.adam_ref(state[0], g, state[2], state[3], start + k, lr, *B_STD, EPS, wd)
        r = A.ratios(*got, ref)
        print(f"ratio graph replay {k} (step {start + k}, lr {lr}): p {r[0]:.4g} m {r[1]:.4g} v {r[2]:.4g}")
        assert all(x <= 1.0 for x in r), (k, r)
        if k == 3:  # the old lr must be outside the bound: the change took effect at exactly this replay
            old = A.adam_ref(state[0], g, state[2], state[3], start + k, LR, *B_STD, EPS, wd)
            assert A.ratios(*got, old)[0] > 1.0
        state = [got[0], g, got[1], got[2]]
    assert torch.equal(_bits(hyper.view.cpu()), _bits(torch.tensor([2.5e-4], dtype=torch.float32)))
