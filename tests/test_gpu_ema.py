"""GPU: the weight EMA fused into the Adam kernels (csrc/optim.hip), from the C ABI up to train.py.

unetseg_adam_ema and unetseg_adam_ema_dev run on guarded slices (element offsets 0, 1 and 3, and one case with a
different offset per array, which takes the kernels' scalar path): the average is held to the bound of
tests/ema_ref.py (proved on the CPU by test_ema_ref_cpu.py) and p', m', v' must equal, bit for bit, what
unetseg_adam / unetseg_adam_dev give on copies of the same inputs.  unetseg_swap_f32 must exchange exactly.  The
capturable form is replayed from a HIP graph with warm-up on, so the device step count has to drive d_t.  FusedAdam
with ema_decay is run through its four update paths (whole arena, per bucket, capturable, a replayed step plan);
averaged(), the state_dict round trip and train.py --ema-decay follow.  The sizes are those of
test_gpu_adam_contract.py: 16384 * 256 + 257 is the first at which the stride loops wrap, for the 16-byte body
(4096 blocks of 256 threads, four elements each) as for the scalar path (16384 blocks).
"""
import contextlib
import copy
import io
import itertools
import os

import pytest
import torch

import adam_ref as A
import ema_ref as E
from test_gpu_adam_contract import BIG, DEV, EPS, LR, Guarded, _bits, _scale_dev, _st

pytestmark = pytest.mark.gpu
B1, B2 = 0.9, 0.999
SIZES = (1, 255, 256, 257, 10007, BIG)
OFFSETS = (0, 1, 3)
KERNELS = ("adam_ema", "adam_ema_dev")
# (step, wd, grad_scale, decay, warmup): the whole grid of the contract
GRID = list(itertools.product((1, 1000), (0.0, 1e-4), (None, 65536.0), (0.9, 0.999), (True, False)))
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()
    yield
    for k, r in sorted(WORST.items()):
        print(f"\nworst |ema - ref| / bound  {k:<13s} {r:.4g}", end="")


def _arrays(n, offs, wd, scale, seed=11):
    inp = A.make_inputs(n, seed, wd, scale) + (E.make_ema(n, seed, wd, scale),)
    return inp, [Guarded(t, o) for t, o in zip(inp, offs)]


def _launch(kernel, arrs, n, step, wd, scale, decay=0.999, warmup=True, lr=LR):
    """one step of `kernel` on the guarded arrays (four for adam / adam_dev, five for the EMA forms)"""
    from unetseg_hip.lib import lib
    ptrs = [a.ptr() for a in arrs]
    sc = _scale_dev(scale)
    sp = None if sc is None else sc.ptr()
    if kernel == "adam":
        rc = lib.adam(*ptrs, n, lr, B1, B2, EPS, wd, step, sp, _st())
    elif kernel == "adam_ema":
        rc = lib.adam_ema(*ptrs, n, lr, B1, B2, EPS, wd, step, E.one_minus_decay(decay, warmup, step), sp, _st())
    else:
        hyper = Guarded(torch.tensor([lr], dtype=torch.float32), 1)
        cnt = Guarded(torch.tensor([step - 1], dtype=torch.int32), 1)
        if kernel == "adam_dev":
            rc = lib.adam_dev(*ptrs, n, hyper.ptr(), cnt.ptr(), B1, B2, EPS, wd, sp, _st())
        else:
            rc = lib.adam_ema_dev(*ptrs, n, hyper.ptr(), cnt.ptr(), B1, B2, EPS, wd, decay, int(warmup), sp, _st())
        torch.cuda.synchronize()
        assert hyper.unchanged(), f"{kernel} wrote hyper or its surroundings"
        want = step if n > 0 or kernel == "adam_dev" else step - 1
        assert cnt.guards_intact() and int(cnt.view.item()) == want, f"*step {int(cnt.view.item())}, expected {want}"
    torch.cuda.synchronize()
    assert sc is None or sc.unchanged(), "grad_scale was written"
    return rc


def _run_case(kernel, n, offs, step, wd, scale, decay, warmup):
    what = f"{kernel} n={n} offs={offs} step={step} wd={wd} scale={scale} decay={decay} warmup={warmup}"
    inp, arrs = _arrays(n, offs, wd, scale)
    assert _launch(kernel, arrs, n, step, wd, scale, decay, warmup) == 0
    base = [Guarded(t, o) for t, o in zip(inp[:4], offs)]
    assert _launch(kernel.replace("_ema", ""), base, n, step, wd, scale) == 0
    for name, a in zip("pgmve", arrs):
        assert a.guards_intact(), f"{what}: guard of {name} overwritten"
    assert arrs[1].unchanged(), f"{what}: the gradient was written"
    for name, i in (("p", 0), ("m", 2), ("v", 3)):
        assert torch.equal(_bits(arrs[i].view), _bits(base[i].view)), f"{what}: {name}' differs from the kernel without EMA"
    ref = E.ema_ref(*inp, step, LR, B1, B2, EPS, wd, E.one_minus_decay(decay, warmup, step), scale)
    r = E.ratio(arrs[4].view.cpu(), ref.ema, E.ema_bound(ref))
    print(f"ratio {what}: ema {r:.4g}")
    assert r <= 1.0, f"{what}: |ema - ref| / bound {r:.4g}"
    if wd == 0.0:  # zero gradient and moments, no decay, average equal to the parameter: nothing moves
        z = A.block_kind(n) == 1
        assert torch.equal(arrs[4].view.cpu()[z], inp[4][z]), f"{what}: the average of the zero block moved"
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)


def _cases(n, off):
    """the whole grid at 10007 elements and offset 1; elsewhere a slice of it that moves with the size and the offset,
    so every value of every factor is met at every size; the large size (which differs only in wrapping the stride
    loop) takes one case per offset"""
    if n == 10007 and off == 1:
        return GRID
    k = 5 * SIZES.index(n) + 11 * OFFSETS.index(off)
    if n == BIG:
        return [GRID[(7 * k + 3) % 32]]
    return [GRID[(k + 9 * i) % 32] for i in range(4)] + [GRID[31 - (k + 9 * i) % 32] for i in range(4)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_fused_kernel_contract(n, off, kernel):
    for step, wd, scale, decay, warmup in _cases(n, off):
        _run_case(kernel, n, (off,) * 5, step, wd, scale, decay, warmup)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", (257, 10007))
def test_fused_kernel_with_unequal_offsets(n, kernel):
    """the five arrays at different distances from a 16-byte boundary: no vector body"""
    _run_case(kernel, n, (0, 1, 2, 3, 1), 1000, 1e-4, 65536.0, 0.999, True)
    _run_case(kernel, n, (3, 3, 3, 3, 0), 1, 0.0, None, 0.9, False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("off", OFFSETS)
def test_empty_slice_is_a_no_op(kernel, off):
    e = torch.empty(0, dtype=torch.float32)
    arrs = [Guarded(e, off) for _ in range(5)]
    assert _launch(kernel, arrs, 0, 1, 1e-4, 65536.0) == 0  # (_launch also holds *step where it was)
    assert all(a.unchanged() for a in arrs)


@pytest.mark.parametrize("kernel", KERNELS)
def test_fused_kernel_refuses_bad_arguments(kernel):
    from unetseg_hip.lib import lib
    inp, arrs = _arrays(257, (0,) * 5, 0.0, None)
    hyper = torch.full((1,), LR, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(ptrs, n, step=1, omd=0.001, decay=0.999, hp=hyper.data_ptr(), cp=cnt.data_ptr()):
        if kernel == "adam_ema":
            return lib.adam_ema(*ptrs, n, LR, B1, B2, EPS, 0.0, step, omd, None, _st())
        return lib.adam_ema_dev(*ptrs, n, hp, cp, B1, B2, EPS, 0.0, decay, 1, None, _st())

    good = [a.ptr() for a in arrs]
    for i in range(5):
        with pytest.raises(RuntimeError, match="null pointer or negative size"):
            call(good[:i] + [None] + good[i + 1:], 257)
    with pytest.raises(RuntimeError, match="null pointer or negative size"):
        call(good, -1)
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        call(good[:4] + [good[4] + 2], 16)
    if kernel == "adam_ema":
        with pytest.raises(RuntimeError, match="step must be >= 1"):
            call(good, 257, step=0)
        for bad in (-0.001, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match="one_minus_decay"):
                call(good, 257, omd=bad)
    else:
        for bad in (-0.001, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match="decay"):
                call(good, 257, decay=bad)
        with pytest.raises(RuntimeError, match="device pointers"):
            call(good, 257, hp=None)
        with pytest.raises(RuntimeError, match="device pointers"):
            call(good, 257, cp=None)
    torch.cuda.synchronize()
    assert all(a.unchanged() for a in arrs) and int(cnt.item()) == 0


# ------------------------------------------------------------------------------------------------
# unetseg_swap_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (3, 3), (1, 2)])
@pytest.mark.parametrize("n", (0,) + SIZES)
def test_swap_is_exact_and_its_own_inverse(n, offs):
    from unetseg_hip.lib import lib
    gen = torch.Generator().manual_seed(n % 1000 + 5)
    # every bit pattern counts: NaNs, infinities and denormals travel as they are
    ta, tb = (torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
              .view(torch.float32) for _ in range(2))
    a, b = Guarded(ta, offs[0]), Guarded(tb, offs[1])
    lib.swap_f32(a.ptr(), b.ptr(), n, _st())
    torch.cuda.synchronize()
    assert a.guards_intact() and b.guards_intact()
    assert torch.equal(_bits(a.view.cpu()), _bits(tb)) and torch.equal(_bits(b.view.cpu()), _bits(ta))
    lib.swap_f32(a.ptr(), b.ptr(), n, _st())
    torch.cuda.synchronize()
    assert a.unchanged() and b.unchanged()


def test_swap_refuses_bad_arguments():
    from unetseg_hip.lib import lib
    a, b = (Guarded(torch.ones(16), 0) for _ in range(2))
    for args in ((None, b.ptr(), 16), (a.ptr(), None, 16), (a.ptr(), b.ptr(), -1)):
        with pytest.raises(RuntimeError, match="null pointer or negative size"):
            lib.swap_f32(*args, _st())
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        lib.swap_f32(a.ptr() + 1, b.ptr(), 8, _st())
    torch.cuda.synchronize()
    assert a.unchanged() and b.unchanged()


# ------------------------------------------------------------------------------------------------
# the capturable form under a HIP graph
# ------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_device_step_for_the_warmup():
    """one captured unetseg_adam_ema_dev step replayed 12 times from *step = 0, warm-up on: replay k must use
    d_t = (1 + k) / (10 + k), 2/11 ... 13/22, on the parameter it has just written.  The average is recomputed on
    the host from the parameter snapshots, so only the EMA line's own roundings (and one ulp on the device's
    1 - d_t) separate the two; the neighbouring step's d_t is outside that bound."""
    from unetseg_hip.lib import lib
    n, off, wd, decay = 10007, 1, 1e-4, 0.999
    inp, arrs = _arrays(n, (off,) * 5, wd, None, seed=31)
    # one eager call on scratch buffers first, so nothing is loaded during the capture
    assert _launch("adam_ema_dev", _arrays(n, (off,) * 5, wd, None, seed=31)[1], n, 1, wd, None) == 0
    hyper = Guarded(torch.tensor([LR], dtype=torch.float32), 1)
    cnt = Guarded(torch.tensor([0], dtype=torch.int32), 1)

    def launch(to, c):
        lib.adam_ema_dev(*(a.ptr() for a in to), n, hyper.ptr(), c, B1, B2, EPS, wd, decay, 1, None, _st())

    warm = _arrays(n, (off,) * 5, wd, None, seed=31)[1]
    wcnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            launch(warm, wcnt.data_ptr())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(arrs, cnt.ptr())
    torch.cuda.synchronize()
    assert all(a.unchanged() for a in arrs) and cnt.unchanged(), "the capture itself ran the update"
    e_prev = inp[4]
    for k in range(1, 13):
        arrs[1].view.copy_(A.make_inputs(n, 31 + k, wd)[1])
        graph.replay()
        torch.cuda.synchronize()
        assert int(cnt.view.item()) == k and cnt.guards_intact() and all(a.guards_intact() for a in arrs)
        p_k, e_k = arrs[0].view.cpu(), arrs[4].view.cpu()
        bound = E.own_bound(e_prev, p_k)
        r = E.ratio(e_k, E.ema_update_ref(e_prev, p_k, E.one_minus_decay(decay, True, k)), bound)
        print(f"graph replay {k}: d_t = {1 + k}/{10 + k}, |ema - ref| / bound {r:.4g}")
        assert E.decay_at(decay, True, k) == (1.0 + k) / (10.0 + k)
        assert r <= 1.0, (k, r)
        for other in (k - 1, k + 1):  # a stale or early step count, or the decay without warm-up, shows
            assert E.ratio(e_k, E.ema_update_ref(e_prev, p_k, E.one_minus_decay(decay, True, max(other, 0))), bound) > 1.0
        assert E.ratio(e_k, E.ema_update_ref(e_prev, p_k, E.one_minus_decay(decay, False, k)), bound) > 1.0
        e_prev = e_k


# ------------------------------------------------------------------------------------------------
# FusedAdam(ema_decay=...)
# ------------------------------------------------------------------------------------------------
DECAY = 0.99
NSTEPS = 4


def _build(mode, ema_decay=DECAY, warmup=True, seed=0):
    from model.model_factory import build_model
    from unetseg_hip.arena import FusedAdam

    torch.manual_seed(seed)
    m = build_model("unet_plain", num_classes=2).to(DEV).train()
    m.compute_dtype = "fp32"
    opt = FusedAdam(m, lr=1e-3, betas=(B1, B2), weight_decay=1e-4, capturable=mode == "capturable",
                    overlap=mode == "overlap", bucket_mb=2.0, ema_decay=ema_decay, ema_warmup=warmup)
    return m, opt


def _batch(it):
    from utils.synthetic import make_batch
    x, y = make_batch(2, 64, seed=40 + it)
    return x.to(DEV), y.to(DEV)


def _train_step(m, opt, x, y):
    from unetseg_hip import losses
    opt.zero_grad()
    loss = losses.binary_segmentation_loss(m(x), y, "lovasz_hinge")
    loss.backward()
    opt.step()
    return loss


def _snap(m, opt):
    torch.cuda.synchronize()
    return tuple(t.clone() for t in (m._flat, opt._m, opt._v) + ((opt._ema,) if opt._ema is not None else ()))


def _run(mode, ema_decay, nsteps=NSTEPS):
    """snapshots (p, m, v[, ema]) after each of nsteps training steps, preceded by the initial arena; mode 'plan'
    records its first step into a StepPlan and replays the rest"""
    from unetseg_hip.plan import StepPlan
    m, opt = _build("eager" if mode == "plan" else mode, ema_decay)
    p0 = m._flat.clone()
    snaps = []
    if mode == "plan":
        rec = _batch(0)
        plan = StepPlan({"x": rec[0], "y": rec[1]})
        plan.record(lambda: _train_step(m, opt, *rec))
        snaps.append(_snap(m, opt))
        for it in range(1, nsteps):
            x, y = _batch(it)
            plan.replay(x=x, y=y)
            snaps.append(_snap(m, opt))
    else:
        for it in range(nsteps):
            _train_step(m, opt, *_batch(it))
            snaps.append(_snap(m, opt))
    assert opt.state_dict()["flat_state"]["step"] == nsteps
    return p0, snaps


@pytest.fixture(scope="module")
def on_side_stream():
    """a step plan replays on the stream it was recorded on: every optimizer-level run uses one stream of its own"""
    stream = torch.cuda.Stream(DEV)
    prev = torch.cuda.current_stream(DEV)
    torch.cuda.set_stream(stream)
    yield
    torch.cuda.synchronize()
    torch.cuda.set_stream(prev)


@pytest.fixture(scope="module")
def eager_run(on_side_stream):
    return _run("eager", DECAY)


@pytest.mark.parametrize("mode", ["eager", "overlap", "capturable", "plan"])
def test_optimizer_paths_keep_the_average(mode, eager_run, on_side_stream):
    """four steps (the plan: one recorded, three replayed): after every step the average is the float64 EMA of
    that run's own parameter snapshots within the EMA line's own roundings, starting from a copy of the initial
    arena; p, m, v are bit-identical to the same run without EMA; the plan run is the eager run, average included"""
    p0, snaps = eager_run if mode == "eager" else _run(mode, DECAY)
    _, plain = _run(mode, 0.0)
    e_prev = p0
    for t, (s, q) in enumerate(zip(snaps, plain), 1):
        assert len(s) == 4 and len(q) == 3
        for name, a, b in zip(("p", "m", "v"), s, q):
            assert torch.equal(_bits(a), _bits(b)), f"{mode} step {t}: {name} differs from the run without EMA"
        omd = E.one_minus_decay(DECAY, True, t)
        r = E.ratio(s[3], E.ema_update_ref(e_prev, s[0], omd), E.own_bound(e_prev, s[0]))
        print(f"{mode} step {t}: 1 - d_t {omd:.6f}  |ema - ref| / bound {r:.4g}")
        assert r <= 1.0, (mode, t, r)
        e_prev = s[3]
    if mode == "plan":
        for t, (s, q) in enumerate(zip(snaps, eager_run[1]), 1):
            for name, a, b in zip(("p", "m", "v", "ema"), s, q):
                assert torch.equal(_bits(a), _bits(b)), f"step {t}: {name} of the plan run differs from the eager run"


def test_averaged_context(on_side_stream):
    from model.model_factory import build_model
    m, opt = _build("eager")
    twin_m, twin_opt = _build("eager")
    for it in range(2):
        _train_step(m, opt, *_batch(it))
        _train_step(twin_m, twin_opt, *_batch(it))
    before = _snap(m, opt)
    assert not torch.equal(before[0], before[3])
    # a model loaded with the average (and the live buffers)
    other = build_model("unet_plain", num_classes=2).to(DEV)
    other.compute_dtype = "fp32"
    other.load_state_dict(copy.deepcopy(m.state_dict()))
    other._flat.copy_(before[3])
    other._prepacked = None
    x, _ = _batch(7)
    m.eval(), other.eval()
    with torch.no_grad():
        want = other(x).clone()
        live = m(x).clone()
        with opt.averaged():
            assert torch.equal(_bits(m._flat), _bits(before[3])) and torch.equal(_bits(opt._ema), _bits(before[0]))
            got = m(x).clone()
            with pytest.raises(RuntimeError, match="averaged weights"):
                opt._plain_step(None)
        again = m(x).clone()
    assert torch.equal(got, want) and not torch.equal(got, live) and torch.equal(again, live)
    with pytest.raises(ZeroDivisionError):  # the live weights come back when the block raises
        with opt.averaged():
            1 / 0
    after = _snap(m, opt)
    for name, a, b in zip(("p", "m", "v", "ema"), before, after):
        assert torch.equal(_bits(a), _bits(b)), f"{name} changed across averaged()"
    m.train()
    _train_step(m, opt, *_batch(2))
    _train_step(twin_m, twin_opt, *_batch(2))
    for name, a, b in zip(("p", "m", "v", "ema"), _snap(m, opt), _snap(twin_m, twin_opt)):
        assert torch.equal(_bits(a), _bits(b)), f"{name} after the next step differs from the run that never swapped"


def test_swap_is_refused(on_side_stream, monkeypatch):
    from unetseg_hip import losses
    from unetseg_hip.plan import StepPlan
    m, opt = _build("eager", 0.0)
    _train_step(m, opt, *_batch(0))
    with pytest.raises(RuntimeError, match="EMA is off"):
        opt.swap_ema()
    with pytest.raises(RuntimeError, match="EMA is off"):
        with opt.averaged():
            pass
    assert opt._ema is None and "ema" not in opt.state_dict()["flat_state"]
    m, opt = _build("overlap")
    x, y = _batch(0)
    _train_step(m, opt, x, y)
    before = _snap(m, opt)
    with pytest.raises(RuntimeError, match="recording"):
        StepPlan({"x": x}).record(opt.swap_ema)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capturing"):
        opt.swap_ema()
    monkeypatch.undo()
    opt.zero_grad()
    losses.binary_segmentation_loss(m(x), y, "lovasz_hinge").backward()
    mid = _snap(m, opt)
    with pytest.raises(RuntimeError, match="overlapped backward"):
        opt.swap_ema()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(mid, _snap(m, opt)))
    opt.step()
    assert not torch.equal(before[3], mid[3])  # (the overlapped update had run in that backward)
    with opt.averaged():
        pass
    with pytest.raises(ValueError, match="ema_decay"):
        _build("eager", 1.0)


def test_state_dict_round_trip(on_side_stream):
    m, opt = _build("eager")
    for it in range(2):
        _train_step(m, opt, *_batch(it))
    f = io.BytesIO()
    torch.save(opt.state_dict(), f)
    f.seek(0)
    sd = torch.load(f, map_location="cpu")
    assert torch.equal(sd["flat_state"]["ema"], opt._ema.cpu())
    msd = copy.deepcopy(m.state_dict())
    m2, opt2 = _build("eager", seed=1)
    m2.load_state_dict(msd)
    pristine = copy.deepcopy(sd)
    opt2.load_state_dict(sd)
    assert torch.equal(sd["flat_state"]["ema"], pristine["flat_state"]["ema"])
    assert opt2._ema.device == m2._flat.device and opt2._ema.data_ptr() != opt._ema.data_ptr()
    assert torch.equal(_bits(opt2._ema), _bits(opt._ema))
    _train_step(m, opt, *_batch(2))
    _train_step(m2, opt2, *_batch(2))
    for name, a, b in zip(("p", "m", "v", "ema"), _snap(m, opt), _snap(m2, opt2)):
        assert torch.equal(_bits(a), _bits(b)), f"{name} of the resumed run differs"
    # a checkpoint from before the feature: loads, and the average starts from the weights then in the arena
    old = copy.deepcopy(pristine)
    del old["flat_state"]["ema"]
    m3, opt3 = _build("eager", seed=1)
    m3.load_state_dict(msd)
    opt3.load_state_dict(old)
    assert opt3._ema is None and opt3._step == 2
    p_before = m3._flat.clone()
    _train_step(m3, opt3, *_batch(2))
    s = _snap(m3, opt3)
    omd = E.one_minus_decay(DECAY, True, 3)
    assert E.ratio(s[3], E.ema_update_ref(p_before, s[0], omd), E.own_bound(p_before, s[0])) <= 1.0
    # a wrong shape is refused before anything changes
    before = _snap(m2, opt2)
    bad = copy.deepcopy(pristine)
    bad["flat_state"]["ema"] = bad["flat_state"]["ema"][:-1].clone()
    bad["flat_state"]["step"] = 77
    with pytest.raises(ValueError, match="ema has shape"):
        opt2.load_state_dict(bad)
    assert opt2._step == 3 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, _snap(m2, opt2)))


def test_train_entry_point_saves_averaged_and_live_weights(tmp_path):
    import json

    import train
    from model.model_factory import build_model

    args = train.parse_args(["--task", "binary", "--model", "unet_plain", "--input-size", "64", "--batch-size", "2",
                             "--epochs", "2", "--max-train-batches", "2", "--max-val-batches", "1", "--synthetic-train",
                             "4", "--synthetic-val", "2", "--workers", "0", "--ema-decay", "0.99", "--out-dir",
                             str(tmp_path)])
    with contextlib.redirect_stdout(io.StringIO()):
        exp = train.train(args)
    cfg = json.load(open(os.path.join(exp, "config.json")))
    assert cfg["ema_decay"] == 0.99 and cfg["no_ema_warmup"] is False
    sds = {}
    for name in ("best", "last", "last_raw"):
        path = os.path.join(exp, "weights", name + ".pth")
        assert os.path.exists(path), name
        sds[name] = torch.load(path, map_location="cpu", weights_only=True)
        build_model("unet_plain", num_classes=2).load_state_dict(sds[name], strict=True)  # the reference's keys
    params = [k for k, _ in build_model("unet_plain", num_classes=2).named_parameters()]
    for name in ("best", "last"):
        assert any(not torch.equal(sds[name][k], sds["last_raw"][k]) for k in params), f"{name}.pth holds the live weights"
    # buffers are not averaged: last.pth and last_raw.pth, written after the same epoch, share them
    bufs = [k for k in sds["last"] if k not in params]
    assert bufs and all(torch.equal(sds["last"][k], sds["last_raw"][k]) for k in bufs)
