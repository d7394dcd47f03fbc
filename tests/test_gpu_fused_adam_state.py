"""GPU: FusedAdam as an object -- the capturable form against the plain one over several eager steps with an lr
change, and state_dict / load_state_dict: a run resumed from a checkpoint (handed over directly, through
torch.save / torch.load(map_location="cpu"), or loaded twice from the same dict) continues bit for bit as the
uninterrupted run does, for the plain, the capturable and the overlapped update."""
import copy
import io

import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("plain", "capturable", "overlap")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _build(mode):
    from model.model_factory import build_model
    from unetseg_hip.arena import FusedAdam

    torch.manual_seed(0)
    m = build_model("unet_plain", num_classes=2).to(DEV).train()
    m.compute_dtype = "fp32"
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-4, capturable=mode == "capturable",
                    overlap=mode == "overlap", bucket_mb=2.0)
    return m, opt


def _steps(m, opt, its, trace=None):
    """training steps `its` (the batch and the lr follow the step index, so a resumed run sees what the
    uninterrupted one saw); trace collects (p, m, v) before each update and the gradient it used"""
    from unetseg_hip import losses
    from utils.synthetic import make_batch

    for it in its:
        x, y = make_batch(2, 64, seed=40 + it)
        if it == 2:
            opt.param_groups[0]["lr"] = 3e-4  # before backward: the overlapped update reads it there
        opt.zero_grad()
        losses.binary_segmentation_loss(m(x.to(DEV)), y.to(DEV), "lovasz_hinge").backward()
        if trace is not None:
            torch.cuda.synchronize()
            before = (m._flat.clone(), None if opt._m is None else opt._m.clone(),
                      None if opt._v is None else opt._v.clone())
        opt.step()
        if trace is not None:
            trace.append((before, m._flat_grad.clone(), _snap(m, opt)))
    return _snap(m, opt)


def _snap(m, opt):
    torch.cuda.synchronize()
    return m._flat.clone(), opt._m.clone(), opt._v.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_capturable_matches_plain_eager():
    """4 eager steps, lr changed before the third.  Induction over the steps: while the two runs hold the same
    state they see the same gradient, so m' and v' (which never read the bias coefficients) stay bit-identical
    and p' stays within what one ulp on each device-computed coefficient allows (adam_ref.dev_vs_host_bound, the
    bound test_gpu_adam_contract.py holds the two kernels to); the bounds of the 4 steps add up.  A capturable
    form that kept a stale lr or step count would leave that bound by orders of magnitude."""
    runs = {}
    for mode in ("plain", "capturable"):
        m, opt = _build(mode)
        trace = []
        _steps(m, opt, range(4), trace)
        assert opt.state_dict()["flat_state"]["step"] == 4, mode
        runs[mode] = trace
    identical = True
    budget = torch.zeros_like(runs["plain"][0][2][0], dtype=torch.float64)
    for t, (a, b) in enumerate(zip(runs["plain"], runs["capturable"]), 1):
        (pa0, _, _), ga, (pa, ma, va) = a
        (_, _, _), gb, (pb, mb, vb) = b
        if identical:
            assert torch.equal(ga, gb), f"step {t}: equal states gave different gradients"
            assert torch.equal(ma, mb) and torch.equal(va, vb), f"step {t}: moments differ"
        budget += A.dev_vs_host_bound(pa.double(), pa.double() - pa0.double())
        err = (pa.double() - pb.double()).abs()
        if identical:
            worst = (err / budget.clamp_min(1e-300)).max().item()
            assert (err <= budget).all(), f"step {t}: max |dp| / bound {worst:.3g}"
        same_p = torch.equal(pa, pb)
        print(f"step {t}: capturable == plain bit for bit: params {same_p}")
        identical = identical and same_p
    if not identical:
        # past a (bounded) parameter difference the gradients differ too; the runs must still agree closely
        torch.testing.assert_close(runs["plain"][-1][2][0], runs["capturable"][-1][2][0], rtol=1e-5, atol=1e-6)


def _resume(mode, uninterrupted, msd, checkpoint, via):
    if via == "cpu_file":
        f = io.BytesIO()
        torch.save(checkpoint, f)
        f.seek(0)
        osd = torch.load(f, map_location="cpu")
        assert osd["flat_state"]["exp_avg"].device.type == "cpu"
    else:
        osd = copy.deepcopy(checkpoint)
    m2, opt2 = _build(mode)
    m2.load_state_dict(msd)
    keep = osd["flat_state"]
    pristine = copy.deepcopy(osd)
    for _ in range(2 if via == "twice" else 1):
        opt2.load_state_dict(osd)
        assert set(osd) == set(pristine) and osd["flat_state"] is keep, "load_state_dict changed its argument"
    assert opt2.state_dict()["flat_state"]["step"] == 3
    assert opt2.param_groups[0]["lr"] == 3e-4
    got = _steps(m2, opt2, range(3, 6))
    assert opt2.state_dict()["flat_state"]["step"] == 6
    # the loaded dict is the caller's: neither the loads nor the three steps after them touched it
    assert osd["flat_state"]["step"] == 3
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(osd["flat_state"][k], pristine["flat_state"][k]), f"{k} of the loaded dict changed"
    assert osd["param_groups"] == pristine["param_groups"]
    for what, u, v in zip(("params", "exp_avg", "exp_avg_sq"), uninterrupted, got):
        assert torch.equal(u, v), f"{mode} via {via}: {what} differ, max |diff| {(u - v).abs().max().item():.3e}"


@pytest.mark.parametrize("mode", MODES)
def test_resume_is_bit_identical(mode):
    """6 steps uninterrupted, with the model's and the optimizer's state_dict taken after the third (copied: the
    live optimizer's dict aliases its moments), against a fresh model and optimizer that load them and run steps
    4 to 6: same kernels, same inputs, so bit-identical parameters and moments"""
    m, opt = _build(mode)
    _steps(m, opt, range(3))
    msd = copy.deepcopy(m.state_dict())
    checkpoint = copy.deepcopy(opt.state_dict())
    assert checkpoint["flat_state"]["step"] == 3
    full = _steps(m, opt, range(3, 6))
    assert opt.state_dict()["flat_state"]["step"] == 6
    del m, opt
    for via in ("direct", "cpu_file", "twice"):
        _resume(mode, full, msd, checkpoint, via)


def test_load_refuses_a_state_of_another_size():
    m, opt = _build("plain")
    _steps(m, opt, range(1))
    before = _snap(m, opt)
    sd = opt.state_dict()
    bad = dict(sd, flat_state=dict(sd["flat_state"], exp_avg=sd["flat_state"]["exp_avg"][:-1].clone()))
    with pytest.raises(ValueError, match="shape"):
        opt.load_state_dict(bad)
    assert opt._step == 1 and _same(before, _snap(m, opt))


def test_refused_combinations_still_raise():
    from unetseg_hip import losses
    from unetseg_hip.arena import FusedAdam
    from utils.synthetic import make_batch

    m, opt = _build("overlap")
    with pytest.raises(ValueError):
        FusedAdam(m, overlap=True, capturable=True)
    x, y = make_batch(2, 64, seed=1)
    opt.zero_grad()
    losses.binary_segmentation_loss(m(x.to(DEV)), y.to(DEV), "lovasz_hinge").backward()
    with pytest.raises(ValueError):
        opt.step(grad_scale=torch.ones(1, device=DEV))
