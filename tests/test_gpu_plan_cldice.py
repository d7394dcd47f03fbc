"""GPU: a training step whose loss carries the soft-clDice term records into a step plan and replays bit for bit.

As tests/test_gpu_plan.py: two identical models train on the same two batches in turn, model A eagerly, model B
with one eager step, one recorded step and three replays; parameters, gradients, Adam moments, BN buffers and the
loss must be torch.equal after every step.  The clDice term reads the batch's target and logits behind the C ABI
only (unetseg_cldice_fwd), so the plan rebases its pointers like any other launch, and it adds no torch op:
the recorded step has no more of them than the same configuration records with weight 0.
"""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


def _setup(name, loss_name, weight, seed=11):
    from model.model_factory import create_model
    from unetseg_hip.arena import FusedAdam
    from unetseg_hip.losses import binary_segmentation_loss, multitask_loss

    torch.manual_seed(seed)
    multitask = name == "multitask_unet"
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model(name, weights="", num_classes=1 if multitask else 2).to(DEV).train()
    model.compute_dtype = "bf16"
    opt = FusedAdam(model, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-4, overlap=True, bucket_mb=8.0)

    def step(x, y, c):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if multitask:
                seg, cls = model(x)
                loss = multitask_loss(seg, cls, y, c, 1.0, loss_name, cldice_weight=weight)[0]
            else:
                loss = binary_segmentation_loss(model(x), y, loss_name, cldice_weight=weight)
        loss.backward()
        opt.step()
        return loss

    return model, opt, step


def _state(model, opt, loss):
    bufs = torch.cat([b.detach().double().reshape(-1) for b in model.buffers()])
    return (model._flat.clone(), model._flat_grad.clone(), opt._m.clone(), opt._v.clone(), bufs,
            loss.detach().clone(), opt._step)


def _planned(name, loss_name, weight, data, nsteps):
    """one eager step, one recorded, nsteps - 2 replayed -> (states, plan statistics)"""
    from unetseg_hip.plan import StepPlan
    model, opt, step = _setup(name, loss_name, weight)
    got = [_state(model, opt, step(*data[0]))]
    rec_in = tuple(t.clone() for t in data[1])
    plan = StepPlan({"x": rec_in[0], "y": rec_in[1], "c": rec_in[2]})
    got.append(_state(model, opt, plan.record(lambda: step(*rec_in))))
    for i in range(2, nsteps):
        x, y, c = data[i % 2]
        got.append(_state(model, opt, plan.replay(x=x, y=y, c=c)))
    torch.cuda.synchronize()
    return got, plan.stats()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,loss_name", [("unet_resnet50", "lovasz_hinge"), ("multitask_unet", "bce")])
def test_plan_replay_with_cldice(name, loss_name):
    from utils.synthetic import make_batch

    batch, size, weight, nsteps = 2, 128, 0.3, 5
    stream = torch.cuda.Stream(DEV)
    prev = torch.cuda.current_stream(DEV)
    torch.cuda.set_stream(stream)
    try:
        data = []
        for i in range(2):
            x, y, c = make_batch(batch, size, seed=1234 + i, with_cls=True)
            data.append((x.to(DEV), y.to(DEV), c.to(DEV)))
        ma, oa, sa = _setup(name, loss_name, weight)
        ref = [_state(ma, oa, sa(*data[i % 2])) for i in range(nsteps)]
        torch.cuda.synchronize()
        del ma, oa, sa
        torch.cuda.empty_cache()
        got, st = _planned(name, loss_name, weight, data, nsteps)
        base, st0 = _planned(name, loss_name, 0.0, data, 2)
        print(f"\n{name}: plan with the clDice term {st}\n{name}: plan with weight 0 {st0}")
        assert st["torch_ops"] <= st0["torch_ops"], (st, st0)
        assert st["c_calls"] > st0["c_calls"]
        # the term is in the objective: the first step's loss differs from the weight-0 step's
        assert not torch.equal(got[0][5], base[0][5])
        names = ("params", "grads", "adam m", "adam v", "BN buffers", "loss", "step")
        for i, (a, b) in enumerate(zip(ref, got)):
            for n, u, v in zip(names, a, b):
                if isinstance(u, torch.Tensor):
                    assert torch.equal(u, v), f"step {i}: {n} differ (max {((u.double() - v.double()).abs().max().item()):.3e})"
                else:
                    assert u == v, f"step {i}: {n} {u} != {v}"
    finally:
        torch.cuda.set_stream(prev)
