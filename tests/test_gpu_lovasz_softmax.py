"""GPU: the fused Lovasz-softmax loss (csrc/lovasz_softmax.hip, unetseg_lovasz_softmax_fwd) against the
float64 restatement of its definition (tests/lovasz_softmax_ref.py), through the autograd op, the
reference-style wrapper and the multiclass train / eval loops.

Inputs: fp32 logits randn x 2, labels uniform in [0, C] with ignore_index = C.  Shapes chosen for the
sort's edges: (2,5,72,68) two radix tiles per segment, the last one partial; (1,21,96,96) three tiles
(the chunk kernel's carry of the positives before a tile) with one class absent; (3,3,65,64) whose
12480-key batch-mode segments have tile boundaries inside an image; (2,2,24,20) one partial tile and the
minimum C; (1,32,40,40) the maximum C.

Loss: 1e-5 relative, the bound of the hinge tests (the fp32 and fp64 restatements agree to 1e-7).
Gradient: the softmax is rounded differently on the two sides, so near-equal errors can swap ranks;
the test measures the fp32 restatement's deviation from the fp64 one (max-abs over max-abs) and holds
the HIP gradient to 3x that noise floor.  A wrong Jacobian, weight or gate is O(1) on that scale.  The
measured figures are printed (pytest -s) and recorded in DESIGN.md.
"""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from lovasz_softmax_ref import loss_and_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"

LOSS_TOL = 1e-5
U32 = 2.0 ** -24  # unit roundoff of fp32

#: B, C, H, W
SHAPES = [(2, 5, 72, 68), (1, 21, 96, 96), (3, 3, 65, 64), (2, 2, 24, 20), (1, 32, 40, 40)]
ABSENT = {(1, 21, 96, 96): 7}  # class removed from the labels of that shape


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


@functools.lru_cache(maxsize=None)
def _inputs(B, C, H, W, ties=False):
    g = torch.Generator().manual_seed(100 * C + H)
    lg = torch.randn(B, C, H, W, generator=g) * 2
    if ties:
        lg = torch.round(lg * 2) / 2  # multiples of 0.5: thousands of equal errors per segment
    tgt = torch.randint(0, C + 1, (B, H, W), generator=g)
    a = ABSENT.get((B, C, H, W))
    if a is not None:
        tgt[tgt == a] = a + 1
    return lg, tgt


@functools.lru_cache(maxsize=None)
def _ref(B, C, H, W, per_image, dtype=torch.float64, ties=False):
    lg, tgt = _inputs(B, C, H, W, ties)
    return loss_and_grad(lg, tgt, C, per_image, dtype)


def _run(lg, tgt, ignore, per_image):
    from unetseg_hip import losses
    x = lg.to(DEV).requires_grad_(True)
    loss = losses.lovasz_softmax_loss(x, tgt.to(DEV), ignore, per_image)
    loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def _hip(B, C, H, W, per_image, ties=False):
    lg, tgt = _inputs(B, C, H, W, ties)
    return _run(lg, tgt, C, per_image)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _dev(g, ref):
    return float((g.double() - ref).abs().max()) / float(ref.abs().max())


def _check_exact(grad, tgt, C):
    """0 at every invalid pixel; per pixel the C gradients sum to 0 within C roundings of the largest"""
    g = grad.double()
    invalid = (tgt < 0) | (tgt >= C)
    assert float(g.abs().amax(1)[invalid].max() if invalid.any() else 0.0) == 0.0
    assert torch.isfinite(g).all()
    s = g.sum(1).abs()
    bound = C * U32 * g.abs().amax(1)
    assert bool((s <= bound).all()), float((s - bound).max())


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient(shape, per_image):
    l64, g64 = _ref(*shape, per_image)
    l32, g32 = _ref(*shape, per_image, torch.float32)
    loss, grad = _hip(*shape, per_image)
    floor, dev = _dev(g32, g64), _dev(grad, g64)
    print(f"\nlovasz_softmax {shape} per_image={per_image}: loss hip {float(loss):.8f} ref64 {l64:.8f} "
          f"rel {_rel(float(loss), l64):.2e} (ref32 rel {_rel(l32, l64):.2e}); grad dev hip {dev:.2e} "
          f"ref32 floor {floor:.2e}")
    assert _rel(float(loss), l64) <= LOSS_TOL
    assert dev <= 3 * floor


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exact_properties(shape, per_image):
    _, tgt = _inputs(*shape)
    _, grad = _hip(*shape, per_image)
    _check_exact(grad, tgt, shape[1])


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_absent_class_contributes_nothing(per_image):
    """The last class never occurs in the labels and its logit plane is so low that its probability is
    exactly 0.  Changing that plane, or deleting it (the same problem with C - 1 classes), must not move
    the loss or the other planes' gradient: the absent class has no loss term, no dL/dp and no share in
    the mean over the present classes."""
    B, C, H, W = 2, 5, 72, 68
    lg, tgt = _inputs(B, C, H, W)
    lg, tgt = lg.clone(), tgt.clone()
    tgt[tgt == C - 1] = C - 2
    lg[:, C - 1] = -1.0e4
    la, ga = _run(lg, tgt, C, per_image)
    lg2 = lg.clone()
    lg2[:, C - 1] = -2.0e4 - 1.0e3 * torch.rand(B, H, W, generator=torch.Generator().manual_seed(3))
    lb, gb = _run(lg2, tgt, C, per_image)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert float(ga[:, C - 1].abs().max()) == 0.0
    tgt3 = torch.where(tgt == C, torch.full_like(tgt, C - 1), tgt)
    lc, gc = _run(lg[:, :C - 1].contiguous(), tgt3, C - 1, per_image)
    assert _rel(float(lc), float(la)) <= 2 * U32  # the final sum visits the segments in another order
    assert torch.equal(gc, ga[:, :C - 1])
    l64, _ = loss_and_grad(lg, tgt, C, per_image)
    assert _rel(float(la), l64) <= LOSS_TOL


def test_degenerate_segments():
    B, C, H, W = 2, 5, 72, 68
    lg, tgt = _inputs(B, C, H, W)
    # an image whose pixels are all ignored, beside a normal one
    t1 = tgt.clone()
    t1[1] = C
    loss, grad = _run(lg, t1, C, True)
    alone, galone = _run(lg[:1], t1[:1], C, True)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert float(grad[1].abs().max()) == 0.0
    assert _rel(float(loss), 0.5 * float(alone)) <= 2 * U32
    assert torch.equal(grad[0], 0.5 * galone[0])
    assert _rel(float(loss), loss_and_grad(lg, t1, C, True)[0]) <= LOSS_TOL
    lb, gb = _run(lg, t1, C, False)  # the batch segment is image 0 alone
    assert _rel(float(lb), float(alone)) <= 2 * U32 and float(gb[1].abs().max()) == 0.0
    # the whole batch ignored (and labels outside [0, C) that are not ignore_index count as ignored)
    t0 = torch.full_like(tgt, C)
    t0[0, :3] = -1
    t0[1, :3] = C + 5
    for per_image in (True, False):
        loss, grad = _run(lg, t0, C, per_image)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    # an image labelled with one class everywhere
    t2 = tgt.clone()
    t2[0] = 3
    for per_image in (True, False):
        loss, grad = _run(lg, t2, C, per_image)
        assert _rel(float(loss), loss_and_grad(lg, t2, C, per_image)[0]) <= LOSS_TOL
        _check_exact(grad, t2, C)
    # a class present in image 0 and absent in image 1: the two modes differ, each matches
    # (image 1 still predicts it often: errors of that class in the batch segment, none per image)
    t3, lg3 = tgt.clone(), lg.clone()
    t3[1][t3[1] == 2] = 1
    lg3[1, 2] += 3.0
    li, _ = _run(lg3, t3, C, True)
    lb, _ = _run(lg3, t3, C, False)
    ri, rb = loss_and_grad(lg3, t3, C, True)[0], loss_and_grad(lg3, t3, C, False)[0]
    assert _rel(float(li), ri) <= LOSS_TOL and _rel(float(lb), rb) <= LOSS_TOL
    assert _rel(ri, rb) > 100 * LOSS_TOL and _rel(float(li), float(lb)) > 100 * LOSS_TOL


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_heavy_ties(per_image):
    """logits on a 0.5 grid: the value is tie-order independent and the exact properties hold; no
    gradient comparison (tie order is by contract, the softmax's rounding is not)"""
    shape = (2, 5, 72, 68)
    _, tgt = _inputs(*shape, ties=True)
    l64, _ = _ref(*shape, per_image, ties=True)
    loss, grad = _hip(*shape, per_image, ties=True)
    assert _rel(float(loss), l64) <= LOSS_TOL
    _check_exact(grad, tgt, shape[1])


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_deterministic(per_image):
    shape = (3, 3, 65, 64)
    lg, tgt = _inputs(*shape)
    la, ga = _hip(*shape, per_image)
    lb, gb = _run(lg, tgt, shape[1], per_image)
    assert torch.equal(la, lb) and torch.equal(ga, gb)


def test_bf16_logits():
    from unetseg_hip import losses
    B, C, H, W = 2, 5, 72, 68
    lg, tgt = _inputs(B, C, H, W)
    xb = lg.to(DEV).bfloat16().requires_grad_(True)
    loss = losses.lovasz_softmax_loss(xb, tgt.to(DEV), C)
    loss.backward()
    assert torch.isfinite(loss) and xb.grad.dtype == torch.bfloat16
    l32, g32 = _run(xb.detach().float().cpu(), tgt, C, True)
    assert torch.equal(loss.cpu(), l32)
    assert torch.equal(xb.grad.cpu(), g32.bfloat16())


def test_value_only_and_upstream_scale():
    """no gradient requested: the same value; an upstream factor scales the unit gradient"""
    from unetseg_hip import losses
    shape = (2, 2, 24, 20)
    lg, tgt = _inputs(*shape)
    la, ga = _hip(*shape, True)
    with torch.no_grad():
        lv = losses.lovasz_softmax_loss(lg.to(DEV), tgt.to(DEV), shape[1])
    assert torch.equal(lv.cpu(), la)
    x = lg.to(DEV).requires_grad_(True)
    (losses.lovasz_softmax_loss(x, tgt.to(DEV), shape[1]) * 0.25).backward()
    assert torch.equal(x.grad.cpu(), 0.25 * ga)


def test_wrappers():
    from model.unet_training import Dice_loss, Lovasz_Softmax_Loss
    from unetseg_hip import losses
    from utils.train_and_eval import _mc_loss
    B, C, H, W = 2, 5, 72, 68
    lg, tgt = _inputs(B, C, H, W)
    x, t = lg.to(DEV), tgt.to(DEV)
    oh = torch.eye(C + 1, device=DEV)[t.reshape(-1)].reshape(B, H, W, C + 1)
    for per_image in (True, False):
        assert torch.equal(Lovasz_Softmax_Loss(x, t, num_classes=C, per_image=per_image),
                           losses.lovasz_softmax_loss(x, t, C, per_image))
    w = torch.ones(C, device=DEV)
    got = _mc_loss(x, t, oh, w, C, dice_loss=True, focal_loss=False, lovasz_softmax=True)
    want = Lovasz_Softmax_Loss(x, t, num_classes=C) + Dice_loss(x, oh)
    assert torch.equal(got, want)
    assert torch.equal(_mc_loss(x, t, oh, w, C, False, True, lovasz_softmax=True), Lovasz_Softmax_Loss(x, t, C))
    # positional calls behave as before
    from model.unet_training import CE_Loss
    assert torch.equal(_mc_loss(x, t, oh, w, C, False, False), CE_Loss(x, t, w, C))


def test_resized_logits():
    """logits at 32^2 against labels at 64^2 go through the align_corners=True resize first"""
    C = 4
    g = torch.Generator().manual_seed(21)
    lg = torch.randn(2, C, 32, 32, generator=g) * 2
    tgt = torch.randint(0, C + 1, (2, 64, 64), generator=g)
    loss, grad = _run(lg, tgt, C, True)
    from lovasz_softmax_ref import lovasz_softmax_ref

    def ref(dtype):
        x = lg.to(dtype).requires_grad_(True)
        up = torch.nn.functional.interpolate(x, size=(64, 64), mode="bilinear", align_corners=True)
        val = lovasz_softmax_ref(up, tgt, C, True, dtype)
        val.backward()
        return float(val.detach()), x.grad.double()

    l64, g64 = ref(torch.float64)
    _, g32 = ref(torch.float32)
    floor, dev = _dev(g32, g64), _dev(grad, g64)
    print(f"\nlovasz_softmax resized 32->64: loss rel {_rel(float(loss), l64):.2e}; grad dev hip {dev:.2e} "
          f"ref32 floor {floor:.2e}")
    assert _rel(float(loss), l64) <= LOSS_TOL
    assert grad.shape == lg.shape and torch.isfinite(grad).all()
    assert dev <= 3 * floor  # the rule of test_value_and_gradient


def test_train_and_eval_loops():
    """evaluate / train_one_epoch with lovasz_softmax=True: two batches of unet_plain at 64^2, four
    classes plus background (five logit channels); finite values, and the step moves the parameters"""
    from model.model_factory import build_model
    from unetseg_hip.arena import FusedAdam
    from utils.train_and_eval import evaluate, train_one_epoch
    C = 5
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = build_model("unet_plain", num_classes=C)
    m = m.to(DEV)
    m.compute_dtype = "fp32"
    g = torch.Generator().manual_seed(8)
    batches = []
    for _ in range(2):
        x = torch.rand(2, 3, 64, 64, generator=g)
        t = torch.randint(0, C + 1, (2, 64, 64), generator=g)
        batches.append((x, t, torch.eye(C + 1)[t.reshape(-1)].reshape(2, 64, 64, C + 1)))
    with contextlib.redirect_stdout(io.StringIO()):
        met = evaluate(m, batches, torch.device(DEV), True, False, C, lovasz_softmax=True)
        ce = evaluate(m, batches, torch.device(DEV), True, False, C)
    assert all(np.isfinite(v) for v in met.values())
    assert met["Loss"] != ce["Loss"] and met["Mean IoU"] == ce["Mean IoU"]
    opt = FusedAdam(m, lr=1e-3)
    before = m._flat.clone()
    with contextlib.redirect_stdout(io.StringIO()):
        lt = train_one_epoch(m, opt, batches, torch.device(DEV), True, False, 0.0, C, None, 0, 1, lovasz_softmax=True)
    assert np.isfinite(lt) and not torch.equal(before, m._flat)
