"""GPU: the multiclass loss / confusion kernels (csrc/multiclass.hip) against float64 references, past
one block.

mc_loss_partial / finalize / bwd: the fixtures of test_multiclass_losses_golden hold <= 960 pixels
(4 blocks).  Here: one mostly idle block, 22 blocks with image boundaries inside a block, C = 32 (the
register-array edge) with saturated softmax (pt == 1 pixels), 270 336 pixels (past the 1024 x 256
grid: the grid-stride second pass), and C = 2 / C = 1; CE with and without class weights, Focal with
alpha None and gamma 0 / 1 / 2, Dice with beta != 1 and a smooth that matters, an upstream gradient
other than 1, every target ignored, and the C ABI's combined CE + Dice launch and its loss[1] / loss[2].
Reference: oracle/ref_cpu.py ce_loss / focal_loss / dice_loss (model/unet_training.py:9-91) in float64
on the same fp32-representable inputs.
Tolerance: that of test_multiclass_losses_golden -- loss 1e-5 relative, gradient 1e-5 of its maximum
(+1e-9).  The fp32 evaluation of the same oracle differs from float64 by at most 1.8e-7 (loss) and
1.3e-6 (gradient) at these sizes, so the bound has room (DESIGN.md section 4 holds the measured maxima).

mc_confusion: the whole [(C+1), C] histogram, exactly, against numpy: targets outside [0, C) -> row C,
exact ties -> the lowest class (torch.max), accumulation into an existing histogram, 532 480 pixels
(past the 2048 x 256 grid).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

LOSS_TOL, GRAD_TOL = 1e-5, 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


#: B, C, H, W, logit scale
SIZES = [(1, 3, 7, 5, 1.0), (3, 21, 37, 50, 1.0), (2, 32, 37, 50, 30.0), (2, 5, 384, 352, 1.0), (2, 2, 16, 16, 1.0),
         (2, 1, 9, 9, 1.0)]

#: name -> (kind, parameters)
VARIANTS = {
    "ce_w": ("ce", True),
    "ce_1": ("ce", False),
    "focal_a0.5_g2": ("focal", (0.5, 2)),
    "focal_aNone_g1": ("focal", (None, 1)),
    "focal_a0.25_g0": ("focal", (0.25, 0)),
    "dice_b1_s1e-5": ("dice", (1, 1e-5)),
    "dice_b2_s1": ("dice", (2, 1.0)),
}


@functools.lru_cache(maxsize=None)
def _inputs(B, C, H, W, scale):
    """fp32 logits, targets in [0, C] (C = the ignore label), class weights 0.5 + rand, one-hot with
    ct = C + 1 channels"""
    g = torch.Generator().manual_seed(1000 * C + H)
    lg = torch.randn(B, C, H, W, generator=g) * scale
    tgt = torch.randint(0, C + 1, (B, H, W), generator=g)
    cw = 0.5 + torch.rand(C, generator=g)
    oh = torch.eye(C + 1)[tgt.reshape(-1)].reshape(B, H, W, C + 1)
    return lg, tgt, cw, oh


def _ref(kind, par, x, tgt, cw, oh, C):
    from oracle import ref_cpu
    if kind == "ce":
        return ref_cpu.ce_loss(x, tgt, cw.double() if par else torch.ones(C, dtype=torch.float64), num_classes=C)
    if kind == "focal":
        return ref_cpu.focal_loss(x, tgt, cw.double(), num_classes=C, alpha=par[0], gamma=par[1])
    return ref_cpu.dice_loss(x, oh.double(), beta=par[0], smooth=par[1])


def _hip(kind, par, x, tgt, cw, oh, C):
    from unetseg_hip import losses
    if kind == "ce":
        return losses.ce_loss(x, tgt.to(DEV), cw.to(DEV) if par else torch.ones(C, device=DEV), num_classes=C)
    if kind == "focal":
        return losses.focal_loss(x, tgt.to(DEV), cw.to(DEV), num_classes=C, alpha=par[0], gamma=par[1])
    return losses.dice_loss(x, oh.to(DEV), beta=par[0], smooth=par[1])


def _check(tag, v, ref, gd, gr):
    """loss 1e-5 relative, gradient 1e-5 of its maximum (+1e-9); prints the measured figures"""
    v, ref = float(v), float(ref)
    gd, gr = gd.detach().cpu().double(), gr.double()
    lerr = abs(v - ref)
    gerr = (gd - gr).abs().max().item()
    gmax = gr.abs().max().item()
    print(f"MCERR {tag}: loss {v:.9g} ref {ref:.9g} rel {lerr / max(abs(ref), 1e-300):.2e}  "
          f"grad err {gerr:.3e} of max {gmax:.3e} = {gerr / max(gmax, 1e-300):.2e}")
    assert lerr <= LOSS_TOL * abs(ref), (tag, v, ref)
    assert torch.isfinite(gd).all(), tag
    assert gerr <= GRAD_TOL * gmax + 1e-9, (tag, gerr, gmax)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B,C,H,W,scale", SIZES)
def test_mc_loss_vs_float64(B, C, H, W, scale, variant):
    """loss value and logit gradient of CE / Focal / Dice.  focal_a0.25_g0 at the x30 size (and at
    C = 1) has pixels with pt == 1: gamma * (1 - pt)^(gamma - 1) is 0 * 0^-1 there, which the kernel
    must give as 0, as torch's pow backward does for a zero exponent."""
    kind, par = VARIANTS[variant]
    lg, tgt, cw, oh = _inputs(B, C, H, W, scale)
    x64 = lg.double().requires_grad_(True)
    ref = _ref(kind, par, x64, tgt, cw, oh, C)
    ref.backward()
    x = lg.to(DEV).requires_grad_(True)
    v = _hip(kind, par, x, tgt, cw, oh, C)
    v.backward()
    _check(f"{variant} {B}x{C}x{H}x{W}", v.item(), ref.item(), x.grad, x64.grad)


@pytest.mark.parametrize("variant", ["ce_w", "focal_a0.5_g2", "dice_b2_s1"])
def test_mc_loss_upstream_gradient(variant):
    """backward of 2.5 * loss: the gscale device scalar of mc_loss_bwd"""
    kind, par = VARIANTS[variant]
    B, C, H, W, scale = SIZES[1]
    lg, tgt, cw, oh = _inputs(B, C, H, W, scale)
    x64 = lg.double().requires_grad_(True)
    ref = _ref(kind, par, x64, tgt, cw, oh, C)
    (2.5 * ref).backward()
    x = lg.to(DEV).requires_grad_(True)
    v = _hip(kind, par, x, tgt, cw, oh, C)
    (2.5 * v).backward()
    _check(f"{variant} x2.5", v.item(), ref.item(), x.grad, x64.grad)


@pytest.mark.parametrize("kind", ["ce", "focal"])
def test_mc_loss_all_ignored(kind):
    """every target is the ignore label: float64 torch gives NaN for CE (0 / 0 weight sum) and 0 for
    Focal (a mean of zeros over every pixel), with an all-zero logit gradient in both; so does the
    kernel (compared with equal_nan, and asserted)"""
    from oracle import ref_cpu
    from unetseg_hip import losses
    B, C, H, W = 2, 5, 9, 11
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(B, C, H, W, generator=g)
    tgt = torch.full((B, H, W), C, dtype=torch.long)
    cw = 0.5 + torch.rand(C, generator=g)
    x64 = lg.double().requires_grad_(True)
    x = lg.to(DEV).requires_grad_(True)
    if kind == "ce":
        ref = ref_cpu.ce_loss(x64, tgt, cw.double(), num_classes=C)
        v = losses.ce_loss(x, tgt.to(DEV), cw.to(DEV), num_classes=C)
        assert torch.isnan(ref).item() and torch.isnan(v).item()
    else:
        ref = ref_cpu.focal_loss(x64, tgt, cw.double(), num_classes=C)
        v = losses.focal_loss(x, tgt.to(DEV), cw.to(DEV), num_classes=C)
        assert ref.item() == 0.0 and v.item() == 0.0
    ref.backward()
    v.backward()
    torch.testing.assert_close(x.grad.cpu().double(), x64.grad, rtol=0, atol=0, equal_nan=True)
    assert (x64.grad == 0).all()


# ------------------------------------------------------------------------------------------------
# the C ABI directly, called the way losses._McLossFn does
# ------------------------------------------------------------------------------------------------
def _abi(lg, tgt, cw, dice_t, kind, C, beta, smooth, ignore):
    """-> (loss[3], dout) of unetseg_mc_loss_fwd / _bwd with gscale NULL"""
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P
    out = lg.to(DEV).contiguous()
    B = out.shape[0]
    Pn = out[0, 0].numel()
    t = tgt.to(DEV).contiguous() if tgt is not None else None
    w = cw.to(DEV).contiguous() if cw is not None else None
    dt = dice_t.to(DEV).float().contiguous()
    nb = lib.mc_loss_workspace(B, C, Pn)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = (P(out), P(t), B, C, Pn, P(w), int(ignore), int(kind), -1.0, 0.0, P(dt), dt.shape[-1], float(beta),
            float(smooth))
    lib.mc_loss_fwd(*args, P(ws), nb, P(loss), st)
    dout = torch.full_like(out, float("nan"))
    lib.mc_loss_bwd(*args, P(ws), 0, P(dout), st)
    torch.cuda.synchronize()
    return loss.cpu().double(), dout.cpu().double()


def test_mc_loss_abi_combined_ce_dice():
    """CE + Dice in one launch (main term 0 with a Dice target): loss[0] = loss[1] + loss[2], each slot
    against its float64 oracle value, dout against the gradient of the sum"""
    from oracle import ref_cpu
    from unetseg_hip.losses import MC_CE
    B, C, H, W, scale = SIZES[1]
    lg, tgt, cw, oh = _inputs(B, C, H, W, scale)
    x64 = lg.double().requires_grad_(True)
    ce = ref_cpu.ce_loss(x64, tgt, cw.double(), num_classes=C)
    dice = ref_cpu.dice_loss(x64, oh.double(), beta=1, smooth=1e-5)
    (ce + dice).backward()
    loss, dout = _abi(lg, tgt, cw, oh, MC_CE, C, 1, 1e-5, C)
    print(f"MCERR abi ce+dice: {loss.tolist()} ref ce {ce.item():.9g} dice {dice.item():.9g}")
    assert abs(loss[0] - (loss[1] + loss[2])) <= 1e-6 * abs(loss[0])
    assert abs(loss[1].item() - ce.item()) <= LOSS_TOL * abs(ce.item())
    assert abs(loss[2].item() - dice.item()) <= LOSS_TOL * abs(dice.item())
    _check("abi ce+dice", loss[0].item(), (ce + dice).item(), dout, x64.grad)


def test_mc_loss_abi_dice_wide_target():
    """a Dice target with ct = C + 3 channels: the header's contract is "first C channels", so the
    reference is the explicit formula (model/unet_training.py:67-91) on target[..., :C]"""
    from unetseg_hip.losses import MC_NONE
    B, C, H, W = 2, 5, 37, 50
    g = torch.Generator().manual_seed(9)
    lg = torch.randn(B, C, H, W, generator=g)
    lab = torch.randint(0, C + 3, (B, H, W), generator=g)
    oh = torch.eye(C + 3)[lab.reshape(-1)].reshape(B, H, W, C + 3)
    beta, smooth = 2, 1.0
    x64 = lg.double().requires_grad_(True)
    p = torch.softmax(x64.permute(0, 2, 3, 1).reshape(B, -1, C), -1)
    t = oh.double().reshape(B, -1, C + 3)[..., :C]
    tp = (t * p).sum((0, 1))
    fp = p.sum((0, 1)) - tp
    fn = t.sum((0, 1)) - tp
    score = ((1 + beta ** 2) * tp + smooth) / ((1 + beta ** 2) * tp + beta ** 2 * fn + fp + smooth)
    ref = 1 - score.mean()
    ref.backward()
    loss, dout = _abi(lg, None, None, oh, MC_NONE, C, beta, smooth, -1)
    assert loss[1].item() == 0.0 and loss[0].item() == loss[2].item()
    _check("abi dice ct=C+3", loss[0].item(), ref.item(), dout, x64.grad)


# ------------------------------------------------------------------------------------------------
# confusion histogram
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conf_inputs(B, C, H, W):
    """logits with ~5 % of the pixels holding the exact same maximum in two or three classes; targets
    in [0, C) plus C, -1, C + 5 and 255 (all row C)"""
    g = torch.Generator().manual_seed(77 * C + W)
    lg = torch.randn(B, C, H, W, generator=g)
    flat = lg.permute(0, 2, 3, 1).reshape(-1, C).clone()
    n = flat.shape[0]
    tie = torch.nonzero(torch.rand(n, generator=g) < 0.05).flatten()
    mx = flat[tie].max(1).values
    for _ in range(3 if C > 2 else 2):
        cls = torch.randint(0, C, (tie.numel(),), generator=g)
        flat[tie, cls] = mx
    flat[4, 0] = flat[4, C - 1] = flat[4].max()  # at least one tie at every size
    lg = flat.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    tgt = torch.randint(0, C, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    for k, val in enumerate((C, -1, C + 5, 255)):
        tgt[(r >= 0.03 * k) & (r < 0.03 * (k + 1))] = val
        tgt.view(-1)[k] = val
    return lg, tgt


@pytest.mark.parametrize("B,C,H,W", [(1, 2, 7, 5), (3, 21, 37, 50), (2, 32, 37, 50), (2, 3, 520, 512)])
def test_mc_confusion_histogram(B, C, H, W):
    from unetseg_hip import losses
    lg, tgt = _conf_inputs(B, C, H, W)
    x = lg.permute(0, 2, 3, 1).reshape(-1, C).numpy()
    pred = x.argmax(1)  # first maximum
    ntie = int(((x == x.max(1, keepdims=True)).sum(1) > 1).sum())
    assert ntie > 0
    t = tgt.reshape(-1).numpy()
    assert all((t == v).any() for v in (C, -1, C + 5, 255))
    row = np.where((t >= 0) & (t < C), t, C)
    ref = np.zeros((C + 1, C), dtype=np.int64)
    np.add.at(ref, (row, pred), 1)
    hist = losses.mc_confusion(lg.to(DEV), tgt.to(DEV))
    assert hist.shape == (C + 1, C)
    np.testing.assert_array_equal(hist.cpu().numpy(), ref)
    again = losses.mc_confusion(lg.to(DEV), tgt.to(DEV), hist)
    assert again is hist
    np.testing.assert_array_equal(hist.cpu().numpy(), 2 * ref)


def test_mc_metrics_from_histogram():
    """the four metrics derived from the kernel's histogram against the oracle's per-class loop
    (utils/train_and_eval.py:20-103), rtol 1e-12.  The oracle's pixel accuracy alone is a float32
    quotient (ref_cpu.mc_metrics: `(pred == target).float().sum() / target.numel()`), so that figure is
    held to 1e-12 against the same integer ratio in float64 and to the oracle's float32 rounding
    (2^-23) against the oracle's own value; the other three are Python-float ratios of integers."""
    from oracle import ref_cpu
    from unetseg_hip import losses
    B, C, H, W = 3, 21, 37, 50
    lg, tgt = _conf_inputs(B, C, H, W)
    hist = losses.mc_confusion(lg.to(DEV), tgt.to(DEV))
    m = losses.mc_metrics_from_hist(hist.cpu().numpy())
    got = [m[k] for k in ("Pixel Accuracy", "Mean Accuracy", "Mean IoU", "Frequency Weighted IoU")]
    ref = ref_cpu.mc_metrics(lg, tgt, C)
    pix = int((lg.argmax(1) == tgt).sum()) / tgt.numel()
    np.testing.assert_allclose(got, [pix] + list(ref[1:]), rtol=1e-12)
    np.testing.assert_allclose(got[0], ref[0], rtol=2.0 ** -23)
