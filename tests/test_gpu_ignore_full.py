"""GPU: ignore_index in the binary losses and confusion counts past the 3 x 20 x 24 fixture
(ignore.npz, test_ignore_index_golden): csrc/loss.hip lovasz_fwd_masked, masked_loss_fwd,
confusion_masked.

* Per-image masked Lovasz (model.unet_training.lovasz_hinge_loss(z, tgt, ignore_index)): ignored pixels
  get the key -inf and sort behind every valid pixel as one tie run, so the radix tiles, the cross-tile
  scans and the Jaccard scan's carried counts run with that tail: 4 tiles with a partial last one,
  valid prefixes ending exactly on / one past a tile edge, 130 tiles (past 128 the radix scan keeps its
  runs in memory), an image with nothing ignored and one entirely ignored (loss 0, still counted in the
  mean over B).  Reference: oracle/ref_cpu.py lovasz_hinge_loss_ignore in float32 -- the kernel restates
  the reference's fp32 Jaccard arithmetic (1 - (G - cp) / (G + cn), then a difference), which a float64
  reference would leave by cancellation noise (tests/test_gpu_losses_full.py works the same way, and its
  tolerances hold here: loss 2e-6 relative, gradient 1e-5 of its max).  Inputs come from that file's
  tie-free generator (shifted in the small cases, see SHIFT); a subset of a tie-free set is tie-free.
* Flattened masked BCE / hinge (losses.binary_segmentation_loss(..., ignore_index)) against
  oracle/ref_cpu.py binary_segmentation_loss in float64, 1e-5 / 1e-5 of max (test_ignore_index_golden),
  past one pass of the 8192 x 256 grid.
* binary_confusion(..., ignore_index) exactly, past the 2048 x 256 grid, in both the argmax (2-channel)
  and the sigmoid (1-channel) mode.
"""
import functools

import pytest
import torch

from test_gpu_losses_full import _tie_free

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = 255


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


# ------------------------------------------------------------------------------------------------
# per-image masked Lovasz
# ------------------------------------------------------------------------------------------------
#: _tie_free gives z = (3k + 1) / 2^15 - 4, which for P < 2^15 pixels is negative throughout: every
#: foreground error is then > 0 and every background error < 0, so only the foreground pixels (all inside
#: the first tile) reach the loss.  The small cases shift it by 3.375 to z = (3k + 1 - 20480) / 2^15 in
#: [-0.625, 0.54] (still exact in fp32), so every error is positive and every tile carries loss and
#: gradient.  Still tie-free: 1 - z_i = 1 + z_j needs 3 (k_i + k_j) + 2 = 40960, and 40960 = 1 (mod 3).
SHIFT = 3.375


def _lovasz_case(name):
    """-> z [B,H,W] fp32, tgt [B,H,W] int64 with IGN, flat index of a valid pixel whose hinge error
    is exactly 0 (or None)"""
    if name == "4tiles":  # 12 707 pixels per image: 4 tiles, last one partial
        B, H, W = 3, 97, 131
        g = torch.Generator().manual_seed(21)
        z = _tie_free(B, H, W, g) + SHIFT
        tgt = (torch.rand(B, H, W, generator=g) < 0.3).long()
        tgt[0][torch.rand(H, W, generator=g) < 0.3] = IGN
        tgt[2] = IGN
        # image 1 (nothing ignored): z = 1 with label 1 -> error exactly 0, below every other error (all
        # are > 0.37 here), so the set stays tie-free
        zero = (1, 40, 17)
        z[zero] = 1.0
        tgt[zero] = 1
        return z, tgt, zero
    if name == "tile_edge":  # 12 288 pixels = exactly 3 tiles; 4096 / 4097 valid pixels
        B, H, W = 2, 128, 96
        g = torch.Generator().manual_seed(22)
        z = _tie_free(B, H, W, g) + SHIFT
        tgt = (torch.rand(B, H, W, generator=g) < 0.3).long()
        for b, nvalid in ((0, 4096), (1, 4097)):
            drop = torch.randperm(H * W, generator=g)[nvalid:]
            tgt[b].view(-1)[drop] = IGN
            assert int((tgt[b] != IGN).sum()) == nvalid
        return z, tgt, None
    if name == "130tiles":  # 529 920 pixels, 40 % ignored
        B, H, W = 1, 736, 720
        g = torch.Generator().manual_seed(23)
        z = _tie_free(B, H, W, g)
        tgt = (torch.rand(B, H, W, generator=g) < 0.3).long()
        tgt[torch.rand(B, H, W, generator=g) < 0.4] = IGN
        # the generator's own z = 1 (k = 54613), labelled 1 and kept valid: error exactly 0
        idx = torch.nonzero(z == 1.0)
        assert idx.shape[0] == 1
        zero = tuple(idx[0].tolist())
        tgt[zero] = 1
        return z, tgt, zero
    raise KeyError(name)


@pytest.mark.parametrize("name", ["4tiles", "tile_edge", "130tiles"])
def test_lovasz_image_masked_tie_free(name):
    from model.unet_training import lovasz_hinge_loss
    from oracle import ref_cpu
    z, tgt, zero = _lovasz_case(name)
    zr = z.clone().requires_grad_(True)
    ref = ref_cpu.lovasz_hinge_loss_ignore(zr, tgt, IGN)
    ref.backward()
    zd = z.to(DEV).requires_grad_(True)
    loss = lovasz_hinge_loss(zd, tgt.to(DEV), ignore_index=IGN)
    loss.backward()
    torch.cuda.synchronize()
    gd, gr = zd.grad.cpu().double(), zr.grad.double()
    err = (gd - gr).abs().max().item()
    print(f"IGNERR lovasz_image {name}: loss {loss.item():.9g} ref {ref.item():.9g} "
          f"rel {abs(loss.item() - ref.item()) / abs(ref.item()):.2e}  grad {err / gr.abs().max().item():.2e} of max")
    assert abs(loss.item() - ref.item()) <= 2e-6 * abs(ref.item()), (loss.item(), ref.item())
    assert err <= 1e-5 * gr.abs().max().item(), err
    assert (gd[tgt == IGN] == 0).all()
    if zero is not None:
        assert tgt[zero] == 1 and gd[zero] == 0 and gr[zero] == 0
    if name == "4tiles":
        # the entirely ignored image adds 0 to the sum and 1 to the count: the mean over the other two
        # (a statement about the reference that the comparison above then carries over to the kernel)
        two = ref_cpu.lovasz_hinge_loss_ignore(z[:2], tgt[:2], IGN)
        assert abs(ref.item() - two.item() * 2 / 3) <= 1e-6 * abs(ref.item())


def test_lovasz_image_masked_ties_value():
    """heavy ties (logits on 5 levels) plus 20 % ignored: the loss value only (with ties only the value
    is order-independent), 1e-5 relative as test_lovasz_multitile_ties_value"""
    from model.unet_training import lovasz_hinge_loss
    from oracle import ref_cpu
    B, H, W, levels = 4, 300, 300, 5
    g = torch.Generator().manual_seed(24)
    z = (torch.randint(0, levels, (B, H, W), generator=g).float() - levels // 2) * 0.5
    tgt = (torch.rand(B, H, W, generator=g) < 0.4).long()
    tgt[torch.rand(B, H, W, generator=g) < 0.2] = IGN
    ref = ref_cpu.lovasz_hinge_loss_ignore(z, tgt, IGN)
    loss = lovasz_hinge_loss(z.to(DEV), tgt.to(DEV), ignore_index=IGN)
    print(f"IGNERR lovasz_image ties: rel {abs(loss.item() - ref.item()) / abs(ref.item()):.2e}")
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())


# ------------------------------------------------------------------------------------------------
# flattened masked losses and confusion counts
# ------------------------------------------------------------------------------------------------
FLAT_SIZES = [(3, 2, 37, 50), (9, 2, 512, 512)]


@functools.lru_cache(maxsize=None)
def _flat_inputs(B, H, W):
    """two-channel logits with planted exact o1 == o0 ties; targets 0 / 1 / IGN: image 0 has nothing
    ignored, the last image everything, the others about 25 %"""
    g = torch.Generator().manual_seed(31 + H)
    out = torch.randn(B, 2, H, W, generator=g) * 3
    out[:, 1, :2] = out[:, 0, :2]
    tgt = (torch.rand(B, H, W, generator=g) < 0.3).long()
    ign = torch.rand(B, H, W, generator=g) < 0.25
    ign[0] = False
    ign[B - 1] = True
    tgt[ign] = IGN
    return out, tgt


def _hinge_mean(out, tgt):
    """the reference's lovasz_hinge on the flattened valid pixels, in closed form: its
    lovasz_hinge_loss gets a 1-D tensor and loops over single pixels (model/unet_training.py:267-276,
    oracle/ref_cpu.py lovasz_hinge_loss_ignore), and the Lovasz loss of one pixel is relu(error) x 1"""
    z = out[:, 1] - out[:, 0]
    valid = tgt != IGN
    sign = 2.0 * (tgt[valid] == 1).to(z.dtype) - 1.0
    return torch.relu(1.0 - z[valid] * sign).mean()


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
@pytest.mark.parametrize("B,C,H,W", FLAT_SIZES)
def test_masked_loss_vs_float64(B, C, H, W, kind):
    """(3, 2, 37, 50): the image edge falls inside a block; (9, 2, 512, 512): 2 359 296 pixels, past
    8192 x 256, so masked_loss_kernel and scale_by_kernel take their second grid pass.
    The Lovasz reference at the large size is _hinge_mean: the oracle's per-pixel Python loop over
    1.6 million valid pixels takes minutes; at the small size the oracle itself is the reference and
    _hinge_mean is checked against it (value and gradient, 1e-12)."""
    from oracle import ref_cpu
    from unetseg_hip import losses
    out, tgt = _flat_inputs(B, H, W)
    pw = torch.tensor([1.3]) if kind == "bce" else None
    o64 = out.double().requires_grad_(True)
    if kind == "lovasz_hinge" and B * H * W > 100000:
        ref = _hinge_mean(o64, tgt)
    else:
        ref = ref_cpu.binary_segmentation_loss(o64, tgt, kind, pos_weight=pw.double() if pw is not None else None,
                                               ignore_index=IGN)
    ref.backward()
    if kind == "lovasz_hinge" and B * H * W <= 100000:
        o2 = out.double().requires_grad_(True)
        closed = _hinge_mean(o2, tgt)
        closed.backward()
        assert abs(closed.item() - ref.item()) <= 1e-12 * abs(ref.item())
        assert (o2.grad - o64.grad).abs().max().item() <= 1e-12 * o64.grad.abs().max().item()
    od = out.to(DEV).requires_grad_(True)
    loss = losses.binary_segmentation_loss(od, tgt.to(DEV), kind, pos_weight=pw.to(DEV) if pw is not None else None,
                                           ignore_index=IGN)
    loss.backward()
    gd, gr = od.grad.cpu().double(), o64.grad
    err = (gd - gr).abs().max().item()
    print(f"IGNERR masked {kind} {B}x{H}x{W}: loss rel {abs(loss.item() - ref.item()) / abs(ref.item()):.2e}  "
          f"grad {err / gr.abs().max().item():.2e} of max")
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    assert err <= 1e-5 * gr.abs().max().item(), err
    assert (gd[:, 0][tgt == IGN] == 0).all() and (gd[:, 1][tgt == IGN] == 0).all()


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
def test_masked_loss_all_ignored(kind):
    """every pixel ignored: BCE is a mean over nothing (NaN), the Lovasz branch's empty loss list gives
    logits.sum() * 0 = 0, and the gradient is all zeros in both (masked_finalize_kernel; the reference
    does the same)"""
    from oracle import ref_cpu
    from unetseg_hip import losses
    out, _ = _flat_inputs(3, 37, 50)
    tgt = torch.full((3, 37, 50), IGN, dtype=torch.long)
    o64 = out.double().requires_grad_(True)
    ref = ref_cpu.binary_segmentation_loss(o64, tgt, kind, ignore_index=IGN)
    ref.backward()
    od = out.to(DEV).requires_grad_(True)
    loss = losses.binary_segmentation_loss(od, tgt.to(DEV), kind, ignore_index=IGN)
    loss.backward()
    if kind == "bce":
        assert torch.isnan(ref).item() and torch.isnan(loss).item()
    else:
        assert ref.item() == 0.0 and loss.item() == 0.0
    assert (o64.grad == 0).all() and (od.grad == 0).all()


@pytest.mark.parametrize("B,C,H,W", FLAT_SIZES)
def test_confusion_masked_argmax(B, C, H, W):
    """two-channel mode (argmax, exact tie -> background), two calls into one counter tensor;
    (9, 2, 512, 512) is past the 2048 x 256 grid"""
    from oracle import ref_cpu
    from unetseg_hip import losses
    out, tgt = _flat_inputs(B, H, W)
    assert ((out[:, 1] == out[:, 0]) & (tgt != IGN)).any()
    ref = [int(v) for v in ref_cpu.binary_confusion(out, tgt, ignore_index=IGN)]
    assert sum(ref) == int((tgt != IGN).sum())
    conf = losses.binary_confusion(out.to(DEV), tgt.to(DEV), ignore_index=IGN)
    assert conf.cpu().tolist() == ref
    again = losses.binary_confusion(out.to(DEV), tgt.to(DEV), conf, ignore_index=IGN)
    assert again is conf and conf.cpu().tolist() == [2 * v for v in ref]


@pytest.mark.parametrize("B,C,H,W", FLAT_SIZES)
def test_confusion_masked_sigmoid(B, C, H, W):
    """one-channel mode: pred = sigmoid(z) > 0.5 under the same mask.  Logits are exactly 0
    (sigmoid = 0.5: background) or at least 1e-3 in magnitude (sigmoid differs from 0.5 by 2.5e-4, four
    thousand fp32 ulps), so no pixel sits where two fp32 sigmoids may round differently"""
    from unetseg_hip import losses
    out, tgt = _flat_inputs(B, H, W)
    z = (out[:, 1] - out[:, 0]).unsqueeze(1).clone()
    z[z.abs() < 1e-3] = 0.0
    assert (z == 0).any() and (z[z != 0].abs() >= 1e-3).all()
    valid = tgt != IGN
    pred = (torch.sigmoid(z[:, 0]) > 0.5)[valid]
    t = tgt[valid] == 1
    ref = [int((pred & t).sum()), int((pred & ~t).sum()), int((~pred & t).sum()), int((~pred & ~t).sum())]
    conf = losses.binary_confusion(z.to(DEV), tgt.to(DEV), ignore_index=IGN)
    assert conf.cpu().tolist() == ref
    losses.binary_confusion(z.to(DEV), tgt.to(DEV), conf, ignore_index=IGN)
    assert conf.cpu().tolist() == [2 * v for v in ref]
