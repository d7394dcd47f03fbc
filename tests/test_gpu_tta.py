"""GPU: flip / rotation test-time augmentation (csrc/tta.hip, unetseg_hip/tta.py, --tta of predict.py / val.py).

The reference is tests/tta_ref.py: torch.flip / torch.rot90 for the views (a permutation: compared
bit for bit) and a float64 softmax / mean / log for the merge.

Bound of the merge: |out - ref| <= 1e-5 + 1e-6 |ref|.  An fp32 restatement of the same formula in torch
on the CPU (one exp, one division, at most 8 adds, one division, one log per value) deviates from
float64 on exactly these inputs (logits 8 N(0,1)) by at most 2.0e-6 at K = 8, C = 32, where |ref|
reaches 27, and by 4.1e-6 for a single view, where |ref| reaches 59; its excess over 1e-6 |ref| never
passes 4e-7, so the absolute term leaves a factor of five and more.

Labels: argmax_c out == argmax_c ref wherever the float64 top-two gap exceeds 2e-4, and at most 1 % of
the pixels may be excluded that way, asserted on the reference alone.  That cap holds for the eight-view
sets and the single views (measured on the reference: at most 0.52 % below the gap); with two or four
views of logits this saturated it cannot: wherever two views vote for different classes with
probability ~1 each the mean is a tie to within exp(-|logit gap|), which is 9 % of the pixels at C = 2,
K = 2 whatever the code under test does.  Those cases assert the agreement off the margin and print the
share.

Sizes: 1, 31, 64, 65, 97 lie below, on and past one and two 32-wide tiles, with more than one block
per plane from 64 on; the rectangles have both edges off the tile.
"""
import os

import numpy as np
import pytest
import torch

import tta_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ATOL, RTOL = 1e-5, 1e-6
GAP, MAX_UNSURE = 2e-4, 0.01

D4 = [(n, n, 0xFF) for n in (1, 31, 64, 65, 97)]
RECT = [(37, 70, 0x33), (64, 33, 0x33), (37, 70, 0x03), (64, 33, 0x03)]
SINGLE = [(65, 65, 1 << k) for k in range(8)]
CASES = D4 + RECT + SINGLE


def _id(v):
    return hex(v[2]) + f"-{v[0]}x{v[1]}" if isinstance(v, tuple) else None


def dev_views(x, mask):
    from unetseg_hip import tta

    return tta.views(x, mask)


def dev_merge(lg, mask):
    from unetseg_hip import tta

    return tta.merge(lg, mask)


def check_bound(got, ref, what=""):
    """prints the figures, then asserts the module docstring's bound"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    over = (err - RTOL * ref.abs()).max().item()
    print(f"{what} max |out - ref| {err.max().item():.3e}, max (|out - ref| - 1e-6 |ref|) {over:.3e} "
          f"(bound {ATOL:.0e}), max |ref| {ref.abs().max().item():.1f}")
    assert over <= ATOL


_CACHE = {}


def merged(C, H, W, mask):
    """(kernel output on the CPU, float64 reference) of the seeded case, computed once"""
    key = (C, H, W, mask)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * C + H + mask)
        K = bin(mask).count("1")
        lg = 8 * torch.randn(K * 2, C, H, W, generator=g)
        _CACHE[key] = (dev_merge(lg.to(DEV), mask).cpu(), tta_ref.merge_ref(lg, mask))
    return _CACHE[key]


# ---- 1. views --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_views_bit_exact(case):
    H, W, mask = case
    x = torch.arange(2 * 3 * H * W, dtype=torch.float32).view(2, 3, H, W)  # every element a different value
    got = dev_views(x.to(DEV), mask)
    want = tta_ref.views_ref(x, mask)
    assert got.shape == want.shape == (bin(mask).count("1") * 2, 3, H, W)
    assert torch.equal(got.cpu(), want)


def test_views_of_the_identity_mask_is_a_copy():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 2, 45, 77, generator=g).to(DEV)
    assert torch.equal(dev_views(x, 0x01).view(torch.int32), x.view(torch.int32))


# ---- 2. merge --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 5, 32])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_merge_matches_float64(case, C):
    got, ref = merged(C, *case)
    check_bound(got, ref, f"C={C} {_id(case)}")


@pytest.mark.parametrize("C,H,W,mask", [(5, 65, 65, 0xFF), (2, 37, 70, 0x03), (1, 65, 65, 0xFF), (1, 37, 70, 0x33)])
def test_merge_stable_with_saturated_classes(C, H, W, mask):
    """a quarter of the pixels of every slab have one class at +60 or -60: no inf, no NaN, and the
    bound still holds (the smallest mean probability here is about exp(-75): a normal fp32 number)"""
    g = torch.Generator().manual_seed(77 + C + H)
    N = bin(mask).count("1") * 2
    lg = 8 * torch.randn(N, C, H, W, generator=g)
    hit = torch.rand(N, H, W, generator=g) < 0.25
    cls = torch.randint(0, C, (N, H, W), generator=g)
    val = torch.where(torch.rand(N, H, W, generator=g) < 0.5, -60.0, 60.0)
    sel = torch.zeros_like(lg, dtype=torch.bool).scatter_(1, cls[:, None], hit[:, None])
    lg = torch.where(sel, val[:, None].expand_as(lg), lg)
    assert 0.2 < sel.any(1).float().mean().item() < 0.3
    got = dev_merge(lg.to(DEV), mask)
    assert torch.isfinite(got).all()
    check_bound(got, tta_ref.merge_ref(lg, mask), f"saturated C={C}")


def test_merge_of_extreme_single_channel_logits_is_finite():
    """sigmoid(-z) underflows from z = 104 on: the floor at FLT_MIN keeps the logit finite and its sign"""
    z = torch.tensor([200.0, -200.0, 0.0, 1e4, -1e4, 50.0]).view(1, 1, 1, 6).to(DEV)
    got = dev_merge(z, 0x01).cpu().view(-1)
    assert torch.isfinite(got).all()
    assert got[0] > 80 and got[3] > 80 and got[1] < -80 and got[4] < -80 and got[2] == 0
    assert abs(got[5].item() - 50.0) <= ATOL + RTOL * 50
    # two views that disagree at full saturation (the mirror view's slab, in its own frame, holds -z):
    # the mean is one half, the logit 0
    both = dev_merge(torch.stack([z[0], (-z[0]).flip(-1)]), 0x03).cpu().view(-1)
    assert torch.isfinite(both).all() and both.abs().max().item() < 1e-6


# ---- 3. labels -------------------------------------------------------------------------------------
def _labels_agree(C, case, cap):
    got, ref = merged(C, *case)
    if C == 1:  # the sign of the logit is the label
        gap, same = ref.abs()[:, 0], (got > 0) == (ref > 0)
        same = same[:, 0]
    else:
        top = ref.topk(2, 1).values
        gap, same = top[:, 0] - top[:, 1], got.argmax(1) == ref.argmax(1)
    sure = gap > GAP
    unsure = 1.0 - sure.double().mean().item()
    bad = int((~same[sure]).sum())
    print(f"C={C} {_id(case)}: share at or below the gap {unsure:.4f} (cap {MAX_UNSURE}), mismatches off it {bad}")
    if cap:
        assert unsure <= MAX_UNSURE  # the reference alone
    assert bad == 0


@pytest.mark.parametrize("C", [1, 2, 5, 32])
@pytest.mark.parametrize("case", D4 + SINGLE, ids=_id)
def test_labels_agree(case, C):
    _labels_agree(C, case, cap=True)


@pytest.mark.parametrize("C", [1, 2, 5, 32])
@pytest.mark.parametrize("case", RECT, ids=_id)
def test_labels_agree_off_the_ties_of_two_and_four_views(case, C):
    _labels_agree(C, case, cap=False)


# ---- 4. K = 1 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 5, 32])
def test_merge_of_the_identity_is_log_softmax(C):
    g = torch.Generator().manual_seed(40 + C)
    z = 8 * torch.randn(2, C, 65, 65, generator=g)
    want = z.double() if C == 1 else torch.log_softmax(z.double(), 1)
    check_bound(dev_merge(z.to(DEV), 0x01), want, f"identity C={C}")


@pytest.mark.parametrize("k", [2, 3, 6, 7, 1, 4])
@pytest.mark.parametrize("C", [1, 5])
def test_merge_of_one_turned_view_undoes_that_view(C, k):
    """the inverse of one quarter turn is three: a forward map used for the inverse shows on views 2, 3, 6, 7"""
    g = torch.Generator().manual_seed(50 + C + k)
    z = 8 * torch.randn(2, C, 65, 65, generator=g)  # the identity-frame logits
    slab = tta_ref.view(z, k).contiguous()
    want = z.double() if C == 1 else torch.log_softmax(z.double(), 1)
    check_bound(dev_merge(slab.to(DEV), 1 << k), want, f"view {k} C={C}")


# ---- 5. the wrapper on real models -------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_model():
    from model.model_factory import build_model

    torch.manual_seed(1234)
    return build_model("unet_plain", num_classes=2).to(DEV).eval()


def _image_batch(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, H, W, generator=g).to(DEV)


def test_wrapper_on_unet_plain(plain_model):
    from unetseg_hip.tta import MODES, TTA

    x = _image_batch(5, 2, 64, 64)
    wrapped = TTA(plain_model)
    assert wrapped.mode == "d4" and wrapped.mask == MODES["d4"]
    with torch.no_grad():
        got = wrapped(x)
        xv = tta_ref.views_ref(x, 0xFF)
        assert torch.equal(xv, dev_views(x, 0xFF))
        lg = plain_model(xv)
        check_bound(got, tta_ref.merge_ref(lg, 0xFF), "unet_plain d4")
        assert got.shape == (2, 2, 64, 64) and got.dtype == torch.float32
        # the merged map is a log-probability: its softmax is the mean probability itself
        assert (torch.logsumexp(got.double(), 1).abs() <= 1e-5).all()
        # chunks of the K * B batch, against the same chunks
        chunked = TTA(plain_model, "d4", max_batch=6)(x)
        lg6 = torch.cat([plain_model(xv[i:i + 6]) for i in range(0, 16, 6)])
        check_bound(chunked, tta_ref.merge_ref(lg6, 0xFF), "unet_plain d4 in chunks of 6")
        assert torch.equal(TTA(plain_model, "none")(x), plain_model(x))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            amp = wrapped(x)
            lg_amp = plain_model(xv)
        assert amp.dtype == torch.float32
        check_bound(amp, tta_ref.merge_ref(lg_amp.float(), 0xFF), "unet_plain d4 bf16")


def test_wrapper_is_inference_only(plain_model):
    from unetseg_hip.tta import TTA

    x = _image_batch(6, 1, 64, 64)
    wrapped = TTA(plain_model, "hflip")
    with pytest.raises(RuntimeError, match="no_grad"):
        wrapped(x)
    try:
        wrapped.train()
        assert plain_model.training
        with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
            wrapped(x)
    finally:
        wrapped.eval()  # the evaluation loops call this on the wrapper
    assert not plain_model.training
    with torch.no_grad():
        assert wrapped(x).shape == (1, 2, 64, 64)


def test_wrapper_refuses_quarter_turns_of_a_rectangle(plain_model):
    from unetseg_hip.tta import TTA

    x = _image_batch(7, 1, 64, 96)
    with torch.no_grad():
        with pytest.raises(ValueError, match="H == W"):
            TTA(plain_model, "d4")(x)
        assert TTA(plain_model, "flips")(x).shape == (1, 2, 64, 96)
    with pytest.raises(ValueError, match="unknown TTA mode"):
        TTA(plain_model, "rot90")


def test_wrapper_on_a_multitask_model():
    from model.model_factory import build_model
    from unetseg_hip.tta import TTA

    torch.manual_seed(4321)
    model = build_model("multitask_unet", num_classes=1, num_seg_classes=1, num_cls_classes=3).to(DEV).eval()
    x = _image_batch(8, 2, 64, 64)
    with torch.no_grad():
        out = TTA(model, "d4")(x)
        seg_v, cls_v = model(tta_ref.views_ref(x, 0xFF))
    assert isinstance(out, tuple) and len(out) == 2
    seg, cls = out
    assert seg.shape == (2, 1, 64, 64) and cls.shape == (2, 3)
    assert torch.isfinite(seg).all() and torch.isfinite(cls).all()
    check_bound(seg, tta_ref.merge_ref(seg_v, 0xFF), "multitask seg")
    want_cls = torch.softmax(cls_v.double().cpu().view(8, 2, 3), -1).mean(0).log()
    check_bound(cls, want_cls, "multitask cls")


# ---- 6. a callable whose output depends on the position -------------------------------------------
def test_position_dependent_callable_is_symmetrised():
    from unetseg_hip.tta import TTA

    H, W = 8, 40
    ramp = torch.zeros(1, 2, H, W)
    ramp[:, 0] = 0.3 * (torch.arange(W, dtype=torch.float32) - 7.0)  # not symmetric about the centre column

    def model(x):
        return ramp.to(x.device).expand(x.shape[0], -1, -1, -1)

    x = _image_batch(9, 2, H, W)
    with torch.no_grad():
        got = TTA(model, "hflip")(x)
        plain = TTA(model, "none")(x)
    p = torch.softmax(ramp.double(), 1)
    want = ((p + p.flip(-1)) / 2).log().expand(2, -1, -1, -1)
    check_bound(got, want, "ramp hflip")
    g = got.double().cpu()
    assert ((g - g.flip(-1)).abs() <= 2 * (ATOL + RTOL * g.abs())).all()
    assert torch.equal(plain.cpu(), ramp.expand(2, -1, -1, -1))
    assert (plain - plain.flip(-1)).abs().max().item() > 1.0


# ---- 7. entry points -----------------------------------------------------------------------------------
def test_tiled_prediction_takes_the_wrapper(plain_model):
    import predict
    from augment_data import make_image
    from unetseg_hip.tta import TTA

    image = make_image(np.random.default_rng(2), 150, 100)
    labels = predict.predict_labels_tiled(TTA(plain_model, "flips"), image, DEV, tile=64, overlap=16)
    assert labels.shape == (100, 150) and labels.dtype == np.int32
    assert labels.min() >= 0 and labels.max() <= 1


def test_predict_cli_with_tta(tmp_path):
    import predict
    from augment_data import make_image
    from model.model_factory import build_model
    from PIL import Image

    assert predict.parse_args([]).tta == "none"
    torch.manual_seed(99)
    wpath = tmp_path / "w.pth"
    torch.save(build_model("unet_plain", num_classes=3).state_dict(), wpath)
    path = tmp_path / "a.png"
    make_image(np.random.default_rng(1), 96, 70).save(path)
    base = ["--data_path", str(path), "--weights", str(wpath), "--num-classes", "2", "--model", "unet_plain",
            "--out-dir", str(tmp_path / "run"), "--tta", "d4"]
    for extra in (["--tile", "0"], ["--tile", "64", "--overlap", "16"]):
        saved = predict.predict(predict.parse_args(base + extra))
        assert len(saved) == 1 and os.path.basename(saved[0]) == "a_mask.png"
        out = Image.open(saved[0])
        assert out.size == (96, 70) and out.mode == "RGB"


@pytest.mark.parametrize("task,model", [("binary", "unet_plain"), ("multitask", "multitask_unet")])
def test_val_cli_with_tta(tmp_path, task, model):
    import val
    from model.model_factory import build_model

    torch.manual_seed(17)
    if task == "multitask":
        net = build_model(model, num_classes=1, num_seg_classes=1, num_cls_classes=3)
    else:
        net = build_model(model, num_classes=2)
    wpath = tmp_path / "w.pth"
    torch.save(net.state_dict(), wpath)
    assert val.parse_args([]).tta == "none"
    m = val.val(val.parse_args(["--data-path", "synthetic", "--synthetic-test", "4", "--input-size", "64", "--tta",
                                "hflip", "--task", task, "--model", model, "--weights", str(wpath), "--batch-size",
                                "2", "--loss", "bce"]))
    assert m and all(np.isfinite(v) for v in m.values()), m
    assert 0.0 <= m["IoU"] <= 1.0 and 0.0 <= m["Dice"] <= 1.0
