"""CPU: the soft skeleton / soft-clDice float64 reference (tests/cldice_ref.py) against PyTorch float64 autograd of
the published soft_skel / soft_cldice (clDice, Shit et al., CVPR 2021), written with F.max_pool2d, hand-written maps
and the stated tie rule; the conditions the GPU comparisons of tests/test_gpu_cldice.py rest on, for the very
inputs they use; the C ABI's argument checks through ctypes without a device; the flags and the signatures.  No
kernel runs here.

The condition "no window of any x_j holds two equal values at distinct pixels" is asserted on the input pixels the
values come from: every x_j is a selection of values of x_0, and with pairwise distinct x_0 two equal entries of a
window of x_j (j >= 1 has them everywhere: a local minimum spreads to its neighbours) are the same input pixel, so
whichever the tie rule picks, the gradient ends at that pixel.  The autograd comparison below holds that reading
to PyTorch, which splits such ties.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cldice_cases as C
import cldice_ref as R


# ---- the published code -----------------------------------------------------------------------------------
def _soft_erode(img):
    p1 = -F.max_pool2d(-img, (3, 1), (1, 1), (1, 0))
    p2 = -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1))
    return torch.min(p1, p2)


def _soft_dilate(img):
    return F.max_pool2d(img, (3, 3), (1, 1), (1, 1))


def _soft_open(img):
    return _soft_dilate(_soft_erode(img))


def _soft_skel(img, iter_):
    img1 = _soft_open(img)
    skel = F.relu(img - img1)
    for _ in range(iter_):
        img = _soft_erode(img)
        img1 = _soft_open(img)
        delta = F.relu(img - img1)
        skel = skel + F.relu(delta - skel * delta)
    return skel


def _soft_cldice(y_true, y_pred, iter_, smooth):
    skel_pred = _soft_skel(y_pred, iter_)
    skel_true = _soft_skel(y_true, iter_)
    tprec = (torch.sum(skel_pred * y_true) + smooth) / (torch.sum(skel_pred) + smooth)
    tsens = (torch.sum(skel_true * y_pred) + smooth) / (torch.sum(skel_true) + smooth)
    return 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)


@pytest.mark.parametrize("shape,iters", C.SKEL_CASES)
def test_skeleton_reference_is_published_autograd(shape, iters):
    case = C.skel_case(shape, iters)
    x = torch.tensor(case["x"], dtype=torch.float64).unsqueeze(1).requires_grad_(True)
    s = _soft_skel(x, iters)
    (s * torch.tensor(case["g"], dtype=torch.float64).unsqueeze(1)).sum().backward()
    np.testing.assert_allclose(case["skel"], s.detach().numpy()[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(case["gx"], x.grad.numpy()[:, 0], rtol=0, atol=1e-12)
    assert (case["A"] >= np.abs(case["gx"]) - 1e-12).all()


@pytest.mark.parametrize("case", C.LOSS_CASES)
def test_loss_reference_is_published_autograd(case):
    c = C.loss_case(*case)
    z = torch.tensor(R.logit(c["out"]), dtype=torch.float64).requires_grad_(True)
    valid = torch.tensor(c["t"] != c["ign"]) if c["ign"] is not None else torch.ones(c["t"].shape, dtype=torch.bool)
    p = (torch.sigmoid(z) * valid).unsqueeze(1)
    y = torch.tensor((c["t"] == 1).astype(np.float64)).unsqueeze(1)
    L = _soft_cldice(y, p, c["iters"], 1.0)
    L.backward()
    assert abs(L.item() - c["L"]) <= 1e-12
    np.testing.assert_allclose(c["gz"], z.grad.numpy(), rtol=0, atol=1e-12)
    assert np.isfinite(c["L"]) and (c["gz_bound"] >= 0).all() and c["L_bound"] < 1e-4
    if c["kind"] == "ignored":
        assert c["L"] == 0.0 and not c["gz"].any()


# ---- the conditions of the GPU comparisons ------------------------------------------------------------------
@pytest.mark.parametrize("shape,iters", C.SKEL_CASES)
def test_skeleton_case_conditions(shape, iters):
    case = C.skel_case(shape, iters)
    assert case["x"].dtype == np.float32 and (case["x"] > 0).all() and (case["x"] < 1).all()
    assert R.distinct_inputs(case["x"])
    a = R.relu_arguments(case["levels"])
    assert not ((a > 0) & (a < 2.0 ** -18)).any()
    assert R.selection_margin(case["levels"]) > 0
    assert C.conditions_hold(case["levels"], case["x"])


@pytest.mark.parametrize("case", C.LOSS_CASES)
def test_loss_case_conditions(case):
    c = C.loss_case(*case)
    assert np.abs(R.logit(c["out"])).max() <= 6.0
    a = R.relu_arguments(c["levels"])
    assert not ((a > 0) & (a < 2.0 ** -18)).any()
    for img in c["p"]:  # ignored pixels are 0 and take no gradient; every other value once per image
        nz = img[img != 0]
        assert np.unique(nz).size == nz.size
    assert R.selection_margin(c["levels"]) > C.LOSS_MARGIN


# ---- hand-written maps --------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 3, 7])
def test_hand_written_skeletons(iters):
    line = np.zeros((1, 7, 9))
    line[0, 3, :] = 1.0  # one pixel wide: its erosion is empty, so it is its own skeleton
    assert np.array_equal(R.soft_skeleton(line, iters), line)
    col = np.zeros((1, 9, 5))
    col[0, 2:, 1] = 0.75
    assert np.array_equal(R.soft_skeleton(col, iters), col)
    const = np.full((2, 6, 5), 0.625)
    assert not R.soft_skeleton(const, iters).any()
    assert R.soft_skeleton(np.array([[[0.3]]]), iters).tolist() == [[[0.0]]]
    gx, A = R.skeleton_backward(R.skeleton_levels(np.array([[[0.3]]]), iters), np.ones((1, 1, 1)))
    assert gx.tolist() == [[[0.0]]] and A.tolist() == [[[0.0]]]


def test_hand_written_bar():
    """a bar three pixels wide: one erosion leaves its centre line, which the second level adds"""
    x = np.zeros((1, 7, 11))
    x[0, 2:5, :] = 1.0
    assert not R.soft_skeleton(x, 0).any()  # E keeps the centre row, D grows it back over the bar: x - O = 0
    want = np.zeros_like(x)
    want[0, 3, :] = 1.0
    assert np.array_equal(R.soft_skeleton(x, 1), want)
    assert np.array_equal(R.soft_skeleton(x, 3), want)


def test_tie_rule():
    """equal neighbours, exactly representable: the first element in window order takes the whole gradient"""
    x = np.full((1, 3, 3), 0.5)
    x[0, 1, 1] = 1.0
    e, sel_e = R.erode(x)
    assert (e == 0.5).all()
    # E, order up, left, centre, right, down, clipped: the corner's first in-image element is its centre (2); the
    # centre pixel's minimum 0.5 is first met at `up` (0); the top middle's at `left` (1)
    assert sel_e[0, 0, 0] == 2 and sel_e[0, 1, 1] == 0 and sel_e[0, 0, 1] == 1 and sel_e[0, 2, 2] == 0
    o, sel_d = R.dilate(e)
    # D, row-major: all equal, so the first in-image element: the top-left of the window
    assert sel_d[0, 1, 1] == 0 and sel_d[0, 0, 0] == 4 and sel_d[0, 0, 1] == 3 and sel_d[0, 1, 0] == 1
    lv = R.skeleton_levels(x, 0)
    assert R.soft_skeleton(x, 0).tolist() == [[[0, 0, 0], [0, 0.5, 0], [0, 0, 0]]]
    gx, A = R.skeleton_backward(lv, np.full((1, 3, 3), 2.0))
    # s = x - O at the centre only: +2 there; -2 to O(centre) -> e(0, 0) (first of the 3 x 3) -> x(0, 0) (its centre)
    assert gx.tolist() == [[[-2, 0, 0], [0, 2, 0], [0, 0, 0]]]
    assert A.tolist() == [[[2, 0, 0], [0, 2, 0], [0, 0, 0]]]
    # one more level: x_1 = 0.5 everywhere adds nothing; the chain factor 1 - d_1 = 1
    gx1, _ = R.skeleton_backward(R.skeleton_levels(x, 1), np.full((1, 3, 3), 2.0))
    assert gx1.tolist() == gx.tolist()


# ---- the C ABI without a device -----------------------------------------------------------------------------
def _cdll():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "..", "unet-embroidery-seg_amd", "unetseg_hip", "libunetseg_hip.so")
    if not os.path.exists(path):
        pytest.skip("library not built")
    lib = ctypes.CDLL(path)
    for n in ("unetseg_soft_skel_workspace", "unetseg_cldice_workspace"):
        getattr(lib, n).restype = ctypes.c_size_t
        getattr(lib, n).argtypes = [ctypes.c_int] * 4
    vp, i, f, sz, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_long
    lib.unetseg_soft_skel_fwd.argtypes = [vp, i, i, i, i, vp, sz, vp, vp]
    lib.unetseg_soft_skel_bwd.argtypes = [vp, i, i, i, i, vp, sz, vp, vp, vp]
    lib.unetseg_cldice_fwd.argtypes = [vp, i, vp, i, i, i, lg, i, f, f, vp, sz, vp, i, vp, vp]
    return lib


def test_workspace_queries():
    lib = _cdll()
    up = lambda n: (n + 255) // 256 * 256
    for N, H, W, k in [(1, 1, 1, 0), (2, 5, 9, 3), (16, 512, 512, 3), (3, 13, 66, 64)]:
        m = up(4 * N * H * W)
        assert lib.unetseg_soft_skel_workspace(N, H, W, k) == (2 * k + 4) * m
        assert lib.unetseg_cldice_workspace(N, H, W, k) == (2 * k + 10) * m + up(4 * 2048 * 8) + 256
    for bad in [(0, 4, 4, 3), (1, 0, 4, 3), (1, 4, -1, 3), (1, 4, 4, -1), (1, 4, 4, 65)]:
        assert lib.unetseg_soft_skel_workspace(*bad) == 0 and lib.unetseg_cldice_workspace(*bad) == 0


def test_argument_checks_launch_nothing():
    """every refusal comes before the first launch: no device is needed to be refused"""
    lib = _cdll()
    A = 1 << 20  # a 16-byte aligned non-null "pointer"; never dereferenced
    big = 1 << 40
    ok = dict(x=A, N=2, H=5, W=9, k=3, ws=A, nb=big, o=A, g=A)

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.unetseg_soft_skel_fwd(a["x"], a["N"], a["H"], a["W"], a["k"], a["ws"], a["nb"], a["o"], None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.unetseg_soft_skel_bwd(a["x"], a["N"], a["H"], a["W"], a["k"], a["ws"], a["nb"], a["g"], a["o"], None)

    for f in (fwd, bwd):
        for kw in (dict(x=None), dict(ws=None), dict(o=None), dict(N=0), dict(H=0), dict(W=-3), dict(k=-1), dict(k=65),
                   dict(nb=lib.unetseg_soft_skel_workspace(2, 5, 9, 3) - 1), dict(ws=A + 8)):
            assert f(**kw) == 1, kw
    assert bwd(g=None) == 1

    def cl(out=A, nch=2, tgt=A, B=2, H=5, W=9, ign=-1, k=3, smooth=1.0, ws=A, nb=big, gz=A, loss=A):
        return lib.unetseg_cldice_fwd(out, nch, tgt, B, H, W, ign, k, smooth, 0.5, ws, nb, gz, 0, loss, None)

    for kw in (dict(out=None), dict(tgt=None), dict(ws=None), dict(loss=None), dict(nch=0), dict(nch=3), dict(B=0),
               dict(H=-1), dict(W=0), dict(k=-1), dict(k=65), dict(smooth=0.0), dict(smooth=-1.0), dict(ign=1),
               dict(nb=lib.unetseg_cldice_workspace(2, 5, 9, 3) - 1), dict(ws=A + 4)):
        assert cl(**kw) == 1, kw


# ---- flags and signatures -----------------------------------------------------------------------------------
def test_flags():
    import train
    import val
    for mod in (train, val):
        a = mod.parse_args([])
        assert a.cldice_weight == 0.0 and a.cldice_iters == 3
        a = mod.parse_args(["--task", "binary", "--cldice-weight", "0.25", "--cldice-iters", "5"])
        assert a.cldice_weight == 0.25 and a.cldice_iters == 5
        a = mod.parse_args(["--task", "multitask", "--cldice-weight", "0.5", "--cldice-iters", "0"])
        assert a.cldice_weight == 0.5 and a.cldice_iters == 0
        for bad in (["--cldice-weight", "-0.1"], ["--cldice-iters", "-1"], ["--cldice-iters", "65"],
                    ["--task", "multiclass", "--cldice-weight", "0.1"], ["--task", "multiclass", "--cldice-iters", "2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(bad)
        assert mod.parse_args(["--task", "multiclass"]).cldice_weight == 0.0


def test_signatures():
    from model.unet_multitask import MultiTaskLoss
    from unetseg_hip import losses
    from utils import train_and_eval as te
    for fn in (losses.binary_segmentation_loss, losses.multitask_loss, MultiTaskLoss.__init__, te.binary_segmentation_loss,
               te.train_one_epoch_binary, te.evaluate_binary):
        names = list(inspect.signature(fn).parameters)
        ps = inspect.signature(fn).parameters
        assert names[-2:] == ["cldice_weight", "cldice_iters"], fn  # appended: every positional call stays
        assert ps["cldice_weight"].default == 0.0 and ps["cldice_iters"].default == 3
        assert ps["boundary_weight"].default == 0.0 and ps["boundary_normalize"].default is True
    ps = inspect.signature(losses.cldice_loss).parameters
    assert list(ps) == ["outputs", "targets", "iters", "smooth", "ignore_index"]
    assert (ps["iters"].default, ps["smooth"].default, ps["ignore_index"].default) == (3, 1.0, None)
    ps = inspect.signature(losses.soft_skeleton).parameters
    assert list(ps) == ["x", "iters"] and ps["iters"].default == 3
    m = MultiTaskLoss(cldice_weight=0.25, cldice_iters=2)
    assert (m.cldice_weight, m.cldice_iters) == (0.25, 2)
    x = torch.zeros(1, 2, 4, 4)
    for kw in (dict(cldice_weight=-1.0), dict(cldice_weight=float("nan")), dict(cldice_weight=0.5, cldice_iters=65),
               dict(cldice_iters=-1)):
        with pytest.raises(ValueError):
            losses.binary_segmentation_loss(x, torch.zeros(1, 4, 4), "bce", **kw)
    from unetseg_hip import plan
    assert {"soft_skel_workspace", "cldice_workspace"} <= plan._PURE
