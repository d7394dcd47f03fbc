"""CPU: the boundary loss's float64 reference (tests/boundary_loss_ref.py) against scipy's exact distance
transform written out as the published one_hot2dist, hand-written maps, the three zero cases and PyTorch
float64 autograd; the C ABI's argument checks and workspace query through ctypes without a device; the
command-line flags and the loss functions' signatures.  No kernel runs here (tests/test_gpu_boundary_loss.py).
"""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import boundary_loss_ref as R

IGN = 255


def _targets(rng, B, H, W, ignore=False):
    t = (rng.random((B, H, W)) < 0.4).astype(np.int64)
    if ignore:
        t[rng.random((B, H, W)) < 0.15] = IGN
    return t


# ---- phi -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (33, 20), (64, 65)])
def test_phi_is_one_hot2dist(H, W):
    """phi == edt(neg) * neg - (edt(pos) - 1) * pos with scipy's exact transform, on images that have both"""
    from scipy.ndimage import distance_transform_edt as edt
    rng = np.random.default_rng(H * 100 + W)
    t = _targets(rng, 3, H, W)
    t[1] = 0
    t[1, H // 3:H // 3 + 2, 1:W - 1] = 1  # a bar: distances well above 1 on both sides
    phi = R.signed_distance(t)
    for b in range(3):
        pos = t[b] == 1
        neg = ~pos
        assert pos.any() and neg.any()
        want = edt(neg) * neg - (edt(pos) - 1) * pos
        np.testing.assert_allclose(phi[b], want, rtol=0, atol=1e-12)


def test_phi_hand_written():
    s2, s5 = math.sqrt(2), math.sqrt(5)
    # 1 x 1: one class only, every distance infinite
    assert R.signed_distance(np.array([[[1]]])).tolist() == [[[0.0]]]
    assert R.signed_distance(np.array([[[0]]])).tolist() == [[[0.0]]]
    # 1 x 5: a run of two
    phi = R.signed_distance(np.array([[[0, 1, 1, 0, 0]]]))
    assert phi.tolist() == [[[1.0, 0.0, 0.0, 1.0, 2.0]]]
    # 1 x 5 with an ignored pixel: it is neither fg nor bg, so the fg pixel beside it looks past it
    phi = R.signed_distance(np.array([[[0, IGN, 1, 1, 1]]]), ignore=IGN)
    assert phi.tolist() == [[[2.0, 0.0, -1.0, -2.0, -3.0]]]
    # 3 x 3: the centre
    phi = R.signed_distance(np.array([[[0, 0, 0], [0, 1, 0], [0, 0, 0]]]))
    np.testing.assert_allclose(phi[0], [[s2, 1, s2], [1, 0, 1], [s2, 1, s2]], rtol=0, atol=1e-15)
    # 3 x 3: a full block with one background corner
    phi = R.signed_distance(np.array([[[0, 1, 1], [1, 1, 1], [1, 1, 1]]]))
    want = [[1, 0, -1], [0, -(s2 - 1), -(s5 - 1)], [-1, -(s5 - 1), -(math.sqrt(8) - 1)]]
    np.testing.assert_allclose(phi[0], want, rtol=0, atol=1e-15)
    # another class value
    phi = R.signed_distance(np.array([[[2, 3, 3, 0, 1]]]), c=3)
    assert phi.tolist() == [[[1.0, 0.0, 0.0, 1.0, 2.0]]]


@pytest.mark.parametrize("nch", [1, 2])
def test_zero_cases(nch):
    """an image without foreground, one without background and an ignored one contribute 0 everywhere; a batch
    of only ignored pixels has L = 0 and gz = 0"""
    rng = np.random.default_rng(5)
    out = 4 * rng.standard_normal((4, nch, 6, 9))
    t = _targets(rng, 4, 6, 9)
    t[1], t[2], t[3] = 0, 1, IGN
    L, gz, phi = R.boundary_loss(out, t, ignore=IGN)
    assert (phi[1:] == 0).all() and (gz[1:] == 0).all() and (phi[0] != 0).any()
    L0, _, _ = R.boundary_loss(out[:1], t[:1], ignore=IGN)
    # the empty images add nothing to the sum and, unless ignored, their pixels to the count
    assert L == pytest.approx(L0 * 54 / (3 * 54), rel=1e-14)
    L, gz, phi = R.boundary_loss(out, np.full((4, 6, 9), IGN), ignore=IGN)
    assert L == 0.0 and not gz.any() and not phi.any()


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("ignore", [None, IGN])
def test_gz_is_autograd(nch, ignore):
    """gz and L against PyTorch float64 autograd of inv_norm * mean over the valid pixels of sigmoid(z) * phi"""
    rng = np.random.default_rng(11 + nch)
    B, H, W = 3, 9, 14
    out = 4 * rng.standard_normal((B, nch, H, W))
    t = _targets(rng, B, H, W, ignore is not None)
    inv = 1.0 / math.sqrt(H * H + W * W)
    L, gz, phi = R.boundary_loss(out, t, ignore=ignore, inv_norm=inv)
    o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    z = o[:, 1] - o[:, 0] if nch == 2 else o[:, 0]
    valid = torch.tensor(np.ones_like(t, bool) if ignore is None else t != ignore)
    ref = inv * (torch.sigmoid(z) * torch.tensor(phi))[valid].mean()
    (gz_t,) = torch.autograd.grad(ref, z)
    assert abs(L - ref.item()) <= 1e-12 * abs(ref.item())
    assert np.abs(gz - gz_t.numpy()).max() <= 1e-12 * np.abs(gz_t.numpy()).max()
    assert (gz[~valid.numpy()] == 0).all()


# ---- the C ABI without a device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw():
    from unetseg_hip import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built (run __graft_entry__.build())")
    return lib.load()


def test_workspace_grows(raw):
    q = raw.unetseg_boundary_loss_workspace
    base = q(2, 64, 64)
    assert base >= 2 * 64 * 64 * 10  # two uint8 site maps and two int32 distance maps
    assert q(3, 64, 64) > base and q(2, 65, 64) > base and q(2, 64, 65) > base
    assert q(16, 512, 512) >= 16 * 512 * 512 * 10


def test_argument_refusals(raw):
    """every refusal returns non-zero with a message before anything is launched (no device here)"""
    f = raw.unetseg_boundary_loss_fwd
    B, H, W = 2, 8, 8
    nb = raw.unetseg_boundary_loss_workspace(B, H, W)
    buf = (ctypes.c_char * (nb + 64))()
    ws = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.addressof((ctypes.c_char * 4096)())  # stands for out / tgt / loss: never dereferenced on a refusal
    ok = dict(out=p, nch=2, tgt=p, B=B, H=H, W=W, c=1, ign=-1, inv=1.0, w=1.0, ws=ws, nb=nb, gz=None, acc=0, phi=None,
              loss=p)

    def refused(match, **kw):
        a = dict(ok, **kw)
        rc = f(a["out"], a["nch"], a["tgt"], a["B"], a["H"], a["W"], a["c"], a["ign"], a["inv"], a["w"], a["ws"],
               a["nb"], a["gz"], a["acc"], a["phi"], a["loss"], None)
        msg = raw.unetseg_last_error().decode()
        assert rc != 0 and "boundary_loss_fwd" in msg and match in msg, (kw, rc, msg)

    for name in ("out", "tgt", "ws", "loss"):
        refused("null", **{name: None})
    for nch in (0, 3):
        refused("nch", nch=nch)
    for name in ("B", "H", "W"):
        refused("shape", **{name: 0})
        refused("shape", **{name: -1})
    refused("exceed", H=16385)
    refused("exceed", W=16385)
    refused("ignore_index", ign=1)
    refused("ignore_index", c=7, ign=7)
    refused("workspace too small", nb=nb - 1)
    refused("aligned", ws=ws + 4)
    # the op layer's wrapper raises with the same message
    from unetseg_hip import lib
    with pytest.raises(RuntimeError, match="boundary_loss_fwd.*nch"):
        lib.lib.boundary_loss_fwd(p, 5, p, B, H, W, 1, -1, 1.0, 1.0, ws, nb, None, 0, None, p, None)
    assert raw.unetseg_abi_version() == 1


def test_workspace_query_is_host_only_for_plans():
    from unetseg_hip import plan
    assert "boundary_loss_workspace" in plan._PURE


# ---- Python surface ---------------------------------------------------------------------------------------------
def test_signatures():
    from model.unet_multitask import MultiTaskLoss
    from unetseg_hip import losses
    from utils import train_and_eval as te
    for fn in (losses.binary_segmentation_loss, losses.multitask_loss, MultiTaskLoss.__init__, te.evaluate_binary,
               te.train_one_epoch_binary, te.binary_segmentation_loss):
        p = inspect.signature(fn).parameters
        assert p["boundary_weight"].default == 0.0 and p["boundary_normalize"].default is True, fn
    p = inspect.signature(losses.boundary_loss).parameters
    assert [p[k].default for k in ("c", "ignore_index", "normalize")] == [1, None, True]
    p = inspect.signature(losses.signed_distance).parameters
    assert [p[k].default for k in ("c", "ignore_index")] == [1, None]
    with pytest.raises(ValueError, match="boundary_weight"):
        losses.binary_segmentation_loss(torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 2), "bce", boundary_weight=-1.0)


def test_flags(capsys):
    import train
    import val
    for mod in (train, val):
        a = mod.parse_args([])
        assert a.boundary_loss_weight == 0.0 and a.boundary_loss_pixels is False
        for task in ("binary", "multitask"):
            a = mod.parse_args(["--task", task, "--boundary-loss-weight", "0.01", "--boundary-loss-pixels"])
            assert a.boundary_loss_weight == 0.01 and a.boundary_loss_pixels is True
        for extra in (["--boundary-loss-weight", "0.01"], ["--boundary-loss-pixels"]):
            with pytest.raises(SystemExit):
                mod.parse_args(["--task", "multiclass"] + extra)
            assert "binary and multitask only" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(["--boundary-loss-weight", "-0.5"])
        capsys.readouterr()
        assert mod.parse_args(["--task", "multiclass"]).boundary_loss_weight == 0.0
