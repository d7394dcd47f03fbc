"""CPU checks of the Lovasz-softmax feature: the command line, the C ABI's argument checks and
workspace query (no launch, no device), and the float64 restatement the GPU tests compare against
(tests/lovasz_softmax_ref.py) on an example small enough to compute by hand.
"""
import ctypes
import os

import pytest
import torch

from lovasz_softmax_ref import loss_and_grad, lovasz_grad, lovasz_softmax_ref


def _raw():
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built (run __graft_entry__.build())")
    return lib.load()


def test_train_parses_lovasz_softmax():
    import train

    a = train.parse_args(["--task", "multiclass", "--loss", "lovasz_softmax"])
    assert a.loss == "lovasz_softmax" and a.task == "multiclass"
    import val

    assert val.parse_args(["--task", "multiclass", "--loss", "lovasz_softmax"]).loss == "lovasz_softmax"


@pytest.mark.parametrize("task", ["binary", "multitask"])
def test_lovasz_softmax_needs_the_multiclass_task(task, monkeypatch, tmp_path):
    """train() refuses the combination before it touches a device, a dataset or the output folder"""
    import train

    def no_device(*a, **k):
        raise AssertionError("device queried before the argument check")

    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(train, "_datasets", no_device)
    out = tmp_path / "logs"
    with pytest.raises(ValueError, match="lovasz_softmax"):
        train.train(train.parse_args(["--task", task, "--loss", "lovasz_softmax", "--out-dir", str(out)]))
    assert not out.exists()


def test_argument_errors_without_device():
    """every refusal happens before a launch, returns non-zero and names the entry point"""
    raw = _raw()
    B, C, Pn = 2, 5, 100
    need = raw.unetseg_lovasz_softmax_workspace(B, C, Pn, 1)
    p = 4096  # never dereferenced: the checks fail first

    def call(**kw):
        a = dict(out=p, tgt=p, B=B, C=C, P=Pn, ign=C, per_image=1, ws=p, ws_bytes=need, dl=p, loss=p)
        a.update(kw)
        rc = raw.unetseg_lovasz_softmax_fwd(a["out"], a["tgt"], a["B"], a["C"], a["P"], a["ign"], a["per_image"],
                                            a["ws"], a["ws_bytes"], a["dl"], a["loss"], None)
        return rc, raw.unetseg_last_error()

    for kw in (dict(C=1), dict(C=33), dict(loss=None), dict(out=None), dict(tgt=None), dict(ws_bytes=need - 1),
               dict(ws=None), dict(B=1 << 16, P=1 << 15, ws_bytes=1 << 62),  # B * P = 2^31
               dict(B=2, P=(1 << 31), ws_bytes=1 << 62)):
        rc, msg = call(**kw)
        assert rc != 0, kw
        assert b"lovasz_softmax_fwd" in msg, (kw, msg)
    from unetseg_hip import lib

    with pytest.raises(RuntimeError, match="lovasz_softmax_fwd.*C=33"):
        lib.lib.lovasz_softmax_fwd(p, p, B, 33, Pn, 33, 1, p, need, p, p, None)


def test_workspace_monotone_and_covers_the_sort_buffers():
    raw = _raw()
    ws = raw.unetseg_lovasz_softmax_workspace
    for per_image in (1, 0):
        for B, C, Pn in ((1, 2, 1), (2, 5, 4896), (3, 3, 4160), (8, 5, 512 * 512), (1, 32, 1600), (4, 21, 4096)):
            n = ws(B, C, Pn, per_image)
            assert n >= 16 * B * C * Pn
            assert ws(B + 1, C, Pn, per_image) >= n
            assert ws(B, C + 1, Pn, per_image) >= n
            assert ws(B, C, Pn + 1, per_image) >= n
            assert ws(B, C, Pn + 4096, per_image) > n
            # the documented formula
            S, L = (B * C, Pn) if per_image else (C, B * Pn)
            T = (L + 4095) // 4096
            assert n == 16 * B * C * Pn + 4 * S * T * 258 + 8 * S + 256


def test_restatement_on_a_hand_computed_example():
    """One image, four pixels, two classes; labels (1, 1, 0, 0) and p_1 = (0.8, 0.4, 0.3, 0.1).

    Class 1: fg = (1, 1, 0, 0), e = |fg - p_1| = (0.2, 0.6, 0.3, 0.1); sorted 0.6 (fg), 0.3, 0.2 (fg), 0.1;
      G = 2; J = (1 - 1/2, 1 - 1/3, 1 - 0/3, 1 - 0/4) = (1/2, 2/3, 1, 1); g = (1/2, 1/6, 1/3, 0);
      loss_1 = 0.6/2 + 0.3/6 + 0.2/3 = 5/12.
    Class 0: fg = (0, 0, 1, 1), p_0 = (0.2, 0.6, 0.7, 0.9), the same errors; sorted 0.6, 0.3 (fg), 0.2, 0.1 (fg);
      J = (1 - 2/3, 1 - 1/3, 1 - 1/4, 1 - 0/4) = (1/3, 2/3, 3/4, 1); g = (1/3, 1/3, 1/12, 1/4);
      loss_0 = 0.6/3 + 0.3/3 + 0.2/12 + 0.1/4 = 41/120.
    loss = (5/12 + 41/120) / 2 = 91/240.  dL/dp_1 = 1/2 * g_rank * (fg ? -1 : +1) = (-1/6, -1/4, +1/12, 0).
    An ignored fifth pixel, or a second image without a valid pixel, changes neither number (the
    latter halves the per-image mean)."""
    p1 = torch.tensor([0.8, 0.4, 0.3, 0.1], dtype=torch.float64)
    probs = torch.stack([1 - p1, p1])                     # [C, P]
    logits = probs.log().reshape(1, 2, 2, 2)               # softmax(log p) = p
    labels = torch.tensor([1, 1, 0, 0]).reshape(1, 2, 2)
    g = lovasz_grad(torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64))
    assert torch.allclose(g, torch.tensor([1 / 2, 1 / 6, 1 / 3, 0.0], dtype=torch.float64), atol=1e-15)
    for per_image in (True, False):
        loss, grad = loss_and_grad(logits, labels, 2, per_image)
        assert abs(loss - 91 / 240) < 1e-14
        # back to dL/dp_1 - dL/dp_0 through the softmax Jacobian: dlogit_1 = p_1 p_0 (dL/dp_1 - dL/dp_0)
        dp1 = torch.tensor([-1 / 6, -1 / 4, 1 / 12, 0.0], dtype=torch.float64)
        dp0 = 0.5 * torch.tensor([1 / 12, 1 / 3, -1 / 3, -1 / 4], dtype=torch.float64)  # class 0: ranks 3, 1, 2, 4
        want = p1 * (1 - p1) * (dp1 - dp0)
        assert torch.allclose(grad[0, 1].reshape(-1), want, atol=1e-14)
        assert torch.allclose(grad[0, 0].reshape(-1), -want, atol=1e-14)
    # an ignored pixel and an out-of-range label are skipped
    lg5 = torch.cat([logits.reshape(1, 2, 4), torch.tensor([[[0.3], [-1.0]]], dtype=torch.float64)], 2).reshape(1, 2, 1, 5)
    for bad in (2, 7, -1):
        lab5 = torch.tensor([1, 1, 0, 0, bad]).reshape(1, 1, 5)
        loss, grad = loss_and_grad(lg5, lab5, 2, True)
        assert abs(loss - 91 / 240) < 1e-14 and float(grad[..., 4].abs().max()) == 0.0
    # an image without a valid pixel counts as 0 in the per-image mean and vanishes from the batch segment
    lg2 = torch.cat([logits, torch.zeros_like(logits)], 0)
    lab2 = torch.cat([labels, torch.full_like(labels, 2)], 0)
    assert abs(float(lovasz_softmax_ref(lg2, lab2, 2, True)) - 91 / 480) < 1e-14
    assert abs(float(lovasz_softmax_ref(lg2, lab2, 2, False)) - 91 / 240) < 1e-14
    assert float(lovasz_softmax_ref(lg2[1:], lab2[1:], 2, True)) == 0.0


def test_restatement_runs_in_the_requested_dtype():
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(2, 3, 8, 8, generator=g)
    lab = torch.randint(0, 4, (2, 8, 8), generator=g)
    l64, g64 = loss_and_grad(lg, lab, 3, True, torch.float64)
    l32, g32 = loss_and_grad(lg, lab, 3, True, torch.float32)
    assert lovasz_softmax_ref(lg, lab, 3, True, torch.float32).dtype == torch.float32
    assert abs(l32 - l64) < 1e-6 * abs(l64)
    assert float((g32 - g64).abs().max()) < 1e-3 * float(g64.abs().max())
