"""GPU: the score histogram kernel (csrc/curve.hip) and what is built on it (unetseg_hip/curve.py, the
``curve=`` option of the evaluate loops, ``val.py --curve-metrics``).

Every histogram comparison is exact integer equality with tests/curve_ref.py, which holds the same edge array
and forms the score with the same fp32 subtraction.  The shapes are the smallest at which the kernel can go
wrong: an odd pixel count per image (unaligned image and channel bases, the group loads' element path and a
group that spans two images), one pixel, more blocks than one with a remainder, and an empty batch; K = 2 (one
edge: no middle bin), 1000 (the default; not a power of two) and 4096 (the largest).
"""
import contextlib
import csv
import io
import json
import os

import numpy as np
import pytest
import torch

import curve_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(3, 37, 53), (1, 1, 1), (2, 257, 263)]
KS = [2, 1000, 4096]
FMAX = np.finfo(np.float32).max


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _c():
    from unetseg_hip import curve
    return curve


def _edges(K):
    return _c().edges(K).numpy()


def _targets(g, shape, ignore=None):
    """int64 {0, 1} with some 2 and 7 (negatives), and ``ignore`` on a third of the pixels"""
    t = (g.random(shape) < 0.3).astype(np.int64)
    other = g.random(shape)
    t[other < 0.05] = 2
    t[other > 0.96] = 7
    if ignore is not None:
        t[g.random(shape) < 1 / 3] = ignore
    return t


def _z_cases(g, n, K):
    """name -> fp32 [n] scores"""
    e = _edges(K)
    on = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
    tiled = np.resize(on, n) if n >= len(on) else g.choice(on, n, replace=False)
    g.shuffle(tiled)
    special = (g.standard_normal(n) * 3).astype(np.float32)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FMAX, -FMAX], np.float32)
    where = g.random(n) < 0.2
    special[where] = g.choice(vals, int(where.sum()))
    mix = np.where(g.random(n) < 0.05, np.float32(30), np.float32(-30)).astype(np.float32)
    return {"normal": (g.standard_normal(n) * 3).astype(np.float32), "edges": tiled.astype(np.float32),
            "special": special, "all_low": np.full(n, -30, np.float32), "all_high": np.full(n, 30, np.float32),
            "mix": mix}


def _outputs(g, z, shape, nch, name):
    """planar logits [B, nch, H, W] whose score is z (nch 2: o0 = 0, so that o1 - o0 is z exactly, except for the
    kinds that exercise the subtraction)"""
    B, H, W = shape
    z = z.reshape(B, 1, H, W)
    if nch == 1:
        return z.copy()
    o0 = np.zeros_like(z)
    if name == "special":  # specials on either side: inf - inf, FLT_MAX - (-FLT_MAX), x - NaN
        o0 = np.roll(z, 1, axis=-1).copy() if z.size > 1 else np.full_like(z, np.inf)
    return np.concatenate([o0, z], 1)


def _check(out, tgt, K, ignore=None, targets=None):
    c = _c()
    t = tgt if targets is None else targets
    got = c.hist(torch.from_numpy(out).to(DEV), torch.from_numpy(t).to(DEV), K, ignore)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, K) and got.is_cuda
    want = curve_ref.hist(out, t, _edges(K), ignore)
    assert np.array_equal(got.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hist_exact(shape, nch, K):
    g = np.random.default_rng(hash((shape, nch, K)) % (1 << 32))
    n = int(np.prod(shape))
    for ignore in (None, 255):
        tgt = _targets(g, shape, ignore)
        for name, z in _z_cases(g, n, K).items():
            out = _outputs(g, z, shape, nch, name)
            want = _check(out, tgt, K, ignore)
            valid = n if ignore is None else int((tgt != ignore).sum())
            assert want.sum() == valid, name
            if name == "all_low":
                assert want[:, 1:].sum() == 0
            if name == "all_high":
                assert want[:, :-1].sum() == 0
            if name == "edges" and n >= 3 * (K - 1) and ignore is None:  # every edge was hit from below, on and above
                assert (want.sum(0) > 0).all()


@pytest.mark.parametrize("K", KS)
def test_hist_difference_rounds(K):
    """two-channel pairs whose fp32 difference rounds: channels of different and of very different size"""
    g = np.random.default_rng(11)
    shape = (3, 37, 53)
    tgt = _targets(g, shape)
    B, H, W = shape
    close = np.concatenate([(g.standard_normal((B, 1, H, W)) * 30).astype(np.float32),
                            (g.standard_normal((B, 1, H, W)) * 3).astype(np.float32)], 1)
    far = np.concatenate([(g.standard_normal((B, 1, H, W)) * 3e-3).astype(np.float32),
                          (g.standard_normal((B, 1, H, W)) * 3).astype(np.float32)], 1)
    for out in (close, far):
        d64 = out[:, 1].astype(np.float64) - out[:, 0].astype(np.float64)
        assert (d64 != (out[:, 1] - out[:, 0]).astype(np.float64)).mean() > 0.25  # the case does round
        _check(out, tgt, K)


def test_hist_empty_and_all_ignored():
    c = _c()
    K = 1000
    g = np.random.default_rng(12)
    seed = torch.arange(2 * K, dtype=torch.int64, device=DEV).view(2, K).contiguous()
    for nch in (1, 2):
        out = seed.clone()
        r = c.hist(torch.zeros(0, nch, 37, 53, device=DEV), torch.zeros(0, 37, 53, dtype=torch.int64, device=DEV), K,
                   out=out)
        assert r is out and torch.equal(out, seed)  # B = 0: unchanged
        assert int(c.hist(torch.zeros(0, nch, 4, 4, device=DEV), torch.zeros(0, 4, 4, device=DEV), K).sum()) == 0
        logits = torch.from_numpy((g.standard_normal((2, nch, 37, 53)) * 3).astype(np.float32)).to(DEV)
        c.hist(logits, torch.full((2, 37, 53), 255, dtype=torch.int64, device=DEV), K, 255, out)
        assert torch.equal(out, seed)  # every pixel ignored: unchanged


@pytest.mark.parametrize("nch", [1, 2])
def test_hist_float_targets(nch):
    """float targets are read as losses._prep reads them: class 1 where equal to 1, ignore_index kept"""
    g = np.random.default_rng(13)
    shape = (3, 37, 53)
    out = (g.standard_normal((3, nch, 37, 53)) * 3).astype(np.float32)
    t = _targets(g, shape, 255).astype(np.float32)
    t[g.random(shape) < 0.1] = 0.5  # neither 0 nor 1: a negative
    for ignore in (None, 255):
        want = _check(out, t, 1000, ignore)
        assert want[1].sum() == (t == 1).sum()
    _check(out, t.reshape(3, 1, 37, 53), 1000, 255)  # [B,1,H,W] targets


def test_hist_accumulates_and_replays():
    c = _c()
    g = np.random.default_rng(14)
    K = 1000
    shape = (2, 257, 263)
    out = torch.from_numpy((g.standard_normal((2, 2, 257, 263)) * 3).astype(np.float32)).to(DEV)
    tgt = torch.from_numpy(_targets(g, shape, 255)).to(DEV)
    one = c.hist(out, tgt, K, 255)
    again = c.hist(out, tgt, K, 255)
    assert torch.equal(one, again)  # two fresh runs are bit-equal
    acc = c.hist(out, tgt, K, 255)
    assert c.hist(out, tgt, K, 255, out=acc) is acc and torch.equal(acc, 2 * one)
    seed = torch.arange(2 * K, dtype=torch.int64, device=DEV).view(2, K) * 1_000_000_007  # past 32 bits
    start = seed.clone()
    c.hist(out, tgt, K, 255, out=start)
    assert torch.equal(start, seed + one)
    for bad in (torch.zeros(2, K + 2, dtype=torch.int64, device=DEV), torch.zeros(2, K, dtype=torch.int32, device=DEV),
                torch.zeros(K, 2, dtype=torch.int64, device=DEV).t(), torch.zeros(2, K, dtype=torch.int64)):
        with pytest.raises(ValueError, match="out must be"):
            c.hist(out, tgt, K, 255, out=bad)
    with pytest.raises(ValueError, match="K must be even"):
        c.hist(out, tgt, 999)
    with pytest.raises(ValueError, match="ignore_index -1"):
        c.hist(out, tgt, K, -1)


def test_unsorted_edges_stay_inside_hist():
    """the C ABI with an edge array that is not ascending (shuffled, with NaN and inf): the bins are unspecified, but
    every valid pixel is counted inside hist and the words around it are untouched"""
    from unetseg_hip.lib import lib

    g = np.random.default_rng(15)
    B, nch, P = 3, 2, 37 * 53
    out = torch.from_numpy((g.standard_normal((B, nch, P)) * 3).astype(np.float32)).to(DEV)
    tgt_np = _targets(g, (B, P), 255)
    tgt = torch.from_numpy(tgt_np).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for K in (2, 1000, 4096):
        e = _edges(K).copy()
        g.shuffle(e)
        if K > 2:
            e[[0, K // 3, K - 2]] = [np.nan, np.inf, -np.inf]
        edges = torch.from_numpy(e).to(DEV)
        guard = 4096
        buf = torch.full((guard + 2 * K + guard,), -7, dtype=torch.int64, device=DEV)
        buf[guard:guard + 2 * K] = 0
        lib.curve_hist(out.data_ptr(), nch, tgt.data_ptr(), B, P, 255, edges.data_ptr(), K,
                       buf[guard:].data_ptr(), stream)
        h = buf.cpu().numpy()
        assert (h[:guard] == -7).all() and (h[guard + 2 * K:] == -7).all()
        rows = h[guard:guard + 2 * K].reshape(2, K)
        assert (rows >= 0).all()
        assert rows[1].sum() == (tgt_np == 1).sum() and rows[0].sum() == ((tgt_np != 1) & (tgt_np != 255)).sum()


@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("nch", [1, 2])
def test_table_at_half_equals_binary_confusion(nch, ignore):
    """on logits that are multiples of 1/64 the one-channel confusion kernel's expf rule and z > 0 agree, and the
    two-channel difference is exact: row K / 2 of the table is binary_confusion's (tp, fp, fn, tn)"""
    from unetseg_hip import losses

    c = _c()
    g = np.random.default_rng(16 + nch)
    shape = (3, 37, 53)
    out = (np.round(g.standard_normal((3, nch, 37, 53)) * 3 * 64) / 64).astype(np.float32)
    z = curve_ref.z_of(out)
    assert (z == 0).any() and (z > 0).any() and (z < 0).any()  # the tie is in the case
    tgt = _targets(g, shape, ignore)
    o, t = torch.from_numpy(out).to(DEV), torch.from_numpy(tgt).to(DEV)
    for K in (2, 1000):
        rows = c.table(c.hist(o, t, K, ignore))
        conf = losses.binary_confusion(o, t, None, ignore).tolist()
        assert list(rows[K // 2][1:]) == conf
        pred = c.labels_at(o, 0.5, K)
        from unetseg_hip.boundary import labels_from_logits
        assert torch.equal(pred, labels_from_logits(o))
    k = 371
    b, y = curve_ref.scores(out, tgt, _edges(1000), ignore)
    assert c.table(c.hist(o, t, 1000, ignore))[k][1:] == curve_ref.confusion_at(b, y, k)
    lab = c.labels_at(o, k / 1000).cpu().numpy().reshape(-1)  # the same rule on the device, in torch ops
    assert np.array_equal(lab, (curve_ref.bins_of(z, _edges(1000)) >= k).astype(np.int32))


class Tiny(torch.nn.Module):
    """a small real model whose k-th answer also carries the k-th prior, so that its scores say something"""

    def __init__(self, net, priors):
        super().__init__()
        self.net, self.priors, self.k = net, priors, 0

    def forward(self, x):
        out = self.net(x) + self.priors[self.k]
        self.k += 1
        return out


def test_accumulator_and_evaluate_binary():
    from model.model_factory import build_model
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_binary

    c = _c()
    K = 1000
    torch.manual_seed(5)
    net = build_model("unet_plain", num_classes=2).to(DEV).eval()
    batches, priors = [], []
    for k in range(2):
        x, y = make_batch(2, 64, seed=170 + k)
        near = torch.from_numpy(np.stack([np.roll(m, (1, 2), (0, 1)) for m in y.numpy()])).float()
        prior = torch.zeros(2, 2, 64, 64)
        prior[:, 1] = 3.0 * (near - 0.3)
        batches.append((x, y, None))
        priors.append(prior.to(DEV))
    want = np.zeros((2, K), np.int64)
    acc = c.Accumulator({"bins": K, "threshold": 0.4})
    with torch.no_grad():
        model = Tiny(net, priors)
        for x, y, _ in batches:
            logits = model(x.to(DEV))
            acc.add(logits, y.to(DEV))
            want += curve_ref.hist(logits.cpu().numpy(), y.numpy(), _edges(K))
    assert np.array_equal(acc.out.cpu().numpy(), want) and want.sum() == 4 * 64 * 64
    want_m = c.metrics_from_counts(want, 10, 0.4)
    assert acc.metrics() == want_m and acc.table() == c.table(want)
    b, y_ = curve_ref.expand(want)
    brute = curve_ref.metrics(b, y_, K, 10, 400)
    assert all(abs(want_m[k] - brute[k]) <= 1e-12 for k in brute) and set(brute) == set(want_m)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None)
        none = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, curve=None)
        met = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, curve={"bins": K, "threshold": 0.4})
        dflt = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, curve={})
        both = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, curve={"bins": K}, skeleton={},
                               boundary={"tolerance": 2.0, "biou_d": None})
    assert set(plain) == {"Dice", "IoU", "Precision", "Recall", "Accuracy", "Loss"} and none == plain
    assert set(met) == set(plain) | set(c.KEYS) | set(c.KEYS_AT)
    assert {k: met[k] for k in plain} == plain  # the existing keys are bit-identical
    assert {k: met[k] for k in c.KEYS + c.KEYS_AT} == want_m
    assert {k: dflt[k] for k in c.KEYS} == {k: want_m[k] for k in c.KEYS} and set(dflt) == set(plain) | set(c.KEYS)
    assert {k: both[k] for k in c.KEYS} == {k: want_m[k] for k in c.KEYS} and "clDice" in both and "HD95" in both
    assert {k: both[k] for k in plain} == plain
    assert list(met)[:len(plain)] == list(plain)  # the new keys come after the existing ones
    # IoU@0.5 is the confusion kernel's IoU without its eps
    tp, fp, fn, _ = c.table(want)[K // 2][1:]
    assert met["IoU@0.5"] == tp / (tp + fp + fn) and abs(met["IoU@0.5"] - plain["IoU"]) < 1e-6
    assert 0.0 < met["Best IoU"] < 1.0 and met["Best IoU"] >= met["IoU@0.5"] and 0.5 < met["AUROC"] < 1.0
    with pytest.raises(ValueError, match="unknown curve options"):
        evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, curve={"K": 10})


def test_evaluate_multitask_takes_the_option():
    from model.unet_multitask import MultiTaskLoss
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_multitask

    c = _c()

    class Fixed(torch.nn.Module):
        def __init__(self, outs):
            super().__init__()
            self.outs, self.k = outs, 0

        def forward(self, x):
            self.k += 1
            return self.outs[self.k - 1]

    x, y, cls = make_batch(2, 64, seed=181, with_cls=True)
    near = torch.from_numpy(np.stack([np.roll(m, (2, 1), (0, 1)) for m in y.numpy()])).float()
    g = torch.Generator().manual_seed(3)
    seg = (4.0 * (near - 0.5) + torch.randn(near.shape, generator=g)).view(2, 1, 64, 64).to(DEV)
    cls_logits = torch.zeros(2, 3, device=DEV)
    batches = [(x, y.float().view(2, 1, 64, 64), None, cls)]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss())
        met = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss(), curve={"bins": 100})
    assert {k: met[k] for k in plain} == plain and set(met) == set(plain) | set(c.KEYS)
    want = curve_ref.hist(seg.cpu().numpy(), y.numpy(), _edges(100))
    assert {k: met[k] for k in c.KEYS} == c.metrics_from_counts(want, 10)


def test_val_cli_writes_curve_and_threshold(tmp_path):
    import val
    from model.model_factory import build_model

    torch.manual_seed(21)
    exp = tmp_path / "exp"
    os.makedirs(exp / "weights")
    wpath = exp / "weights" / "best.pth"
    torch.save(build_model("unet_plain", num_classes=2).state_dict(), wpath)
    K = 100
    base = ["--weights", str(wpath), "--task", "binary", "--model", "unet_plain", "--input-size", "64", "--data-path",
            "synthetic", "--synthetic-test", "2", "--loss", "bce"]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = val.val(val.parse_args(base))
    assert not os.path.exists(exp / "curve.csv")
    with contextlib.redirect_stdout(io.StringIO()) as text:
        m = val.val(val.parse_args(base + ["--curve-metrics", "--curve-bins", str(K), "--threshold", "0.3"]))
    c = _c()
    assert {k: m[k] for k in plain} == plain and set(m) == set(plain) | set(c.KEYS) | set(c.KEYS_AT)
    assert "Best Threshold" in text.getvalue() and "AUROC" in text.getvalue()
    rows = list(csv.reader(open(exp / "curve.csv")))
    assert len(rows) == 1 + K + 1 and rows[0][0] == "threshold"  # a header and K + 1 rows
    assert [float(r[0]) for r in rows[1:]] == [k / K for k in range(K + 1)]
    n = 2 * 64 * 64
    assert all(sum(int(v) for v in r[1:5]) == n for r in rows[1:])
    d = json.load(open(exp / "threshold.json"))
    assert set(d) == {"threshold", "bins", "iou", "iou_at_half"} and d["bins"] == K
    k = round(d["threshold"] * K)
    assert 1 <= k <= K - 1 and d["threshold"] == k / K  # on the grid
    assert d["threshold"] == m["Best Threshold"] and d["iou"] == m["Best IoU"] and d["iou_at_half"] == m["IoU@0.5"]
    assert float(rows[1 + k][7]) == d["iou"] and float(rows[1 + K // 2][7]) == d["iou_at_half"]
    assert d["iou"] >= d["iou_at_half"]
    out = tmp_path / "elsewhere"
    with contextlib.redirect_stdout(io.StringIO()):
        val.val(val.parse_args(base + ["--curve-metrics", "--curve-out", str(out)]))
    assert len(list(csv.reader(open(out / "curve.csv")))) == 1 + 1000 + 1
    with pytest.raises(SystemExit):
        val.parse_args(base + ["--curve-metrics", "--task", "multiclass"])


def test_train_cli_keeps_the_validation_threshold(tmp_path):
    """train.py --curve-metrics: the keys enter the metric history and the test metrics, and threshold.json holds the
    best epoch's validation threshold, not the test split's"""
    import train

    K = 100
    args = train.parse_args(["--task", "binary", "--model", "unet_plain", "--loss", "bce", "--input-size", "64",
                             "--batch-size", "2", "--epochs", "2", "--synthetic-train", "2", "--synthetic-val", "2",
                             "--workers", "0", "--out-dir", str(tmp_path), "--curve-metrics", "--curve-bins", str(K)])
    with contextlib.redirect_stdout(io.StringIO()):
        exp = train.train(args)
    c = _c()
    history = json.load(open(os.path.join(exp, "val_metrics_history.json")))
    summary = json.load(open(os.path.join(exp, "summary.json")))
    tested = json.load(open(os.path.join(exp, "test_metrics.json")))
    assert len(history) == 2 and all(set(c.KEYS) <= set(m) for m in history) and set(c.KEYS) <= set(tested)
    best = history[summary["best_epoch"] - 1]
    assert summary["best_score"] == best["IoU"]  # model selection stays on IoU
    d = json.load(open(os.path.join(exp, "threshold.json")))
    assert d == {"threshold": best["Best Threshold"], "bins": K, "iou": best["Best IoU"], "iou_at_half": best["IoU@0.5"]}
    assert d["threshold"] == round(d["threshold"] * K) / K
    with pytest.raises(SystemExit):
        train.parse_args(["--task", "multiclass", "--curve-metrics"])
