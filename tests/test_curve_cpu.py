"""CPU checks of the operating-point and calibration metrics (unetseg_hip/curve.py): the edge table, the host
readers against a brute force that never sees a histogram (tests/curve_ref.py), ``labels_at`` on CPU tensors, and
the argument checks of the built library (no device is touched)."""
import ctypes

import numpy as np
import pytest
import torch

import curve_ref
from unetseg_hip import curve

TOL = 1e-12


def _close(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])


def _hist_of(bins, labels, K):
    return np.stack([np.bincount(bins[labels == 0], minlength=K), np.bincount(bins[labels == 1], minlength=K)])


# ---- the edge table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 10, 1000, 4096])
def test_edges(K):
    e = curve.edges(K)
    assert e.dtype == torch.float32 and e.device.type == "cpu" and tuple(e.shape) == (K - 1,)
    a = e.numpy()
    assert (a[1:] > a[:-1]).all()  # strictly ascending in fp32
    assert a[K // 2 - 1] == 0.0 and not np.signbit(a[K // 2 - 1])
    assert np.array_equal(a.view(np.uint32)[:K // 2 - 1], (-a[::-1]).view(np.uint32)[:K // 2 - 1])  # bit for bit
    assert np.array_equal(a, -a[::-1])
    k = np.arange(1, K, dtype=np.float64)
    want = np.log(k / (K - k))
    assert np.abs(a - want).max() <= np.abs(want).max() * 2.0 ** -23  # the float64 value, rounded once (or negated)
    assert np.array_equal(a[:K // 2 - 1], want[:K // 2 - 1].astype(np.float32))
    assert curve.edges(K) is e  # cached


@pytest.mark.parametrize("K", [3, 999, 0, 1, -2, 4098])
def test_edges_refuse(K):
    with pytest.raises(ValueError, match="K must be even"):
        curve.edges(K)


# ---- table and histogram sums --------------------------------------------------------------------------
def _random_case(seed, nch, shape=(3, 17, 23), K=100, ignore=None):
    g = np.random.default_rng(seed)
    B, H, W = shape
    out = (g.standard_normal((B, nch, H, W)) * 2.0).astype(np.float32)
    tgt = (g.random((B, H, W)) < 0.3).astype(np.int64)
    tgt[g.random((B, H, W)) < 0.05] = 7  # another class: a negative
    if ignore is not None:
        tgt[g.random((B, H, W)) < 0.3] = ignore
    return out, tgt


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("ignore", [None, 255])
def test_table_and_row_sums(nch, ignore):
    K = 100
    out, tgt = _random_case(1, nch, K=K, ignore=ignore)
    e = curve.edges(K).numpy()
    h = curve_ref.hist(out, tgt, e, ignore)
    valid = np.ones(tgt.shape, bool) if ignore is None else tgt != ignore
    assert h.sum() == valid.sum() and h[1].sum() == (tgt == 1).sum() and h[0].sum() == (valid & (tgt != 1)).sum()
    rows = curve.table(h)
    assert [r[0] for r in rows] == list(range(K + 1))
    # k = K / 2 is the z > 0 rule
    z = curve_ref.z_of(out).reshape(-1)
    pred, pos, v = z > 0, tgt.reshape(-1) == 1, valid.reshape(-1)
    want = (int((pred & pos & v).sum()), int((pred & ~pos & v).sum()), int((~pred & pos & v).sum()),
            int((~pred & ~pos & v).sum()))
    assert rows[K // 2][1:] == want
    assert rows[0][1:] == (int(h[1].sum()), int(h[0].sum()), 0, 0)  # everything positive
    assert rows[K][1:] == (0, 0, int(h[1].sum()), int(h[0].sum()))  # nothing positive
    b, y = curve_ref.scores(out, tgt, e, ignore)
    for k in (1, 17, K - 1):
        assert rows[k][1:] == curve_ref.confusion_at(b, y, k)
    assert curve.table(torch.from_numpy(h)) == rows and curve.table(h.tolist()) == rows


# ---- metrics_from_counts against the brute force -------------------------------------------------------
@pytest.mark.parametrize("K,ece_bins", [(100, 10), (10, 5), (1000, 10), (2, 1), (4096, 16)])
@pytest.mark.parametrize("seed", [0, 1])
def test_metrics_random(K, ece_bins, seed):
    g = np.random.default_rng(100 + seed)
    n = 3000
    y = (g.random(n) < 0.25).astype(np.int64)
    p = np.clip(g.normal(0.3 + 0.4 * y, 0.2), 0, 1 - 1e-9)  # informative, imperfect scores
    b = (p * K).astype(np.int64)
    tk = max(1, K // 3) if K > 2 else 1
    _close(curve.metrics_from_counts(_hist_of(b, y, K), ece_bins, tk / K), curve_ref.metrics(b, y, K, ece_bins, tk))
    got = curve.metrics_from_counts(_hist_of(b, y, K), ece_bins)
    assert tuple(got) == curve.KEYS
    if K >= 100:
        assert got["Best IoU"] >= got["IoU@0.5"] and 0.5 < got["AUROC"] < 1.0 and 0.0 < got["AP"] < 1.0


def test_metrics_perfect_separator():
    K = 100
    b = np.array([3, 10, 20, 39, 60, 61, 99, 80])
    y = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    got = curve.metrics_from_counts(_hist_of(b, y, K), 10)
    _close(got, curve_ref.metrics(b, y, K, 10))
    assert got["AP"] == 1.0 and got["AUROC"] == 1.0 and got["Best IoU"] == 1.0 and got["Best F1"] == 1.0
    assert got["Best Threshold"] == 0.5  # every k in 40 .. 60 separates: the one nearest K / 2
    assert got["IoU@0.5"] == 1.0


@pytest.mark.parametrize("label", [0, 1])
def test_metrics_one_class_only(label):
    """all-negative and all-positive targets: the documented 0 / 0.5 values, nothing divided by zero"""
    K = 10
    b = np.array([0, 2, 2, 5, 9, 9, 7])
    y = np.full(b.shape, label)
    got = curve.metrics_from_counts(_hist_of(b, y, K), 5, 0.3)
    _close(got, curve_ref.metrics(b, y, K, 5, 3))
    assert got["AUROC"] == 0.5
    if label == 0:
        assert got["AP"] == 0.0 and got["Best IoU"] == 0.0 and got["Best F1"] == 0.0 and got["IoU@0.5"] == 0.0
        assert got["Best Threshold"] == 0.5  # every k ties at 0
        assert got["Recall@T"] == 0.0 and got["Precision@T"] == 0.0
    else:
        # the pixel of bin 0 is positive at no k >= 1; k = 1 and 2 keep the other six, 2 is nearer K / 2
        assert got["AP"] == 1.0 and got["Best IoU"] == 6 / 7 and got["Best Threshold"] == 0.2
        assert got["Precision@T"] == 1.0 and got["Recall@T"] == 4 / 7
    empty = curve.metrics_from_counts(np.zeros((2, K), np.int64), 5, 0.3)
    _close(empty, curve_ref.metrics(np.zeros(0, np.int64), np.zeros(0, np.int64), K, 5, 3))
    assert empty["ECE"] == 0.0 and empty["AUROC"] == 0.5 and empty["AP"] == 0.0 and empty["Best Threshold"] == 0.5


def test_metrics_tie_rule():
    """the best IoU is reached at two thresholds on either side of K / 2: the nearer one wins, and at equal
    distance the lower"""
    K = 20
    h = np.zeros((2, K), np.int64)
    h[1, 15] = 4  # positives in bin 15, negatives in bin 2: every k in 3 .. 15 gives IoU 1
    h[0, 2] = 4
    got = curve.metrics_from_counts(h, 10)
    assert got["Best IoU"] == 1.0 and got["Best Threshold"] == 10 / K
    h2 = h.copy()
    h2[0, 9] = 1  # a negative in bin 9 spoils k <= 9: the best k are 10 .. 15
    assert curve.metrics_from_counts(h2, 10)["Best Threshold"] == 10 / K
    h3 = h.copy()
    h3[0, 10] = 1  # spoils k <= 10: the best k are 11 .. 15
    assert curve.metrics_from_counts(h3, 10)["Best Threshold"] == 11 / K
    h4 = np.zeros((2, K), np.int64)
    h4[1, 8] = h4[1, 15] = 1  # k = 7 .. 8 and k = 12 .. 15 reach the best IoU 1/2, k = 9 .. 11 only 1/4:
    h4[0, 6], h4[0, 11] = 3, 2  # 8 and 12 are equally near K / 2, the lower wins
    for hh in (h, h2, h3, h4):
        _close(curve.metrics_from_counts(hh, 10), curve_ref.metrics(*curve_ref.expand(hh), K, 10))
    rows = curve.table(h4)
    iou = [tp / (tp + fp + fn) for _, tp, fp, fn, _ in rows[1:K]]
    assert [k + 1 for k, v in enumerate(iou) if v == max(iou)] == [7, 8, 12, 13, 14, 15]
    assert curve.metrics_from_counts(h4, 10)["Best Threshold"] == 8 / K


def test_metrics_refusals():
    h = np.zeros((2, 100), np.int64)
    with pytest.raises(ValueError, match="multiple of ece_bins"):
        curve.metrics_from_counts(h, 7)
    with pytest.raises(ValueError, match="multiple of ece_bins"):
        curve.metrics_from_counts(h, 0)
    with pytest.raises(ValueError, match="threshold"):
        curve.metrics_from_counts(h, 10, 0.505)
    with pytest.raises(ValueError, match="threshold"):
        curve.metrics_from_counts(h, 10, 1.0)
    with pytest.raises(ValueError, match="K must be even"):
        curve.metrics_from_counts(np.zeros((2, 101), np.int64))
    with pytest.raises(ValueError, match=r"\[2, K\]"):
        curve.table(np.zeros((3, 100), np.int64))


def test_ece_is_foreground_reliability():
    """a perfectly calibrated histogram at the midpoints scores 0; shifting every pixel's label to 1 scores the
    mean distance of the midpoints from 1"""
    K = 10
    h = np.zeros((2, K), np.int64)
    for b in range(K):  # bin b: 20 pixels, (2 b + 1) of them positive = the midpoint (b + 1/2) / K
        h[1, b], h[0, b] = 2 * b + 1, 20 - (2 * b + 1)
    assert curve.metrics_from_counts(h, 10)["ECE"] <= TOL
    assert curve.metrics_from_counts(h, 5)["ECE"] <= TOL
    allpos = np.stack([np.zeros(K, np.int64), h.sum(0)])
    assert abs(curve.metrics_from_counts(allpos, 10)["ECE"] - 0.5) <= TOL


# ---- labels_at -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2])
def test_labels_at_cpu(nch):
    K = 100
    out, _ = _random_case(5, nch)
    e = curve.edges(K).numpy()
    flat = out.reshape(out.shape[0], nch, -1)
    flat[0, -1, :K - 1] = e  # scores exactly on the edges (nch 2: o0 = 0 there)
    if nch == 2:
        flat[0, 0, :K - 1] = 0.0
    b = curve_ref.bins_of(curve_ref.z_of(out), e).reshape(out.shape[0], *out.shape[2:])
    t = torch.from_numpy(out)
    for k in (1, 37, 50, 99):
        lab = curve.labels_at(t, k / K, K)
        assert lab.dtype == torch.int32 and tuple(lab.shape) == (out.shape[0],) + out.shape[2:]
        assert np.array_equal(lab.numpy(), (b >= k).astype(np.int32)), k
    from unetseg_hip.boundary import labels_from_logits
    assert torch.equal(curve.labels_at(t, 0.5, K), labels_from_logits(t))
    for bad in (0.505, 0.0, 1.0, -0.1, 1 / 3):
        with pytest.raises(ValueError, match="threshold"):
            curve.labels_at(t, bad, K)
    with pytest.raises(ValueError, match="logits"):
        curve.labels_at(torch.zeros(2, 3, 4, 4), 0.5, K)


# ---- accumulator options -------------------------------------------------------------------------------
def test_accumulator_options():
    with pytest.raises(ValueError, match="unknown curve options"):
        curve.Accumulator({"K": 100})
    with pytest.raises(ValueError, match="ece_bins"):
        curve.Accumulator({"bins": 100, "ece_bins": 7})
    with pytest.raises(ValueError, match="threshold"):
        curve.Accumulator({"bins": 100, "threshold": 0.505})
    with pytest.raises(ValueError, match="K must be even"):
        curve.Accumulator({"bins": 101})
    acc = curve.Accumulator({"bins": 100, "threshold": 0.3})
    assert acc.out is None and len(acc.table()) == 101
    m = acc.metrics()  # nothing added
    assert tuple(m) == curve.KEYS + curve.KEYS_AT and m["AUROC"] == 0.5 and m["Best IoU"] == 0.0
    assert curve.Accumulator({}).K == 1000


def test_written_files(tmp_path):
    import csv
    import json

    K = 10
    g = np.random.default_rng(3)
    h = g.integers(0, 50, (2, K))
    rows = curve.table(h)
    curve.write_csv(tmp_path / "curve.csv", rows)
    got = list(csv.reader(open(tmp_path / "curve.csv")))
    assert got[0] == ["threshold", "tp", "fp", "fn", "tn", "precision", "recall", "iou"] and len(got) == K + 2
    for line, (k, tp, fp, fn, tn) in zip(got[1:], rows):
        assert float(line[0]) == k / K and [int(v) for v in line[1:5]] == [tp, fp, fn, tn]
        assert float(line[7]) == (tp / (tp + fp + fn) if tp + fp + fn else 0.0)
    m = curve.metrics_from_counts(h, 5)
    curve.write_threshold(tmp_path / "threshold.json", m, K)
    d = json.load(open(tmp_path / "threshold.json"))
    assert d == {"threshold": m["Best Threshold"], "bins": K, "iou": m["Best IoU"], "iou_at_half": m["IoU@0.5"]}


# ---- the built library: host-only checks ---------------------------------------------------------------
def test_argument_errors_reported_without_device():
    """unetseg_curve_max_bins answers, and every bad argument of unetseg_curve_hist is refused before any HIP call;
    an empty input returns 0 without a launch"""
    from unetseg_hip import lib

    raw = lib.load()
    assert raw.unetseg_curve_max_bins() == 4096 == curve.MAX_BINS
    assert lib.lib.curve_max_bins() == 4096
    assert raw.unetseg_abi_version() == 1
    A, T, E, H = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced

    def call(out=A, nch=2, tgt=T, B=2, P=35, ignore=-1, edges=E, K=1000, hist=H):
        return raw.unetseg_curve_hist(out, nch, tgt, B, P, ignore, edges, K, hist, None)

    for bad, word in ((dict(K=1), b"K 1 "), (dict(K=4097), b"K 4097"), (dict(K=0), b"K 0 "), (dict(K=-5), b"K -5"),
                      (dict(nch=3), b"nch 3"), (dict(nch=0), b"nch 0"), (dict(out=None), b"null"),
                      (dict(tgt=None), b"null"), (dict(edges=None), b"null"), (dict(hist=None), b"null"),
                      (dict(B=-1), b"shape"), (dict(P=-1), b"shape"), (dict(B=1 << 20, P=1 << 30), b"2^40")):
        assert call(**bad) != 0, bad
        msg = raw.unetseg_last_error()
        assert b"curve_hist" in msg and word in msg, (bad, msg)
    assert call(B=0) == 0 and call(P=0) == 0  # empty: nothing is launched
    assert call(B=0, K=2) == 0 and call(B=0, K=4096) == 0 and call(B=0, nch=1) == 0
    with pytest.raises(RuntimeError, match="unetseg_curve_hist failed.*K 4097"):
        lib.lib.curve_hist(A, 2, T, 2, 35, -1, E, 4097, H, None)
    assert ctypes.sizeof(ctypes.c_long) == 8
