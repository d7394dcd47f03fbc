"""GPU: edge map, exact distance transform, boundary counts and the entry points that report them
(csrc/boundary.hip, unetseg_hip/boundary.py, utils/train_and_eval.py, val.py) against
tests/boundary_ref.py.  Everything is an integer, so every comparison is equality.

Sizes: 1 x 1, single rows and columns, 2 x 2, 63 .. 65 and 129 around one and two chunks, two rectangles
with both edges off the chunk, and L - 1, L, L + 1, 2 L + 1 on each axis (the other at 5) from
``boundary.chunk()``, so that a change of the segment length moves the cases with it.  The counts run
at the default K (one histogram window in LDS), at K = 5000 (two windows) and at K = 16 and 65536.
"""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import boundary_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXED = [(1, 1), (1, 70), (70, 1), (2, 2), (63, 63), (64, 64), (65, 65), (129, 129), (37, 130), (130, 37)]
AROUND = ["L-1", "L", "L+1", "2L+1"]


def _b():
    from unetseg_hip import boundary

    return boundary


def around(name, L):
    return {"L-1": L - 1, "L": L, "L+1": L + 1, "2L+1": 2 * L + 1}[name]


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def host(t):
    return t.cpu().numpy()


def patterns(H, W, seed):
    """name -> site map: none, all, each corner, a full row, a full column, a checkerboard, noise"""
    g = np.random.default_rng(seed)
    out = {"none": np.zeros((H, W), np.uint8), "all": np.ones((H, W), np.uint8)}
    for name, (y, x) in {"corner00": (0, 0), "corner01": (0, W - 1), "corner10": (H - 1, 0),
                         "corner11": (H - 1, W - 1)}.items():
        out[name] = np.zeros((H, W), np.uint8)
        out[name][y, x] = 1
    out["row"] = np.zeros((H, W), np.uint8)
    out["row"][H // 3] = 1
    out["column"] = np.zeros((H, W), np.uint8)
    out["column"][:, (2 * W) // 3] = 1
    out["checker"] = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)
    for d in (0.001, 0.01, 0.3):
        out[f"noise{d}"] = (g.random((H, W)) < d).astype(np.uint8)
    return out


def check_sqdist(H, W):
    b = _b()
    pats = patterns(H, W, 7 * H + W)
    stack = np.stack(list(pats.values()))
    want = boundary_ref.sqdist(stack)
    assert (want[0] == b.INF).all() and not want[1].any()
    d = dev(stack, np.uint8)
    got = b.sqdist(d)
    assert got.dtype == torch.int32 and got.shape == d.shape
    got = host(got)
    for k, name in enumerate(pats):
        assert np.array_equal(got[k], want[k]), (name, H, W)
    assert np.array_equal(host(d), stack)  # the input is left alone
    one = b.sqdist(d[3])  # a single [H, W] map, and a bool one
    assert one.shape == (H, W) and np.array_equal(host(one), want[3])
    assert np.array_equal(host(b.sqdist(d[-1].bool())), want[-1])


# ---- sqdist ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", FIXED)
def test_sqdist_sizes_and_patterns(H, W):
    check_sqdist(H, W)


@pytest.mark.parametrize("name", AROUND)
@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_sqdist_around_the_chunk(name, axis):
    L = _b().chunk()
    if L == 0:
        return  # no seam to place a size at
    n = around(name, L)
    check_sqdist(*((n, 5) if axis == "rows" else (5, n)))


def test_sqdist_sites_on_a_slanted_line_and_far_apart():
    """the window of the row pass stays open longest along a diagonal; two sites in opposite corners of a
    300-wide image put whole chunks between a pixel and its nearest site"""
    b = _b()
    diag = np.eye(150, 300, dtype=np.uint8)
    two = np.zeros((150, 300), np.uint8)
    two[0, 0] = two[149, 299] = 1
    stack = np.stack([diag, two])
    assert np.array_equal(host(b.sqdist(dev(stack, np.uint8))), boundary_ref.sqdist(stack))


def test_sqdist_batch_does_not_leak():
    b = _b()
    g = np.random.default_rng(5)
    stack = np.stack([(g.random((70, 133)) < 0.01).astype(np.uint8), np.zeros((70, 133), np.uint8),
                      (g.random((70, 133)) < 0.2).astype(np.uint8)])
    got = host(b.sqdist(dev(stack, np.uint8)))
    assert np.array_equal(got, boundary_ref.sqdist(stack))
    assert (got[1] == b.INF).all()
    for n in range(3):
        assert np.array_equal(host(b.sqdist(dev(stack[n], np.uint8))), got[n])


def test_sqdist_is_reproducible():
    b = _b()
    g = np.random.default_rng(6)
    d = dev((g.random((2, 200, 131)) < 0.003).astype(np.uint8), np.uint8)
    assert torch.equal(b.sqdist(d), b.sqdist(d))


# ---- edges -------------------------------------------------------------------------------------------
def class_noise(seed, shape, ignore=7):
    g = np.random.default_rng(seed)
    m = g.integers(0, 5, shape).astype(np.int32)
    m[g.random(shape) < 0.1] = ignore
    return m


@pytest.mark.parametrize("shape", [(37, 130), (3, 65, 64), (1, 1), (1, 9), (9, 1)])
def test_edges_every_class_with_and_without_ignore(shape):
    b = _b()
    m = class_noise(11, shape)
    d = dev(m)
    for c in (0, 1, 2, 3, 4, 7):
        for ignore in (None, 7):
            got = b.edges(d, c, ignore)
            assert got.dtype == torch.uint8 and got.shape == d.shape
            assert np.array_equal(host(got), boundary_ref.edges(m, c, ignore)), (c, ignore)
    assert np.array_equal(host(d), m)
    assert not host(b.edges(d, 7, 7)).any()


def test_edges_of_smooth_shapes_and_the_frame():
    b = _b()
    m = discs(129, 70)
    assert np.array_equal(host(b.edges(dev(m), 1)), boundary_ref.edges(m, 1))
    full = np.ones((40, 70), np.int32)
    assert not host(b.edges(dev(full), 1)).any()


# ---- counts ------------------------------------------------------------------------------------------
def discs(H, W):
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.int32)
    for cy, cx, r in ((0.3, 0.35, 0.22), (0.72, 0.6, 0.2), (0.05, 0.9, 0.15)):  # the last one runs over the frame
        m[(y - cy * H) ** 2 + (x - cx * W) ** 2 < (r * min(H, W)) ** 2] = 1
    return m


def curves(H, W):
    """one-pixel-wide lines: a sine, a slanted line and a vertical stroke"""
    m = np.zeros((H, W), np.int32)
    x = np.arange(W)
    m[np.clip((H / 2 + H / 4 * np.sin(x / 6.0)).astype(int), 0, H - 1), x] = 1
    m[np.clip(x * H // (2 * W) + 2, 0, H - 1), x] = 1
    m[H // 5:H - 3, W // 4] = 1
    return m


def shifted(m, dy, dx):
    """m moved down by dy and right by dx; what leaves the image is lost and background comes in"""
    out = np.zeros_like(m)
    H, W = m.shape
    out[dy:, dx:] = m[:H - dy, :W - dx]
    return out


SHAPES = {"discs": discs, "curves": curves}


@pytest.mark.parametrize("shape", [(65, 65), (129, 70)])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_counts_of_shifted_shapes(kind, shape):
    b = _b()
    t = SHAPES[kind](*shape)
    for dy, dx in ((0, 0), (1, 0), (0, 3), (5, 5)):
        p = shifted(t, dy, dx)
        dp, dt = dev(p), dev(t)
        got = b.counts(dp, dt)
        assert got.dtype == torch.int64 and got.shape == (2 * (4096 + 2) + 2,) and got.is_cuda
        want = boundary_ref.counts(p, t, 1, 4096)
        assert np.array_equal(host(got), want), (dy, dx)
        assert np.array_equal(host(dp), p) and np.array_equal(host(dt), t)  # the inputs are left alone
        assert torch.equal(b.counts(dp, dt), got)  # and a second run gives the same array
        if (dy, dx) == (0, 0):
            m = b.metrics_from_counts(got, 4096)
            assert m["Boundary F1"] == 1.0 and m["Boundary IoU"] == 1.0 and m["HD95"] == 0.0


def test_counts_empty_prediction_and_beyond_k():
    b = _b()
    t = discs(65, 65)
    p = np.zeros_like(t)
    for K, d in ((4096, None), (16, 2)):
        got = host(b.counts(dev(p), dev(t), K=K, biou_d=d))
        assert np.array_equal(got, boundary_ref.counts(p, t, 1, K, biou_d=d))
        assert got[:K + 2].sum() == 0 and got[2 * K + 3] == got[K + 2:2 * K + 4].sum() > 0
    far_p, far_t = np.zeros((40, 90), np.int32), np.zeros((40, 90), np.int32)
    far_p[3:9, 2:8] = 1
    far_t[30:36, 70:80] = 1  # every edge pixel is further than sqrt(16) from the other side's
    got = host(b.counts(dev(far_p), dev(far_t), K=16, biou_d=3))
    assert np.array_equal(got, boundary_ref.counts(far_p, far_t, 1, 16, biou_d=3))
    assert got[17] > 0 and got[35] > 0 and got[:17].sum() == 0 and got[18:35].sum() == 0
    assert b.metrics_from_counts(got, 16, 2.0)["HD95"] == math.inf


@pytest.mark.parametrize("K", [5000, 65536])
def test_counts_over_several_histogram_windows(K):
    """bins beyond the block's LDS window are counted by further grid rows"""
    b = _b()
    t, p = np.zeros((129, 70), np.int32), np.zeros((129, 70), np.int32)
    t[5:15, 5:15] = t[110:120, 50:60] = 1  # the second square is some 90 pixels from every prediction edge
    p[6:16, 8:18] = p[20, 3:40] = 1
    got = host(b.counts(dev(p), dev(t), K=K, biou_d=9))
    want = boundary_ref.counts(p, t, 1, K, biou_d=9)
    assert np.array_equal(got, want)
    assert want[:8196].sum() > 0 and want[8196:2 * K + 4].sum() > 0  # both the first window and a later one count


def test_counts_batch_classes_and_ignore():
    b = _b()
    t = class_noise(21, (3, 40, 67), ignore=5)
    p = class_noise(22, (3, 40, 67), ignore=5)
    p[p == 5] = 0  # a prediction holds classes only
    t[1] = 0       # one image without any target edge
    for c in (1, 4):
        for ignore in (None, 5):
            got = host(b.counts(dev(p), dev(t), c=c, K=64, biou_d=3, ignore_index=ignore))
            assert np.array_equal(got, boundary_ref.counts(p, t, c, 64, biou_d=3, ignore=ignore)), (c, ignore)


def test_counts_accumulate_into_out():
    b = _b()
    t1, t2 = discs(65, 65), curves(65, 65)
    p1, p2 = shifted(t1, 0, 3), shifted(t2, 1, 0)
    out = b.counts(dev(p1), dev(t1))
    again = b.counts(dev(p2), dev(t2), out=out)
    assert again is out
    assert np.array_equal(host(out), boundary_ref.counts(p1, t1) + boundary_ref.counts(p2, t2))
    assert np.array_equal(host(b.counts(dev(np.stack([p1, p2])), dev(np.stack([t1, t2])))), host(out))


def test_refusals():
    b = _b()
    z = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        b.edges(z.long())
    with pytest.raises(ValueError):
        b.sqdist(z)
    with pytest.raises(ValueError):
        b.counts(z, torch.zeros(4, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        b.counts(z, z, K=65537)
    with pytest.raises(ValueError):
        b.counts(z, z, K=16, biou_d=5)
    with pytest.raises(ValueError):
        b.counts(z, z, out=torch.zeros(7, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        b.edges(z, 1, ignore_index=-1)


# ---- entry points --------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """a model that answers the k-th call with the k-th of its fixed outputs"""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.k = outputs, 0

    def forward(self, x):
        out = self.outputs[self.k]
        self.k += 1
        return out


def smooth_logits(seed, B, C, H, W):
    """low-frequency logits, so that the argmax has regions rather than salt and pepper"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(B, C, H // 8, W // 8, generator=g)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False).contiguous()


def test_labels_from_logits_agrees_with_binary_confusion_on_ties():
    from unetseg_hip import losses

    b = _b()
    g = torch.Generator().manual_seed(3)
    two = torch.randn(2, 2, 16, 24, generator=g)
    two[:, 1, ::2] = two[:, 0, ::2]  # every other row a tie
    one = torch.randn(2, 1, 16, 24, generator=g)
    one[:, :, ::2] = 0.0
    tgt = torch.randint(0, 2, (2, 16, 24), generator=g)
    for out in (two, one):
        lab = b.labels_from_logits(out.to(DEV))
        assert lab.dtype == torch.int32 and lab.shape == (2, 16, 24)
        assert not lab[:, ::2].any()  # a tie is class 0
        tp, fp, fn, tn = losses.binary_confusion(out.to(DEV), tgt.to(DEV)).tolist()
        pred, t = lab.cpu() == 1, tgt == 1
        assert [tp, fp, fn, tn] == [int((pred & t).sum()), int((pred & ~t).sum()), int((~pred & t).sum()),
                                    int((~pred & ~t).sum())]
    many = torch.randn(2, 4, 16, 24, generator=g)
    many[:, 2] = many[:, 1]
    many[:, 3, 4:] = many[:, 0, 4:]
    assert torch.equal(b.labels_from_logits(many.to(DEV)).cpu(), many.argmax(1).to(torch.int32))
    assert not (b.labels_from_logits(many.to(DEV)) == 2).any()


def test_evaluate_binary_reports_the_reference_metrics():
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_binary

    b = _b()
    batches, outs, want = [], [], 0
    for k in range(2):
        x, y = make_batch(2, 64, seed=40 + k)
        logits = smooth_logits(50 + k, 2, 2, 64, 64)
        near = np.stack([shifted(m, 1, 2) for m in y.numpy()])  # near the target, not on it
        logits[:, 1] += 4.0 * (torch.from_numpy(near).float() - 0.5)
        batches.append((x, y, None))
        outs.append(logits.to(DEV))
        pred = (logits[:, 1] > logits[:, 0]).numpy().astype(np.int32)
        want = want + boundary_ref.counts(pred, y.numpy().astype(np.int32), 1, 4096)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_binary(Stub(outs), batches, DEV, "bce", None)
        met = evaluate_binary(Stub(outs), batches, DEV, "bce", None, boundary={"tolerance": 2.0, "biou_d": None})
    assert set(plain) == {"Dice", "IoU", "Precision", "Recall", "Accuracy", "Loss"}
    assert set(met) == set(plain) | set(b.KEYS)
    assert {k: met[k] for k in plain} == plain
    ref = boundary_ref.metrics_from_counts(want, 4096, 2.0)
    assert {k: met[k] for k in b.KEYS} == ref
    assert 0.0 < ref["Boundary F1"] < 1.0 and 0.0 < ref["Boundary IoU"] < 1.0  # the case says something
    with contextlib.redirect_stdout(io.StringIO()):
        wide = evaluate_binary(Stub(outs), batches, DEV, "bce", None, boundary={"tolerance": 5.0, "biou_d": 3})
    want3 = sum(boundary_ref.counts((o[:, 1] > o[:, 0]).cpu().numpy().astype(np.int32),
                                    bt[1].numpy().astype(np.int32), 1, 4096, biou_d=3) for o, bt in zip(outs, batches))
    assert {k: wide[k] for k in b.KEYS} == boundary_ref.metrics_from_counts(want3, 4096, 5.0)


def test_evaluate_multitask_and_multiclass_report_the_reference_metrics():
    from model.unet_multitask import MultiTaskLoss
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate, evaluate_multitask

    b = _b()
    # multitask: one seg logit, class 1 where it is positive
    batches, outs, want = [], [], 0
    for k in range(2):
        x, y, c = make_batch(2, 64, seed=60 + k, with_cls=True)
        seg = smooth_logits(70 + k, 2, 1, 64, 64) + 4.0 * (torch.roll(y, 2, 1).float().unsqueeze(1) - 0.5)
        batches.append((x, y, None, c))
        outs.append((seg.to(DEV), torch.randn(2, 3, generator=torch.Generator().manual_seed(k)).to(DEV)))
        want = want + boundary_ref.counts((seg[:, 0] > 0).numpy().astype(np.int32), y.numpy().astype(np.int32), 1, 4096)
    plain = evaluate_multitask(Stub(outs), batches, DEV, MultiTaskLoss())
    met = evaluate_multitask(Stub(outs), batches, DEV, MultiTaskLoss(), boundary={"tolerance": 2.0})
    assert set(plain) == {"Loss", "Seg Loss", "Cls Loss", "IoU", "Dice", "Cls Acc"}
    assert {k: met[k] for k in plain} == plain
    assert {k: met[k] for k in b.KEYS} == boundary_ref.metrics_from_counts(want, 4096, 2.0)
    # multiclass: classes 1 .. C - 1, target value C ignored, mean over the classes with a target edge
    C = 4
    g = torch.Generator().manual_seed(9)
    batches, outs, per = [], [], {c: 0 for c in range(1, C)}
    for k in range(2):
        logits = smooth_logits(80 + k, 2, C, 64, 64)
        t = smooth_logits(90 + k, 2, C + 1, 64, 64).argmax(1)
        t[t == 3] = 0  # class 3 never occurs in the target: it has no say in the mean
        batches.append((torch.rand(2, 3, 64, 64, generator=g), t, torch.eye(C + 1)[t.reshape(-1)].reshape(2, 64, 64, C + 1)))
        outs.append(logits.to(DEV))
        pred = logits.argmax(1).numpy().astype(np.int32)
        for c in per:
            per[c] = per[c] + boundary_ref.counts(pred, t.numpy().astype(np.int32), c, 4096, ignore=C)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate(Stub(outs), batches, DEV, True, False, C)
        met = evaluate(Stub(outs), batches, DEV, True, False, C, boundary={"tolerance": 3.0})
    assert set(plain) == {"Pixel Accuracy", "Mean Accuracy", "Mean IoU", "Frequency Weighted IoU", "Loss"}
    assert {k: met[k] for k in plain} == plain
    assert per[3][4098:2 * 4098].sum() == 0 and all(per[c][4098:2 * 4098].sum() > 0 for c in (1, 2))
    refs = [boundary_ref.metrics_from_counts(per[c], 4096, 3.0) for c in (1, 2)]
    for k in b.KEYS:
        assert met[k] == pytest.approx((refs[0][k] + refs[1][k]) / 2, rel=1e-12), k


def test_val_flags():
    import val

    a = val.parse_args(["--boundary-metrics"])
    assert a.boundary_metrics and a.boundary_tolerance == 2.0 and a.boundary_iou_d == 0
    assert val.metric_options(a)["boundary"] == {"tolerance": 2.0, "biou_d": None}
    assert val.metric_options(val.parse_args([]))["boundary"] is None
