"""GPU: the object-level counts, the pair listing and their way into the evaluate loops (csrc/objects.hip,
unetseg_hip/objects.py) against tests/objects_ref.py, bit for bit.

Everything is integer, so every comparison is equality: ``counts`` as a whole and ``pairs`` as a whole.  Sizes
come from ``ccl.tile()`` and ``objects.tile()`` so that a change of either tile moves the cases with it.  The maps
are those of ``objects_ref.all_maps``, on which tests/test_objects_cpu.py checks the capacity claim.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

import ccl_ref
import objects_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _o():
    from unetseg_hip import objects

    return objects


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def check(pred, target, conn=8, c=1, ignore=None):
    """counts and pairs of one map or batch against the reference; the inputs stay what they were, two runs are
    bitwise equal and no insertion is dropped.  Returns the reference counts"""
    o = _o()
    want = ref.counts(pred, target, c, conn, ignore)
    p, t = dev(pred), dev(target)
    got = o.counts(p, t, c, conn, ignore)
    assert got.dtype == torch.int64 and got.shape == (20,) and got.device.type == "cuda"
    assert got.tolist() == want
    assert got[18].item() == 0
    rows = o.pairs(p, t, c, conn, ignore)
    assert rows.dtype == torch.int32 and rows.device.type == "cuda"
    assert np.array_equal(rows.cpu().numpy(), ref.pairs(pred, target, c, conn, ignore))
    assert torch.equal(o.counts(p, t, c, conn, ignore), got)
    assert torch.equal(o.pairs(p, t, c, conn, ignore), rows)
    assert np.array_equal(p.cpu().numpy(), pred) and np.array_equal(t.cpu().numpy(), target)
    return want


def test_tile_query():
    tw, th = _o().tile()
    assert tw == 64 and th > 0


@pytest.mark.parametrize("H,W", ref.FIXED_SIZES)
def test_sizes(H, W):
    p, t = ref.size_map(H, W)
    for conn in (4, 8):
        check(p, t, conn)
    check(np.ones((H, W), np.int32), np.ones((H, W), np.int32))
    check(np.zeros((H, W), np.int32), np.ones((H, W), np.int32))


@pytest.mark.parametrize("which,axis", [("ccl", "H"), ("ccl", "W"), ("objects", "H"), ("objects", "W")])
def test_sizes_around_the_tiles(which, axis):
    from unetseg_hip import ccl

    tw, th = ccl.tile() if which == "ccl" else _o().tile()
    for H, W in ref.tile_sizes(th if axis == "H" else tw, axis):
        p, t = ref.size_map(H, W)
        for conn in (4, 8):
            want = check(p, t, conn)
        assert want[17] > 0


@pytest.mark.parametrize("H,W", ref.FLIP_SHAPES)
def test_flip_noise(H, W):
    tp50 = tp95 = splits = merges = 0
    for k, (d, f, conn) in enumerate(ref.FLIP_CASES):
        c = check(*ref.flip_noise(H, W, d, f, 50 + k), conn)
        tp50, tp95, splits, merges = tp50 + c[6], tp95 + c[15], splits + c[4], merges + c[5]
    # on the reference: the inputs are alive
    assert tp50 > 0 and tp95 < tp50 and splits > 0 and merges > 0


@pytest.mark.parametrize("H,W", ref.FLIP_SHAPES)
def test_independent_noise(H, W):
    for conn in (4, 8):
        c = check(ref.noise(H, W, 0.5, 7), ref.noise(H, W, 0.45, 8), conn)
        assert c[17] > 2 * c[6]  # many pairs of low IoU


@pytest.mark.parametrize("n", [65, 129])
def test_checkerboard_fills_the_table(n):
    board = ref.checkerboard(n, n)
    c = check(board, board, 4)
    assert c[0] == c[1] == c[6] == c[17] == (n * n + 1) // 2  # every pixel its own pair: the full load
    c = check(board, board, 8)
    assert c[0] == c[1] == c[17] == 1


def test_one_key_for_every_pixel():
    ones = np.ones((129, 129), np.int32)
    c = check(ones, ones)
    assert c[:6] == [1, 1, 1, 1, 0, 0] and c[16] == 1 << 32


def test_stripes_make_a_pair_grid():
    p, t = ref.stripes(66, 70)
    for conn in (4, 8):
        c = check(p, t, conn)
        assert c[17] == 33 * 35 and c[4] == 35 and c[5] == 33  # every run has length 1


def test_batch_is_the_sum_of_its_images():
    maps = [ref.flip_noise(65, 70, 0.41, 0.1, s) for s in (11, 12, 13)]
    for p, t in maps:  # an object with root 0 on either side in every image: equal keys that must not meet
        p[:3, :3] = t[:2, :4] = 1
    one = [check(p, t) for p, t in maps]
    both = check(np.stack([p for p, _ in maps]), np.stack([t for _, t in maps]))
    assert both == [sum(v) for v in zip(*one)] and both[19] == 3
    rows = ref.pairs(np.stack([p for p, _ in maps]), np.stack([t for _, t in maps]))
    assert [r[0] for r in rows.tolist() if r[1] == 0 and r[2] == 0] == [0, 1, 2]


def test_multiclass_rows():
    o = _o()
    p, t = ref.multiclass(2, 65, 70, 4, 3)
    want = [check(p, t, 8, c) for c in (1, 2, 3, 4)]
    assert all(w[0] > 0 and w[6] > 0 for w in want)
    acc = o.Accumulator({}, classes=(1, 2, 3, 4), ignore_index=5)
    acc.add(dev(p), dev(t))
    assert acc.out.tolist() == want
    assert acc.metrics() == ref.class_mean(want)


def test_ignore_index():
    p, t = ref.flip_noise(65, 70, 0.5, 0.05, 21)
    t = np.where(np.random.default_rng(22).random(t.shape) < 0.2, 9, t).astype(np.int32)
    for conn in (4, 8):
        c = check(p, t, conn, 1, 9)
        assert c != ref.counts(p, np.where(t == 9, 0, t), 1, conn)  # the ignored pixels matter on the prediction's side
    with pytest.raises(ValueError, match="ignore_index"):
        _o().counts(dev(p), dev(t), 9, 8, 9)


def test_out_accumulates():
    o = _o()
    p, t = ref.flip_noise(37, 130, 0.41, 0.1, 31)
    want = ref.counts(p, t)
    out = torch.zeros(20, dtype=torch.int64, device=DEV)
    assert o.counts(dev(p), dev(t), out=out) is out and out.tolist() == want
    o.counts(dev(p), dev(t), out=out)
    assert out.tolist() == [2 * v for v in want]
    with pytest.raises(ValueError, match="out"):
        o.counts(dev(p), dev(t), out=torch.zeros(6, dtype=torch.int64, device=DEV))


def test_empty_batch_and_bad_arguments():
    o = _o()
    e = torch.zeros(0, 8, 8, dtype=torch.int32, device=DEV)
    assert o.counts(e, e).tolist() == [0] * 20 and o.pairs(e, e).shape == (0, 6)
    a = dev(np.ones((4, 4)))
    with pytest.raises(ValueError, match="connectivity"):
        o.counts(a, a, connectivity=6)
    with pytest.raises(ValueError, match="class"):
        o.counts(a, a, c=0)
    with pytest.raises(ValueError, match="differ"):
        o.counts(a, dev(np.ones((4, 5))))
    from unetseg_hip import lib
    ws = torch.empty(o.workspace_bytes(1, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        lib.lib.objects_label(a.data_ptr(), a.data_ptr(), 1, 4, 4, 8, ws.data_ptr(), ws.numel() - 1, 0)
    with pytest.raises(RuntimeError, match="class"):
        lib.lib.objects_pairs(a.data_ptr(), a.data_ptr(), 1, 4, 4, 256, 1, ws.data_ptr(), ws.numel(), 0)


def test_plain_pair_kernel_fills_the_same_table():
    """the variant without the LDS aggregation (the timing tool's comparison) gives the same counts"""
    o = _o()
    for p, t in (ref.flip_noise(65, 130, 0.41, 0.1, 41), ref.stripes(66, 70), (ref.checkerboard(65, 65),) * 2):
        lab = o._Labelled(dev(p)[None], dev(t)[None], 4)
        outs = []
        for agg in (True, False):
            out = torch.zeros(20, dtype=torch.int64, device=DEV)
            lab.pairs(1, aggregate=agg)
            lab.match(1, out)
            outs.append(out.tolist())
        assert outs[0] == outs[1] == ref.counts(p, t, 1, 4)


def test_accumulator_with_min_area():
    o = _o()
    p, t = ref.flip_noise(65, 70, 0.41, 0.1, 51)
    P, T = np.stack([p, np.roll(p, 3, 1)]), np.stack([t, np.roll(t, 3, 1)])
    for conn in (4, 8):
        acc = o.Accumulator({"connectivity": conn, "min_area": 4})
        acc.add(dev(P), dev(T))
        acc.add(dev(P[:1]), dev(T[:1]))
        cleaned = ccl_ref.clean(P, 4, 0, conn)
        assert (cleaned != P).any()
        want = [a + b for a, b in zip(ref.counts(cleaned, T, 1, conn), ref.counts(cleaned[:1], T[:1], 1, conn))]
        assert acc.out.tolist() == [want] and acc.metrics() == ref.metrics(want)
        assert want != [2 * v for v in ref.counts(P[:1], T[:1], 1, conn)]


class Fixed(torch.nn.Module):
    def __init__(self, outs):
        super().__init__()
        self.outs, self.k = outs, 0

    def forward(self, x):
        self.k += 1
        return self.outs[self.k - 1]


def test_evaluate_binary_reports_the_reference_metrics():
    from unetseg_hip.boundary import labels_from_logits
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_binary

    o = _o()
    batches, logits = [], []
    for k in range(2):
        x, y = make_batch(2, 64, seed=70 + k)
        near = torch.from_numpy(np.stack([np.roll(m, (1, 2), (0, 1)) for m in y.numpy()])).float()
        speck = (torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(k)) < 0.02).float()
        z = torch.zeros(2, 2, 64, 64)
        z[:, 1] = 8.0 * ((near + speck).clamp(max=1) - 0.5)
        batches.append((x, y, None))
        logits.append(z.to(DEV))
    want = [0] * 20
    for z, (_, y, _) in zip(logits, batches):
        pred = labels_from_logits(z).cpu().numpy()  # the downloaded class maps
        want = [a + b for a, b in zip(want, ref.counts(pred, y.numpy().astype(np.int32), 1, 8))]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_binary(Fixed(logits), batches, DEV, "bce", None)
        none = evaluate_binary(Fixed(logits), batches, DEV, "bce", None, objects=None)
        met = evaluate_binary(Fixed(logits), batches, DEV, "bce", None, objects={})
        every = evaluate_binary(Fixed(logits), batches, DEV, "bce", None, objects={"connectivity": 8},
                                boundary={"tolerance": 2.0, "biou_d": None}, skeleton={}, curve={"bins": 100})
    assert set(plain) == {"Dice", "IoU", "Precision", "Recall", "Accuracy", "Loss"} and none == plain
    assert list(met) == list(plain) + list(o.KEYS)
    assert {k: met[k] for k in plain} == plain
    want_m = ref.metrics(want)
    assert {k: met[k] for k in o.KEYS} == want_m == {k: every[k] for k in o.KEYS}
    assert list(every)[-len(o.KEYS):] == list(o.KEYS) and "Boundary F1" in every and "clDice" in every and "AP" in every
    assert 0.0 < want_m["PQ"] < 1.0 and want[0] > 0 and want[1] > want[6]  # the case says something


def test_evaluate_multitask_and_multiclass_take_the_option():
    from model.unet_multitask import MultiTaskLoss
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate, evaluate_multitask

    o = _o()
    x, y, c = make_batch(2, 64, seed=81, with_cls=True)
    near = torch.from_numpy(np.stack([np.roll(m, (2, 1), (0, 1)) for m in y.numpy()])).float()
    seg = (6.0 * (near - 0.5)).view(2, 1, 64, 64).to(DEV)
    cls_logits = torch.zeros(2, 3, device=DEV)
    batches = [(x, y.float().view(2, 1, 64, 64), None, c)]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss())
        met = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss(),
                                 objects={"connectivity": 4})
    pred = (seg[:, 0] > 0).cpu().numpy().astype(np.int32)
    assert {k: met[k] for k in plain} == plain and list(met) == list(plain) + list(o.KEYS)
    want = ref.counts(pred, y.numpy().astype(np.int32), 1, 4)
    assert {k: met[k] for k in o.KEYS} == ref.metrics(want) and want[6] > 0

    # multiclass: classes 1 .. 2 and the ignored value num_classes; the mean over the classes with a target object
    p, t = ref.multiclass(2, 64, 64, 2, 9)
    t = np.where(np.random.default_rng(10).random(t.shape) < 0.1, 3, t).astype(np.int32)
    logits = torch.full((2, 3, 64, 64), -4.0)
    logits.scatter_(1, torch.from_numpy(p).long().unsqueeze(1), 4.0)
    tgt = torch.from_numpy(t).long()
    onehot = torch.nn.functional.one_hot(tgt, 4).float()
    mc = [(torch.zeros(2, 3, 64, 64), tgt, onehot)]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate(Fixed([logits.to(DEV)]), mc, DEV, True, False, 3)
        met = evaluate(Fixed([logits.to(DEV)]), mc, DEV, True, False, 3, objects={})
    assert {k: met[k] for k in plain} == plain and list(met) == list(plain) + list(o.KEYS)
    assert {k: met[k] for k in o.KEYS} == ref.class_mean([ref.counts(p, t, c_, 8, 3) for c_ in (1, 2)])
