"""GPU: unetseg_hip.metricset.MetricSet against the four stand-alone accumulators fed by hand with the same class
map.  The counts are integers, so the merged metrics are compared with ``==``; the kernels themselves are held to
their references in the test files of the families."""
import numpy as np
import pytest
import torch

import objects_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _by_hand(accs, curve_acc, batches):
    """the stand-alone accumulators over the batches, and their metrics merged in the order given"""
    from unetseg_hip.boundary import labels_from_logits

    for z, y in batches:
        pred = labels_from_logits(z)
        for a in accs:
            if a is curve_acc:
                a.add(z, y)
            else:
                a.add(pred, y)
    want = {}
    for a in accs:
        want.update(a.metrics())
    return want


def test_binary_all_four_families_with_ignore_index():
    from unetseg_hip import boundary, curve, objects, skeleton
    from unetseg_hip.metricset import MetricSet
    from utils.synthetic import make_batch

    batches = []
    for k in range(2):
        _, y = make_batch(2, 64, seed=70 + k)
        near = torch.from_numpy(np.stack([np.roll(m, (1, 2), (0, 1)) for m in y.numpy()])).float()
        speck = (torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(k)) < 0.02).float()
        z = torch.zeros(2, 2, 64, 64)
        z[:, 1] = 8.0 * ((near + speck).clamp(max=1) - 0.5)
        hole = torch.rand(2, 64, 64, generator=torch.Generator().manual_seed(100 + k)) < 0.05
        y = torch.where(hole, torch.full_like(y, 255), y)
        assert 0.03 < hole.float().mean() < 0.07 and (y == 1).any() and (y == 0).any()
        batches.append((z.to(DEV), y.to(DEV)))
    opts = dict(boundary={"tolerance": 2.0, "biou_d": None}, skeleton={}, curve={"bins": 100},
                objects={"connectivity": 8})
    ms = MetricSet(**opts, ignore_index=255)
    for z, y in batches:
        ms.add(z, y)
    c = curve.Accumulator(opts["curve"], 255)
    accs = [boundary.Accumulator(opts["boundary"], (1,), 255), skeleton.Accumulator(opts["skeleton"], (1,), 255), c,
            objects.Accumulator(opts["objects"], (1,), 255)]
    want = _by_hand(accs, c, batches)
    got = ms.metrics()
    assert got == want
    assert list(got) == list(boundary.KEYS + skeleton.KEYS + curve.KEYS + objects.KEYS)
    for mine, theirs in zip(ms.accs, accs):
        assert type(mine) is type(theirs) and torch.equal(mine.out, theirs.out)
    # the case says something: edges, skeletons and objects on both sides, and the ignored pixels are left out
    b, s, _, o = (a.out[0].tolist() for a in accs)
    assert sum(b[:4098]) > 0 and sum(b[4098:8196]) > 0 and s[1] > 0 and s[3] > 0 and s[4] == 0 and s[5] == 4
    assert o[0] > 0 and o[1] > o[6] > 0 and o[18] == 0 and o[19] == 4
    assert int(c.out.sum()) == sum(int((y != 255).sum()) for _, y in batches) < 4 * 64 * 64
    assert 0.0 < got["Boundary F1"] < 1.0 and 0.0 < got["clDice"] < 1.0 and 0.0 < got["PQ"] < 1.0


def test_multiclass_three_families():
    from unetseg_hip import boundary, objects, skeleton
    from unetseg_hip.metricset import MetricSet

    p, t = objects_ref.multiclass(2, 64, 64, 2, 9)
    t = np.where(np.random.default_rng(10).random(t.shape) < 0.1, 3, t).astype(np.int32)
    logits = torch.full((2, 3, 64, 64), -4.0)
    logits.scatter_(1, torch.from_numpy(p).long().unsqueeze(1), 4.0)
    batches = [(logits.to(DEV), torch.from_numpy(t).long().to(DEV))]
    ms = MetricSet(boundary={}, skeleton={}, objects={}, classes=(1, 2), ignore_index=3)
    assert ms.curve is None
    ms.add(*batches[0])
    accs = [boundary.Accumulator({}, (1, 2), 3), skeleton.Accumulator({}, (1, 2), 3),
            objects.Accumulator({}, (1, 2), 3)]
    want = _by_hand(accs, None, batches)
    got = ms.metrics()
    assert got == want
    assert list(got) == list(boundary.KEYS + skeleton.KEYS + objects.KEYS)
    for mine, theirs in zip(ms.accs, accs):
        assert tuple(mine.out.shape) == (2, mine.N) and torch.equal(mine.out, theirs.out)
    for row in accs[2].out.tolist():  # both classes have target objects and matches
        assert row[0] > 0 and row[6] > 0
    assert 0.0 < got["Boundary F1"] <= 1.0 and 0.0 < got["clDice"] <= 1.0 and 0.0 < got["PQ"] < 1.0
