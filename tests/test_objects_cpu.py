"""CPU: the object-level reference (tests/objects_ref.py), the host code of unetseg_hip/objects.py and the flags of
val.py and train.py.  No kernel is launched; the tile queries are host-only calls of the built library."""
import os

import numpy as np
import pytest

import objects_ref as ref


def _o():
    from unetseg_hip import objects

    return objects


def _rect(H, W, *boxes):
    a = np.zeros((H, W), np.int32)
    for y0, x0, y1, x1 in boxes:
        a[y0:y1, x0:x1] = 1
    return a


MATCH_KEYS = ("PQ", "SQ", "Object F1", "Object Precision", "Object Recall", "Object F1@[.5:.95]", "Detection Recall",
              "Split Rate", "Merge Rate")


def test_identical_maps_score_one():
    a = _rect(20, 30, (1, 1, 5, 6), (8, 10, 15, 12), (17, 20, 19, 29))
    for conn in (4, 8):
        c = ref.counts(a, a, 1, conn)
        assert c[:6] == [3, 3, 3, 3, 0, 0] and c[6:16] == [3] * 10 and c[16] == 3 << 32 and c[17:] == [3, 0, 1]
        m = ref.metrics(c)
        assert m["PQ"] == m["SQ"] == m["Object F1"] == m["Object F1@[.5:.95]"] == 1.0
        assert m["Object Precision"] == m["Object Recall"] == m["Detection Recall"] == 1.0
        assert m["False Object Rate"] == m["Split Rate"] == m["Merge Rate"] == 0.0


def test_disjoint_and_empty_maps_score_zero():
    a, b = _rect(10, 10, (0, 0, 3, 3)), _rect(10, 10, (5, 5, 9, 9))
    zero = np.zeros((10, 10), np.int32)
    for p, t, n_gt, n_pred in ((a, b, 1, 1), (a, zero, 0, 1), (zero, b, 1, 0), (zero, zero, 0, 0)):
        c = ref.counts(p, t)
        assert c == [n_gt, n_pred] + [0] * 17 + [1]
        m = ref.metrics(c)
        assert all(m[k] == 0.0 for k in MATCH_KEYS)
        # every predicted object is spurious; without a predicted object there is no rate
        assert m["False Object Rate"] == (1.0 if n_pred else 0.0)


def test_iou_of_exactly_one_half_is_no_match():
    t, p = _rect(6, 6, (2, 2, 3, 4)), _rect(6, 6, (2, 1, 3, 5))  # 2 pixels inside 4: inter 2, union 4
    c = ref.counts(p, t)
    assert c[:6] == [1, 1, 1, 1, 0, 0] and c[6:17] == [0] * 11 and c[17] == 1
    assert ref.pairs(p, t).tolist() == [[0, 13, 14, 2, 4, 2]]
    c = ref.counts(_rect(6, 6, (2, 1, 3, 4)), t)  # 3 pixels: inter 2, union 3
    assert c[6:10] == [1, 1, 1, 1] and c[10:16] == [0] * 6 and c[16] == (2 << 32) // 3


def test_both_sides_of_every_threshold():
    """a bar of m of the 20 pixels of the target bar has IoU m / 20: over k / 20 iff m > k"""
    t = _rect(3, 24, (1, 2, 2, 22))
    for m in range(9, 21):
        c = ref.counts(_rect(3, 24, (1, 2, 2, 2 + m)), t)
        assert c[6:16] == [int(m > k) for k in range(10, 20)], m
        assert c[16] == ((m << 32) // 20 if m > 10 else 0)
    # the same from the other side: the prediction is the larger one
    p = _rect(3, 44, (1, 2, 2, 42))
    for m in range(19, 41):
        c = ref.counts(p, _rect(3, 44, (1, 2, 2, 2 + m)))
        assert c[6:16] == [int(20 * m > k * 40) for k in range(10, 20)], m


def test_merge_and_split():
    squares = _rect(12, 20, (2, 2, 6, 6), (2, 12, 6, 16))
    bar = _rect(12, 20, (3, 1, 5, 18))
    c = ref.counts(bar, squares)
    assert c[:6] == [2, 1, 2, 1, 0, 1] and c[17] == 2
    c = ref.counts(squares, bar)
    assert c[:6] == [1, 2, 1, 2, 1, 0] and c[17] == 2
    m = ref.metrics(c)
    assert m["Split Rate"] == 1.0 and m["Merge Rate"] == 0.0 and m["Detection Recall"] == 1.0


def test_connectivity_and_ignore_index():
    diag = np.eye(4, dtype=np.int32)
    assert ref.counts(diag, diag, 1, 8)[:2] == [1, 1] and ref.counts(diag, diag, 1, 4)[:2] == [4, 4]
    t = _rect(5, 9, (1, 1, 4, 8))
    t[:, 4] = 7  # an ignored column cuts the target and the prediction in two
    p = _rect(5, 9, (1, 1, 4, 8))
    assert ref.counts(p, t, 1, 8, 7)[:6] == [2, 2, 2, 2, 0, 0]
    assert ref.counts(p, t, 1, 8)[:6] == [2, 1, 2, 1, 0, 1]


def test_batch_is_the_sum_of_its_images():
    maps = [ref.flip_noise(20, 23, 0.41, 0.1, s) for s in (1, 2, 3)]
    one = [ref.counts(p, t) for p, t in maps]
    both = ref.counts(np.stack([p for p, _ in maps]), np.stack([t for _, t in maps]))
    assert both == [sum(v) for v in zip(*one)] and both[19] == 3


def test_metrics_from_counts_by_hand():
    o = _o()
    c = [4, 5, 3, 4, 1, 1, 2, 2, 1, 1, 1, 0, 0, 0, 0, 0, 3 << 31, 6, 0, 2]
    m = o.metrics_from_counts(c)
    assert tuple(m) == o.KEYS == ref.KEYS
    # tp 2, fp 3, fn 2, S 1.5
    assert m["Object Precision"] == 2 / 5 and m["Object Recall"] == 2 / 4 and m["Object F1"] == 4 / 9
    assert m["SQ"] == 0.75 and m["PQ"] == 1.5 / 4.5
    assert m["Object F1@[.5:.95]"] == (4 / 9 + 4 / 9 + 2 / 9 + 2 / 9 + 2 / 9) / 10
    assert m["Detection Recall"] == 3 / 4 and m["False Object Rate"] == 1 - 4 / 5
    assert m["Split Rate"] == 1 / 4 and m["Merge Rate"] == 1 / 5
    assert m == ref.metrics(c)
    assert o.metrics_from_counts(np.array(c)) == m
    zero = o.metrics_from_counts([0] * 20)
    assert all(v == 0.0 for v in zero.values()) and zero == ref.metrics([0] * 20)
    rng = np.random.default_rng(0)
    for _ in range(20):
        r = sorted(rng.integers(0, 50, 10).tolist(), reverse=True)
        c = [60, 70, 55, 52, 3, 4] + r + [int(rng.integers(0, r[0] + 1)) << 31, 80, 0, 4]
        assert o.metrics_from_counts(c) == ref.metrics(c)


def test_metrics_from_counts_refuses_dropped_insertions_and_wrong_lengths():
    o = _o()
    c = [1] * 20
    with pytest.raises(RuntimeError, match="found no slot"):
        o.metrics_from_counts(c)
    c[18] = 0
    o.metrics_from_counts(c)
    for n in (0, 6, 19, 21):
        with pytest.raises(ValueError, match="entries"):
            o.metrics_from_counts([0] * n)


def test_accumulator_options():
    o = _o()
    a = o.Accumulator({})
    assert (a.connectivity, a.min_area, a.classes) == (8, 0, (1,))
    a = o.Accumulator({"connectivity": 4, "min_area": 9}, classes=(1, 2, 3), ignore_index=4)
    assert (a.connectivity, a.min_area, a.classes, a.ignore_index) == (4, 9, (1, 2, 3), 4)
    assert a.metrics() == dict.fromkeys(o.KEYS, 0.0)  # nothing added: no launch, all zeros
    with pytest.raises(ValueError, match="unknown objects options"):
        o.Accumulator({"min_size": 3})
    with pytest.raises(ValueError, match="connectivity"):
        o.Accumulator({"connectivity": 6})
    with pytest.raises(ValueError, match="min_area"):
        o.Accumulator({"min_area": -1})
    with pytest.raises(ValueError, match="class"):
        o.Accumulator({}, classes=(0,))
    with pytest.raises(ValueError, match="class"):
        o.Accumulator({}, classes=(256,))
    with pytest.raises(ValueError, match="ignore_index"):
        o.Accumulator({}, classes=(1, 2), ignore_index=2)


def test_entry_point_flags_default_to_off():
    import train
    import val

    for mod in (val, train):
        a = mod.parse_args([])
        assert (a.object_metrics, a.object_connectivity, a.object_min_area) == (False, 8, 0)
        a = mod.parse_args(["--object-metrics", "--object-connectivity", "4", "--object-min-area", "12"])
        assert (a.object_metrics, a.object_connectivity, a.object_min_area) == (True, 4, 12)
        for bad in (["--object-connectivity", "6"], ["--object-min-area", "-2"]):
            with pytest.raises(SystemExit):
                mod.parse_args(bad)
    assert val.metric_options(val.parse_args([]))["objects"] is None
    assert val.metric_options(val.parse_args(["--object-metrics", "--object-min-area", "5"]))["objects"] == \
        {"connectivity": 8, "min_area": 5}


def test_evaluate_loops_take_the_option():
    import inspect

    from utils import train_and_eval as te

    for fn in (te.evaluate_multitask, te.evaluate):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "objects" and params[-1].default is None
    # evaluate_binary keeps the loss-term arguments last (tests/test_cldice_cpu.py): the option stands with the
    # other metric options, after `curve`
    names = list(inspect.signature(te.evaluate_binary).parameters)
    assert names[names.index("curve") + 1] == "objects" and names[-2:] == ["cldice_weight", "cldice_iters"]
    assert inspect.signature(te.evaluate_binary).parameters["objects"].default is None
    from unetseg_hip.metricset import MetricSet

    assert te.MetricSet is MetricSet  # what the three loops build
    assert MetricSet(None, None).accs == [] and MetricSet(None, None, objects=None).accs == []
    accs = MetricSet(None, {}, None, {"connectivity": 4}, (1, 2), 3).accs
    assert [type(a).__module__ for a in accs] == ["unetseg_hip.skeleton", "unetseg_hip.objects"]
    assert accs[1].classes == (1, 2) and accs[1].ignore_index == 3 and accs[1].connectivity == 4


def test_capacity_claim_on_every_gpu_test_map():
    """the pair table has at least H W slots, and no test map has more than ceil(H W / 2) distinct pairs; the
    checkerboard at connectivity 4 reaches the bound"""
    from unetseg_hip import ccl, lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built (run __graft_entry__.build())")
    o = _o()
    tw, th = o.tile()
    assert tw == 64 and th >= 1  # a wave takes a 64-pixel row segment
    seen = 0
    for name, p, t, conn, c, ign in ref.all_maps([ccl.tile(), (tw, th)]):
        H, W = p.shape[-2:]
        k = ref.distinct_pairs(p, t, c, conn, ign)
        assert k <= (H * W + 1) // 2, name
        if name.startswith("checkerboard") and conn == 4:
            assert k == (H * W + 1) // 2
        seen += 1
    assert seen > 80
    # the workspace: a table of the smallest power of two >= max(H W, 2) slots per image
    at = (__import__("ctypes").c_int64 * 6)()
    for N, H, W in ((1, 1, 1), (3, 65, 65), (2, 64, 64), (1, 37, 130)):
        lib.lib.objects_layout(N, H, W, __import__("ctypes").addressof(at))
        cap = at[5]
        assert cap >= max(H * W, 2) and cap & (cap - 1) == 0 and cap // 2 < max(H * W, 2)
        assert at[0] == 0 and at[0] < at[1] < at[2] < at[3] < at[4] < o.workspace_bytes(N, H, W)
        assert at[3] - at[2] >= 8 * N * cap and at[4] - at[3] >= 4 * N * cap + 4
    assert o.workspace_bytes(0, 4, 4) == 0 and o.workspace_bytes(1, 1 << 16, 1 << 16) == 0


def test_flip_noise_cases_say_something():
    """over the flip-noise cases the reference finds matches, loses some at 0.95, and sees splits and merges"""
    tp50 = tp95 = splits = merges = 0
    for H, W in ref.FLIP_SHAPES:
        for k, (d, f, conn) in enumerate(ref.FLIP_CASES):
            c = ref.counts(*ref.flip_noise(H, W, d, f, 50 + k), 1, conn)
            assert c[6] > 0, (H, W, d, f, conn)
            tp50, tp95, splits, merges = tp50 + c[6], tp95 + c[15], splits + c[4], merges + c[5]
    assert tp50 > 0 and tp95 < tp50 and splits > 0 and merges > 0
