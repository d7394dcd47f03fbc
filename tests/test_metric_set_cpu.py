"""CPU: unetseg_hip.metricset.MetricSet, what an evaluation loop holds of the optional metric families: which
families it builds and in which order, what it does with none, and that the options reach the accumulators.  No
kernel is launched."""
import pytest

from unetseg_hip import boundary, curve, objects, skeleton
from unetseg_hip.classmap import ClassCounts
from unetseg_hip.metricset import MetricSet

ALL = dict(boundary={}, skeleton={}, curve={}, objects={})


@pytest.mark.parametrize("on", [(), ("boundary",), ("objects", "boundary"), ("curve", "skeleton"),
                                ("objects", "curve"), ("boundary", "skeleton", "objects"),
                                ("boundary", "skeleton", "curve", "objects")])
def test_keys_follow_the_fixed_order(on):
    ms = MetricSet(**{name: {} for name in on})  # whatever order the caller names them in
    order = [(name, mod.KEYS) for name, mod in (("boundary", boundary), ("skeleton", skeleton), ("curve", curve),
                                                ("objects", objects)) if name in on]
    assert ms.keys == tuple(keys for _, keys in order)
    assert list(ms.metrics()) == [k for _, keys in order for k in keys]
    assert (ms.curve is not None) == ("curve" in on)


def test_curve_keys_with_a_threshold():
    ms = MetricSet(curve={"bins": 100, "threshold": 0.3}, objects={})
    assert ms.keys == (curve.KEYS + curve.KEYS_AT, objects.KEYS)
    assert list(ms.metrics()) == list(curve.KEYS + curve.KEYS_AT + objects.KEYS)


def test_the_empty_set_touches_nothing():
    ms = MetricSet()
    ms.add(object(), object())  # neither argument is looked at
    assert ms.metrics() == {} and ms.keys == () and ms.curve is None and ms.accs == []
    assert MetricSet(None, None, None, None, (1, 2), 3).metrics() == {}


def test_full_set_before_any_batch():
    ms = MetricSet(**ALL)
    want = {}
    for acc in (boundary.Accumulator({}), skeleton.Accumulator({}), curve.Accumulator({}), objects.Accumulator({})):
        want.update(acc.metrics())
    got = ms.metrics()
    assert got == want and list(got) == list(want)
    assert list(got) == list(boundary.KEYS + skeleton.KEYS + curve.KEYS + objects.KEYS)
    assert all(a.out is None for a in ms.accs)  # nothing was allocated, let alone launched


def test_curve_given_as_an_accumulator_is_kept():
    acc = curve.Accumulator({"bins": 100})
    ms = MetricSet(curve=acc, objects={}, ignore_index=7)
    assert ms.curve is acc and ms.accs[0] is acc and acc.ignore_index is None  # taken as it is
    assert MetricSet(curve={"bins": 100}, ignore_index=7).curve.ignore_index == 7


def test_options_classes_and_ignore_index_arrive():
    ms = MetricSet({"tolerance": 3.0, "K": 100}, {"max_passes": 5}, {"bins": 50, "ece_bins": 5},
                   {"connectivity": 4, "min_area": 9}, classes=range(1, 3), ignore_index=3)
    b, s, c, o = ms.accs
    assert [type(a).__module__ for a in ms.accs] == ["unetseg_hip.boundary", "unetseg_hip.skeleton",
                                                     "unetseg_hip.curve", "unetseg_hip.objects"]
    assert (b.tolerance, b.K, b.biou_d, s.max_passes, c.K, c.ece_bins, o.connectivity, o.min_area) == \
        (3.0, 100, None, 5, 50, 5, 4, 9)
    for a in (b, s, o):
        assert isinstance(a, ClassCounts) and a.classes == (1, 2) and a.ignore_index == 3 and a.out is None
    assert c.ignore_index == 3 and not isinstance(c, ClassCounts)
    assert (b.N, s.N, o.N) == (2 * (100 + 2) + 2, 6, objects.N_COUNTS)


@pytest.mark.parametrize("family", ["boundary", "skeleton", "curve", "objects"])
def test_unknown_options_name_their_family(family):
    with pytest.raises(ValueError, match=f"unknown {family} options \\['nonsense'\\]"):
        MetricSet(**{family: {"nonsense": 1}})
    with pytest.raises(ValueError, match=f"unknown {family} options"):
        MetricSet(**{**ALL, family: {"nonsense": 1}})


def test_class_checks_of_the_families_still_hold():
    with pytest.raises(ValueError, match="ignore_index"):
        MetricSet(skeleton={}, classes=(1, 2), ignore_index=2)
    with pytest.raises(ValueError, match="class"):
        MetricSet(objects={}, classes=(0,))
    assert MetricSet(boundary={}, classes=(0,)).accs[0].classes == (0,)  # the boundary counts take any class value
