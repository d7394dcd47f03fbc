"""CPU: the thinning rule's reference (tests/skeleton_ref.py) against scipy's component labelling and against
maps worked out by hand, the metric arithmetic of unetseg_hip/skeleton.py, and the argument checks of the
skeleton entry points of the built library (no device is touched: every check fails before a launch)."""
import ctypes
import os

import numpy as np
import pytest
from scipy import ndimage

import skeleton_ref as ref

EIGHT = np.ones((3, 3), int)


def _fg_components(a, c):
    return ndimage.label(a == c, structure=EIGHT)[1]


def _bg_components(a):
    return ndimage.label(np.pad(a, 1) == 0)[1]  # 4-connected; the pad joins everything that touches the frame


def _check_topology(a):
    sk, passes, unconverged = ref.thin_image(a)
    assert unconverged == 0
    assert passes <= ref.default_max_passes(*a.shape) - 4, (a.shape, passes)
    assert np.all((sk == a) | (sk == 0))  # a subset of the input, class by class
    for c in np.unique(a[a != 0]):
        assert _fg_components(sk, c) == _fg_components(a, c), (a.shape, int(c))
    # holes are the background components of each class mask (another class is not a hole of this one)
    for c in np.unique(a[a != 0]):
        assert _bg_components((sk == c).astype(int)) == _bg_components((a == c).astype(int)), (a.shape, int(c))
    again, p2, _ = ref.thin_image(sk)
    assert np.array_equal(again, sk) and p2 == 1  # idempotent: one empty pass
    return passes


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_reference_keeps_topology_small(kind):
    rng = np.random.default_rng(100 + kind)
    for size in range(1, 41):
        H, W = size, int(rng.integers(1, 41))
        _check_topology(ref.random_map(kind, H, W, rng))
        _check_topology(ref.random_map(kind, W, H, rng, classes=3))


@pytest.mark.parametrize("kind,H,W", [(0, 97, 61), (1, 140, 90), (1, 75, 140), (2, 120, 133)])
def test_reference_keeps_topology_large(kind, H, W):
    _check_topology(ref.random_map(kind, H, W, np.random.default_rng(H * 1000 + W)))


def test_pass_counts_of_full_maps_and_discs():
    for H, W in ((70, 45), (12, 12), (9, 30)):
        assert _check_topology(np.ones((H, W), np.int32)) <= (min(H, W) + 1) // 2 + 1
    for r in (3, 10, 30):
        assert _check_topology(ref.disc(2 * r + 4, r)) <= r + 2


def _thin(rows):
    a = np.array([[int(ch) for ch in r] for r in rows], np.int32)
    return ref.thin_image(a)[0]


def _is(rows):
    return np.array([[int(ch) for ch in r] for r in rows], np.int32)


def test_hand_single_pixel_and_lines():
    # a lone pixel has no neighbour: C = 0, so it is never deleted
    assert np.array_equal(_thin(["1"]), _is(["1"]))
    # an inner pixel of a one-pixel line has P8 and P4 only: C = (!P2 & P4) + (!P6 & P8) = 2.  An end pixel has
    # one neighbour: C = 1 but N1 = N2 = 1 < 2.  Nothing is deleted; the same holds turned by 90 degrees
    assert np.array_equal(_thin(["1111111"]), _is(["1111111"]))
    assert np.array_equal(_thin(["1"] * 7), _is(["1"] * 7))


def test_hand_bar_3x9():
    # first subiteration (m = (P6|P7|!P9) & P8, so a pixel needs P8 = 0, or P6 = P7 = 0 and P9 = 1, to go):
    #   top row, x = 0: P4 P5 P6 set, C = 1, N = min(2, 2) = 2, P8 = 0 -> deleted.  top row, x >= 1: P8 set and P6
    #   set -> m = 1, kept.  middle row, x = 0: P2 P3 P4 P5 P6, C = 1, N = 3, P8 = 0 -> deleted; x >= 1 inner: C = 0.
    #   middle row, x = 8: P2 P9 P8 P7 P6: m = 1 kept.  bottom row, x = 0: P2 P3 P4: C = 1, N = 2, P8 = 0 -> deleted.
    #   bottom row, x >= 1: P6 = P7 = 0, P9 = 1, P8 = 1: m = (0|0|0) & 1 = 0; x in 1..7: P8 P9 P2 P3 P4, C = 1, N = 3 ->
    #   deleted; x = 8: P8 P9 P2: C = 1, N = 2 -> deleted.  Left: the top row x = 1..8 and the middle row x = 1..8.
    # second subiteration (m = (P2|P3|!P5) & P4) on that 2 x 8 block: top row x = 1..7: P4 set, P2 = P3 = 0, P5 set ->
    #   m = 0; x = 1: P4 P5 P6, C = 1, N = 2 -> deleted; x = 2..7: P8 P7 P6 P5 P4, C = 1, N = 3 -> deleted; x = 8: P8 P7
    #   P6: C = 1, N = 2, P4 = 0 -> m = 0 -> deleted.  middle row: x = 1..7 have P2|P3 and P4 -> m = 1, kept; x = 8: P4 = 0,
    #   P9 P2 P8, C = 1, N = 2 -> deleted.  Left after pass 1: the middle row, x = 1..7, a line that stays.
    assert np.array_equal(_thin(["111111111"] * 3), _is(["000000000", "011111110", "000000000"]))


def test_hand_square_2x2():
    # first subiteration: (0,0) has P4 P5 P6: C = 1, N1 = (P3|P4) + (P5|P6) = 2, N2 = (P4|P5) + (P6|P7) = 2, P8 = 0 ->
    # deleted.  (0,1): P8 P7 P6, P8 = 1 and P6 = 1 -> m = 1, kept.  (1,0): P2 P3 P4: C = 1, N = 2, P8 = 0 -> deleted.
    # (1,1): P8 P9 P2: m = (0|0|!1) & 1 = 0, C = 1, N = 2 -> deleted.  Left: (0,1) alone, which stays.
    assert np.array_equal(_thin(["11", "11"]), _is(["01", "00"]))


def test_hand_plus_sign():
    # arms one pixel wide: an arm's inner pixel has two opposite neighbours (C = 2), an arm's end one (N = 1), the
    # centre four (C = 4).  Nothing is deleted.
    plus = ["0000000", "0001000", "0001000", "0111110", "0001000", "0001000", "0000000"]
    assert np.array_equal(_thin(plus), _is(plus))


def test_hand_diagonal_ring_keeps_its_hole():
    # the one-pixel ring around a hole: every pixel has two diagonal neighbours that are not adjacent to each other,
    # e.g. the top pixel P7 and P5: C = (!P4 & (P5|P6)) + (!P6 & (P7|P8)) = 2.  Unchanged, the hole stays
    ring = ["00000", "00100", "01010", "00100", "00000"]
    assert np.array_equal(_thin(ring), _is(ring))
    big = ["0001000", "0010100", "0100010", "1000001", "0100010", "0010100", "0001000"]
    assert np.array_equal(_thin(big), _is(big))
    assert _bg_components(_thin(big)) == 2


def test_hand_two_classes_side_by_side():
    # a neighbour of another class does not count: each 4 x 4 block is thinned as if the other were background
    both = _is(["11112222"] * 4)
    left, right = _is(["11110000"] * 4), _is(["00002222"] * 4)
    want = ref.thin_image(left)[0] + ref.thin_image(right)[0]
    assert np.array_equal(ref.thin_image(both)[0], want)
    assert (want == 1).sum() >= 1 and (want == 2).sum() >= 1
    # and a class value outside 1 .. 255 is background
    assert np.array_equal(ref.thin_image(_is(["11", "11"]) * 256)[0], np.zeros((2, 2), np.int32))


def test_max_passes_and_unconverged_of_the_reference():
    full = np.ones((70, 45), np.int32)
    sk0, p0, u0 = ref.thin_image(full, 0)
    assert np.array_equal(sk0, full) and p0 == 0 and u0 == 0  # no pass runs, nothing is reported
    _, p1, u1 = ref.thin_image(full, 1)
    assert p1 == 1 and u1 == 1
    _, p, u = ref.thin_image(full)
    assert u == 0 and p < ref.default_max_passes(70, 45)
    _, pe, ue = ref.thin_image(full, p - 1)
    assert pe == p - 1 and ue == 1  # the empty pass was cut off
    _, pe, ue = ref.thin_image(full, p)
    assert ue == 0


def test_metrics_from_counts():
    from unetseg_hip import skeleton

    assert skeleton.KEYS == ("clDice", "Skeleton Precision", "Skeleton Recall")
    assert skeleton.default_max_passes(70, 45) == 30 == ref.default_max_passes(70, 45)
    m = skeleton.metrics_from_counts([3, 4, 1, 2, 0, 5])
    assert m["Skeleton Precision"] == 0.75 and m["Skeleton Recall"] == 0.5
    assert m["clDice"] == pytest.approx(2 * 0.75 * 0.5 / 1.25, rel=1e-15)
    assert m == ref.metrics_from_counts([3, 4, 1, 2, 0, 5])
    # both skeletons empty: a perfect score; one empty: that side 0, the other its share (0 of something), clDice 0
    assert skeleton.metrics_from_counts([0, 0, 0, 0, 0, 1]) == {"clDice": 1.0, "Skeleton Precision": 1.0,
                                                                "Skeleton Recall": 1.0}
    assert skeleton.metrics_from_counts([0, 0, 0, 7, 0, 1]) == {"clDice": 0.0, "Skeleton Precision": 0.0,
                                                                "Skeleton Recall": 0.0}
    assert skeleton.metrics_from_counts([0, 7, 0, 0, 0, 1]) == {"clDice": 0.0, "Skeleton Precision": 0.0,
                                                                "Skeleton Recall": 0.0}
    # zero sum: both skeletons there, neither inside the other's mask
    assert skeleton.metrics_from_counts([0, 5, 0, 9, 0, 2])["clDice"] == 0.0
    with pytest.raises(RuntimeError, match=r"2 of 3 images.*max_passes"):
        skeleton.metrics_from_counts([1, 1, 1, 1, 2, 3])
    with pytest.raises(ValueError):
        skeleton.metrics_from_counts([1, 2, 3])
    for c in ([3, 4, 1, 2, 0, 5], [0, 0, 0, 7, 0, 1], [9, 9, 4, 4, 0, 1]):
        assert skeleton.metrics_from_counts(np.array(c)) == ref.metrics_from_counts(c)


def test_accumulator_options_checked_without_device():
    from unetseg_hip import skeleton

    with pytest.raises(ValueError, match="unknown skeleton options"):
        skeleton.Accumulator({"passes": 3})
    with pytest.raises(ValueError, match="max_passes"):
        skeleton.Accumulator({"max_passes": -1})
    with pytest.raises(ValueError, match="class"):
        skeleton.Accumulator({}, classes=(0,))
    with pytest.raises(ValueError, match="ignore_index"):
        skeleton.Accumulator({}, classes=(1, 2), ignore_index=2)
    acc = skeleton.Accumulator({}, classes=(1, 2))
    assert acc.metrics() == dict.fromkeys(skeleton.KEYS, 0.0)  # nothing added: no class has a target skeleton
    assert skeleton.Accumulator({"max_passes": 5}).metrics()["clDice"] == 1.0


def test_argument_errors_reported_without_device():
    """every bad argument of the skeleton entry points is refused by the loaded library before any HIP call; the
    host-only queries answer"""
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    raw = lib.load()
    tw, th, k = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert raw.unetseg_skel_tile(ctypes.byref(tw), ctypes.byref(th), ctypes.byref(k)) == 0
    assert tw.value > 0 and th.value > 0 and k.value > 0
    assert raw.unetseg_skel_tile(None, ctypes.byref(th), ctypes.byref(k)) != 0
    assert b"skel_tile" in raw.unetseg_last_error()
    size = raw.unetseg_skel_workspace(2, 70, 45)
    assert size >= 2 * 2 * 70 * 45  # two byte maps at least
    assert raw.unetseg_skel_workspace(0, 70, 45) == 0 and raw.unetseg_skel_workspace(2, -1, 45) == 0
    assert raw.unetseg_skel_workspace(2, 70, 0) == 0

    A, B, WS = 0x1000, 0x2000, 0x4000  # never dereferenced: every call below fails its checks

    def thin(cls=A, N=2, H=70, W=45, passes=3, out=B, unc=None, ws=WS, ws_bytes=size):
        return raw.unetseg_skel_thin(cls, N, H, W, passes, out, unc, ws, ws_bytes, None)

    for bad, word in ((dict(cls=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                      (dict(N=0), b"shape"), (dict(H=0), b"shape"), (dict(W=-3), b"shape"),
                      (dict(passes=-1), b"max_passes"), (dict(ws_bytes=size - 1), b"workspace"),
                      (dict(ws_bytes=0), b"workspace"), (dict(ws=WS + 4), b"aligned")):
        assert thin(**bad) != 0, bad
        msg = raw.unetseg_last_error()
        assert b"skel_thin" in msg and word in msg, (bad, msg)

    def counts(ptrs=(A, A, A, A, A, A), N=2, H=70, W=45, c=1, ignore=-1, out=B):
        return raw.unetseg_skel_counts(*ptrs, N, H, W, c, ignore, out, None)

    for i in range(6):
        ptrs = tuple(None if j == i else A for j in range(6))
        assert counts(ptrs=ptrs) != 0 and b"null" in raw.unetseg_last_error()
    for bad, word in ((dict(out=None), b"null"), (dict(N=0), b"shape"), (dict(H=-1), b"shape"), (dict(W=0), b"shape"),
                      (dict(c=0), b"class"), (dict(c=-2), b"class"), (dict(c=256), b"class"),
                      (dict(c=2, ignore=2), b"ignore")):
        assert counts(**bad) != 0, bad
        msg = raw.unetseg_last_error()
        assert b"skel_counts" in msg and word in msg, (bad, msg)
    with pytest.raises(RuntimeError, match="skel_thin.*max_passes"):
        lib.lib.skel_thin(A, 2, 70, 45, -1, B, None, WS, size, None)
