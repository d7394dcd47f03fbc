"""CPU: the boundary reference and the host side of the feature (csrc/boundary.hip,
unetseg_hip/boundary.py, the boundary flags of val.py).

* tests/boundary_ref.py (the reference the GPU tests hold the kernels to, integer for integer) against
  scipy's exact Euclidean distance transform and against maps whose edges, counts and metrics are
  written out by hand, the frame rule and the ignore rule among them;
* ``metrics_from_counts`` of the package and of the reference on the corner cases;
* the C ABI's argument checks, which refuse before any HIP call.
"""
import math
import os

import numpy as np
import pytest

import boundary_ref

PTR = 4096  # a non-null pointer value; every call below is refused before it is used
A = lambda rows: np.array(rows, np.int32)  # noqa: E731


# ---- 1. the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (17, 31), (64, 65), (97, 33)])
@pytest.mark.parametrize("density", [0.001, 0.02, 0.3, 1.0])
def test_reference_sqdist_equals_scipy(shape, density):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(shape[0] * 1000 + shape[1])
    s = g.random(shape) < density
    s[g.integers(shape[0]), g.integers(shape[1])] = True  # scipy has no answer for an image without a site
    want = np.rint(ndimage.distance_transform_edt(~s) ** 2).astype(np.int64)
    assert np.array_equal(boundary_ref.sqdist(s), want)


def test_reference_sqdist_by_hand():
    s = np.zeros((3, 4), np.uint8)
    assert np.array_equal(boundary_ref.sqdist(s), np.full((3, 4), boundary_ref.INF))
    s[0, 0] = 1
    assert np.array_equal(boundary_ref.sqdist(s), A([[0, 1, 4, 9], [1, 2, 5, 10], [4, 5, 8, 13]]))
    s[2, 3] = 1
    assert np.array_equal(boundary_ref.sqdist(s), A([[0, 1, 4, 4], [1, 2, 2, 1], [4, 4, 1, 0]]))
    both = boundary_ref.sqdist(np.stack([s, np.zeros_like(s)]))  # nothing leaks across the batch
    assert np.array_equal(both[0], boundary_ref.sqdist(s)) and (both[1] == boundary_ref.INF).all()
    assert boundary_ref.sqdist(s).dtype == np.int32 and boundary_ref.INF == 1 << 30


SQUARE = A([[0, 0, 0, 0, 0],
            [0, 1, 1, 1, 0],
            [0, 1, 1, 1, 0],
            [0, 1, 1, 1, 0],
            [0, 0, 0, 0, 0]])


def test_edges_of_a_square():
    ring = SQUARE.copy()
    ring[2, 2] = 0  # the centre has four neighbours of its own class
    assert np.array_equal(boundary_ref.edges(SQUARE, 1), ring)
    around = A([[0, 1, 1, 1, 0],
                [1, 0, 0, 0, 1],
                [1, 0, 0, 0, 1],
                [1, 0, 0, 0, 1],
                [0, 1, 1, 1, 0]])  # the corners touch the square by a diagonal only
    assert np.array_equal(boundary_ref.edges(SQUARE, 0), around)
    assert not boundary_ref.edges(SQUARE, 2).any()
    assert boundary_ref.edges(SQUARE, 1).dtype == np.uint8


def test_the_image_frame_is_no_boundary():
    assert not boundary_ref.edges(np.ones((5, 5), np.int32), 1).any()
    m = np.zeros((5, 5), np.int32)
    m[:2, :2] = 1
    want = np.zeros((5, 5), np.int32)
    want[0, 1] = want[1, 0] = want[1, 1] = 1  # (0, 0) sees its own class and the frame only
    assert np.array_equal(boundary_ref.edges(m, 1), want)


IGN = A([[1, 1, 9, 0, 0],
         [1, 1, 9, 0, 0],
         [1, 1, 1, 0, 0],
         [0, 0, 0, 0, 0],
         [0, 0, 0, 0, 0]])


def test_ignored_pixels_make_and_are_no_edge():
    want = np.zeros((5, 5), np.int32)
    want[2, :3] = 1  # (0, 1) and (1, 1) touch the ignored column only
    assert np.array_equal(boundary_ref.edges(IGN, 1, ignore=9), want)
    want[0, 1] = want[1, 1] = 1  # without the rule, 9 is one more class
    assert np.array_equal(boundary_ref.edges(IGN, 1), want)
    assert not boundary_ref.edges(IGN, 9, ignore=9).any()
    assert boundary_ref.edges(IGN, 9).sum() == 2
    zero = np.zeros((5, 5), np.int32)
    zero[2, 3] = zero[3, 0] = zero[3, 1] = zero[3, 2] = 1  # (0, 3) and (1, 3) touch the ignored column only
    assert np.array_equal(boundary_ref.edges(IGN, 0, ignore=9), zero)


def _squares7():
    t = np.zeros((7, 7), np.int32)
    t[2:5, 2:5] = 1
    p = np.zeros((7, 7), np.int32)
    p[2:5, 3:6] = 1  # the target one pixel to the right
    return p, t


def test_counts_and_metrics_of_a_shifted_square_by_hand():
    p, t = _squares7()
    K = 16
    c = boundary_ref.counts(p, t, 1, K, biou_d=1)
    want = np.zeros(2 * (K + 2) + 2, np.int64)
    want[0], want[1] = 4, 4            # prediction ring: 4 pixels on the target ring, 4 one pixel off
    want[K + 2], want[K + 3] = 4, 4    # and the same seen from the target
    want[2 * K + 4], want[2 * K + 5] = 6, 12  # both bands are the whole squares: 3 x 2 shared, 3 x 4 covered
    assert np.array_equal(c, want)
    c0 = boundary_ref.counts(p, t, 1, K, biou_d=0)  # the bands are the rings: 4 shared pixels, 12 in all
    assert (c0[2 * K + 4], c0[2 * K + 5]) == (4, 12) and np.array_equal(c0[:2 * K + 4], want[:2 * K + 4])
    m = boundary_ref.metrics_from_counts(c, K, tolerance=0.0)
    assert (m["Boundary Precision"], m["Boundary Recall"], m["Boundary F1"]) == (0.5, 0.5, 0.5)
    assert m["Boundary IoU"] == 0.5 and m["HD95"] == 1.0
    m = boundary_ref.metrics_from_counts(c, K, tolerance=1.0)
    assert (m["Boundary Precision"], m["Boundary Recall"], m["Boundary F1"]) == (1.0, 1.0, 1.0)


def test_counts_with_an_ignored_target_pixel_by_hand():
    p, t = _squares7()
    t[3, 5] = 9  # right of the target square, inside the prediction
    K = 16
    c = boundary_ref.counts(p, t, 1, K, biou_d=1, ignore=9)
    # (3, 4) of the target ring sees its own class and the ignored pixel only: 7 target edge pixels; the
    # prediction's (3, 5) is now sqrt(2) from the target edge, and out of the prediction's band
    assert c[:4].tolist() == [4, 3, 1, 0]
    assert c[K + 2:K + 5].tolist() == [4, 3, 0]
    assert (c[2 * K + 4], c[2 * K + 5]) == (6, 11)
    assert c.sum() == 8 + 7 + 17


def test_counts_overflow_bin_and_empty_sides():
    p, t = _squares7()
    K = 16
    e = boundary_ref.counts(np.zeros_like(p), t, 1, K, biou_d=1)
    assert e[:K + 2].sum() == 0 and e[K + 2:2 * K + 4].tolist() == [0] * (K + 1) + [8]
    assert (e[2 * K + 4], e[2 * K + 5]) == (0, 9)
    far_p, far_t = np.zeros((3, 12), np.int32), np.zeros((3, 12), np.int32)
    far_p[1, 1], far_t[1, 10] = 1, 1  # 9 pixels apart: 81 > K
    f = boundary_ref.counts(far_p, far_t, 1, K, biou_d=1)
    assert f[K + 1] == 1 and f[2 * K + 3] == 1 and f.sum() == 2 + 0 + 2
    one = boundary_ref.counts(p, t, 1, K, biou_d=1)
    assert np.array_equal(boundary_ref.counts(np.stack([p, np.zeros_like(p)]), np.stack([t, t]), 1, K, biou_d=1),
                          one + e)  # a batch adds up, image by image


def test_default_band_width_is_two_percent_of_the_diagonal():
    assert boundary_ref.default_biou_d(512, 512) == 14  # 0.02 * 724.08
    assert boundary_ref.default_biou_d(10, 10) == 1
    assert boundary_ref.default_biou_d(4096, 6144) == 64  # 147.7 clamped to sqrt(K)
    assert boundary_ref.default_biou_d(4096, 6144, K=16) == 4


# ---- 2. metrics_from_counts: the package's against the reference's ---------------------------------------
def _both(c, K, tol=2.0):
    from unetseg_hip import boundary

    got = boundary.metrics_from_counts(c, K, tol)
    assert got == boundary_ref.metrics_from_counts(c, K, tol)
    assert tuple(got) == boundary.KEYS
    return got


def _arr(K, hp=(), hg=(), inter=0, union=0):
    c = np.zeros(2 * (K + 2) + 2, np.int64)
    for b, n in hp:
        c[b] = n
    for b, n in hg:
        c[K + 2 + b] = n
    c[2 * K + 4], c[2 * K + 5] = inter, union
    return c


def test_metrics_both_sides_empty():
    m = _both(_arr(16), 16)
    assert m == {"Boundary Precision": 1.0, "Boundary Recall": 1.0, "Boundary F1": 1.0, "Boundary IoU": 1.0,
                 "HD95": 0.0}


def test_metrics_one_side_empty():
    K = 16
    m = _both(_arr(K, hg=[(K + 1, 5)], union=9), K)  # no prediction edge: the target's pixels overflow
    assert (m["Boundary Precision"], m["Boundary Recall"], m["Boundary F1"]) == (0.0, 0.0, 0.0)
    assert m["Boundary IoU"] == 0.0 and m["HD95"] == math.inf
    m = _both(_arr(K, hp=[(K + 1, 3)], union=4), K)
    assert (m["Boundary Precision"], m["Boundary Recall"], m["Boundary F1"]) == (0.0, 0.0, 0.0)


def test_metrics_hd95():
    K = 16
    assert _both(_arr(K, hp=[(0, 19), (9, 1)]), K)["HD95"] == 0.0          # 19 of 20 is 95 % exactly
    assert _both(_arr(K, hp=[(0, 18), (4, 1)], hg=[(9, 1)]), K)["HD95"] == 2.0
    assert _both(_arr(K, hp=[(0, 18)], hg=[(4, 1), (9, 1)]), K)["HD95"] == 2.0  # pooled, whichever side
    assert _both(_arr(K, hp=[(0, 10)], hg=[(K + 1, 10)]), K)["HD95"] == math.inf
    assert _both(_arr(K, hp=[(0, 19)], hg=[(K + 1, 1)]), K)["HD95"] == 0.0
    assert _both(_arr(K, hp=[(K, 1)]), K, 4.0)["HD95"] == 4.0                # bin K is a real distance


def test_metrics_tolerance():
    K = 16
    c = _arr(K, hp=[(0, 1), (4, 1), (5, 1), (16, 1)], hg=[(1, 2), (8, 2)], inter=3, union=4)
    m = _both(c, K, 2.0)
    assert (m["Boundary Precision"], m["Boundary Recall"], m["Boundary IoU"]) == (0.5, 0.5, 0.75)
    m = _both(c, K, 2.5)  # 6.25: bin 5 is within
    assert m["Boundary Precision"] == 0.75
    m = _both(c, K, 4.0)
    assert (m["Boundary Precision"], m["Boundary Recall"]) == (1.0, 1.0)
    from unetseg_hip import boundary

    with pytest.raises(ValueError):
        boundary.metrics_from_counts(c, K, 4.5)  # 20.25 > K
    with pytest.raises(ValueError):
        boundary.metrics_from_counts(c[:-1], K, 2.0)


def test_val_flags_round_trip():
    import val

    a = val.parse_args([])
    assert (a.boundary_metrics, a.boundary_tolerance, a.boundary_iou_d) == (False, 2.0, 0)
    assert val.metric_options(a)["boundary"] is None
    a = val.parse_args(["--boundary-metrics", "--boundary-tolerance", "3.5", "--boundary-iou-d", "7"])
    assert val.metric_options(a)["boundary"] == {"tolerance": 3.5, "biou_d": 7}
    assert val.metric_options(val.parse_args(["--boundary-metrics"]))["boundary"] == {"tolerance": 2.0, "biou_d": None}


def test_python_layer_refuses_what_is_no_gpu_map():
    import torch

    from unetseg_hip import boundary

    for bad in (None, torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            boundary.edges(bad)
        with pytest.raises(ValueError):
            boundary.sqdist(bad)
        with pytest.raises(ValueError):
            boundary.counts(bad, bad)
    assert boundary.INF == boundary_ref.INF
    for shape in ((512, 512), (10, 10), (4096, 6144), (65, 129)):
        assert boundary.default_biou_d(*shape) == boundary_ref.default_biou_d(*shape)


# ---- 3. the C ABI's argument checks ----------------------------------------------------------------------
def _raw():
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    return lib.load()


def test_argument_errors_reported_without_device():
    from unetseg_hip import lib

    raw = _raw()

    def refused(rc, *texts):
        err = raw.unetseg_last_error().decode()
        assert rc != 0 and all(t in err for t in texts), err

    # unetseg_boundary_edges(cls, N, H, W, c, ignore, edge)
    refused(raw.unetseg_boundary_edges(None, 1, 4, 4, 1, -1, PTR, None), "boundary_edges", "null")
    refused(raw.unetseg_boundary_edges(PTR, 1, 4, 4, 1, -1, None, None), "boundary_edges", "null")
    refused(raw.unetseg_boundary_edges(PTR, 1, 4, 16385, 1, -1, PTR, None), "boundary_edges", "16384")
    refused(raw.unetseg_boundary_edges(PTR, 0, 4, 4, 1, -1, PTR, None), "boundary_edges", "bad shape")
    # unetseg_edt_sqdist(sites, N, H, W, d2)
    refused(raw.unetseg_edt_sqdist(None, 1, 4, 4, PTR, None), "edt_sqdist", "null")
    refused(raw.unetseg_edt_sqdist(PTR, 1, 4, 4, None, None), "edt_sqdist", "null")
    refused(raw.unetseg_edt_sqdist(PTR, 1, 4, 16385, PTR, None), "edt_sqdist", "16384")
    refused(raw.unetseg_edt_sqdist(PTR, 1, 16385, 4, PTR, None), "edt_sqdist", "16384")
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        refused(raw.unetseg_edt_sqdist(PTR, *shape, PTR, None), "edt_sqdist", "bad shape")
    refused(raw.unetseg_edt_chunk(None), "edt_chunk", "null")
    # unetseg_boundary_counts(pred, target, eP, eG, dP, dG, N, H, W, c, ignore, K, biou_d2, counts)
    ok = [PTR] * 6 + [1, 4, 4, 1, -1, 4096, 100, PTR]
    for k in (0, 1, 2, 3, 4, 5, 13):
        args = list(ok)
        args[k] = None
        refused(raw.unetseg_boundary_counts(*args, None), "boundary_counts", "null")

    def but(**kw):
        names = ["pred", "target", "eP", "eG", "dP", "dG", "N", "H", "W", "c", "ignore", "K", "biou_d2", "counts"]
        return [kw.get(n, v) for n, v in zip(names, ok)]

    refused(raw.unetseg_boundary_counts(*but(K=65537), None), "boundary_counts", "K = 65537")
    refused(raw.unetseg_boundary_counts(*but(K=-1, biou_d2=0), None), "boundary_counts", "K = -1")
    refused(raw.unetseg_boundary_counts(*but(K=16, biou_d2=17), None), "boundary_counts", "biou_d2 = 17")
    refused(raw.unetseg_boundary_counts(*but(biou_d2=-1), None), "boundary_counts", "biou_d2 = -1")
    refused(raw.unetseg_boundary_counts(*but(W=16385), None), "boundary_counts", "16384")
    refused(raw.unetseg_boundary_counts(*but(N=0), None), "boundary_counts", "bad shape")
    with pytest.raises(RuntimeError, match="16384"):
        lib.lib.edt_sqdist(PTR, 1, 4, 16385, PTR, None)
    with pytest.raises(RuntimeError, match="biou_d2"):
        lib.lib.boundary_counts(*but(K=16, biou_d2=17), None)


def test_chunk_query_needs_no_device():
    from unetseg_hip import boundary

    _raw()
    L = boundary.chunk()
    assert L == 0 or 2 <= L <= 128  # the GPU tests' seam cases (2 L + 1 on an axis) stay small
