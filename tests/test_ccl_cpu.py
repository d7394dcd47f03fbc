"""CPU: the connected-component reference and the host side of the feature (csrc/ccl.hip,
unetseg_hip/ccl.py, the cleanup flags of predict.py).

* tests/ccl_ref.py (the reference the GPU tests hold the kernels to, bit for bit) against hand-written
  maps whose answers are typed in below, and, where scipy imports, against scipy.ndimage.label per class;
* predict.check_clean and the new command-line flags;
* every entry point refuses bad arguments before any launch, with a non-zero status and a message.
"""
import os

import numpy as np
import pytest

import ccl_ref

PTR = 4096  # a non-null pointer value; every call below is refused before it is used


def A(rows):
    return np.array(rows, np.int32)


# ---- 1. the reference against typed answers ---------------------------------------------------------
def test_checkerboard_shows_the_duality():
    board = A([[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1], [1, 0, 1, 0]])
    own = np.arange(16, dtype=np.int32).reshape(4, 4)
    # 8: the ones hang together by their corners (root: the first one, index 1), the zeros are 4-connected singletons
    assert np.array_equal(ccl_ref.label(board, 8), np.where(board == 1, 1, own))
    # 4: the flip
    assert np.array_equal(ccl_ref.label(board, 4), np.where(board == 1, own, 0))
    assert np.array_equal(ccl_ref.components(board, 8), A([[0, 1, 8, 0, 0, 3, 3]]))
    want4 = A([[0, 1, 1, y, x, y, x] for y in range(4) for x in range(4) if board[y, x]])
    assert np.array_equal(ccl_ref.components(board, 4), want4)


RINGS = A([[1, 1, 1, 1, 1, 1, 1],
           [1, 0, 0, 0, 0, 0, 1],
           [1, 0, 1, 1, 1, 0, 1],
           [1, 0, 1, 0, 1, 0, 1],
           [1, 0, 1, 1, 1, 0, 1],
           [1, 0, 0, 0, 0, 0, 1],
           [1, 1, 1, 1, 1, 1, 1]])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_nested_rings(connectivity):
    want = A([[0, 0, 0, 0, 0, 0, 0],
              [0, 8, 8, 8, 8, 8, 0],
              [0, 8, 16, 16, 16, 8, 0],
              [0, 8, 16, 24, 16, 8, 0],
              [0, 8, 16, 16, 16, 8, 0],
              [0, 8, 8, 8, 8, 8, 0],
              [0, 0, 0, 0, 0, 0, 0]])
    root = ccl_ref.label(RINGS, connectivity)
    assert np.array_equal(root, want)
    st = ccl_ref.stats(root)
    at = ccl_ref.is_root(root)
    assert np.array_equal(np.flatnonzero(at), [0, 8, 16, 24])
    assert st[:, at].T.tolist() == [[24, 6, 0, 6], [16, 5, 1, 5], [8, 4, 2, 4], [1, 3, 3, 3]]  # area ymax xmin xmax
    assert not st[0][~at].any()
    assert np.array_equal(ccl_ref.components(RINGS, connectivity), A([[0, 1, 24, 0, 0, 6, 6], [0, 1, 8, 2, 2, 4, 4]]))
    # the centre pixel is a hole of area 1, the zero ring one of area 16: the `<` is strict
    assert np.array_equal(ccl_ref.clean(RINGS, 0, 1, connectivity), RINGS)
    filled = RINGS.copy()
    filled[3, 3] = 1
    assert np.array_equal(ccl_ref.clean(RINGS, 0, 2, connectivity), filled)
    assert np.array_equal(ccl_ref.clean(RINGS, 0, 16, connectivity), filled)
    assert np.array_equal(ccl_ref.clean(RINGS, 0, 17, connectivity), np.ones_like(RINGS))
    # the inner ring has 8 pixels; without it the two holes are one of 25
    assert np.array_equal(ccl_ref.clean(RINGS, 8, 0, connectivity), RINGS)
    no_ring = RINGS.copy()
    no_ring[1:6, 1:6] = 0
    assert np.array_equal(ccl_ref.clean(RINGS, 9, 0, connectivity), no_ring)
    assert np.array_equal(ccl_ref.clean(RINGS, 9, 25, connectivity), no_ring)
    assert np.array_equal(ccl_ref.clean(RINGS, 9, 26, connectivity), np.ones_like(RINGS))
    assert np.array_equal(ccl_ref.clean(RINGS, 25, 0, connectivity), np.zeros_like(RINGS))


def test_hole_touching_the_border_only_at_a_corner():
    m = A([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]])
    # foreground 8, background 4: (1, 1) is cut off from the corner pixel, a hole of its own, and fills
    filled = m.copy()
    filled[1, 1] = 1
    assert np.array_equal(ccl_ref.clean(m, 0, 5, 8), filled)
    assert ccl_ref.label(m, 8)[1, 1] == 5
    # foreground 4, background 8: the two zeros join across the corner and reach the border: nothing fills
    assert ccl_ref.label(m, 4)[1, 1] == 0
    assert np.array_equal(ccl_ref.clean(m, 0, 5, 4), m)


def test_speck_inside_a_pinhole_pins_the_order():
    m = np.ones((5, 5), np.int32)
    m[1:4, 1:4] = 0
    m[2, 2] = 1
    hole = np.ones((5, 5), np.int32)
    hole[1:4, 1:4] = 0
    # the speck goes first (1 < 2), which makes the hole 9 pixels: not < 9, it stays; filling first
    # (the ring of 8 zeros is < 9) would give all ones
    assert np.array_equal(ccl_ref.clean(m, 2, 9, 8), hole)
    assert np.array_equal(ccl_ref.clean(m, 2, 10, 8), np.ones_like(m))
    assert np.array_equal(ccl_ref.clean(m, 0, 9, 8), np.ones_like(m))
    assert np.array_equal(ccl_ref.clean(m, 0, 8, 8), m)
    assert np.array_equal(ccl_ref.clean(m, 0, 0, 8), m)


def test_multiclass_hole_takes_the_class_above_its_root():
    m = A([[2, 2, 3, 3, 3],
           [2, 2, 3, 0, 3],
           [2, 0, 0, 0, 3],
           [2, 2, 2, 3, 3]])
    root = ccl_ref.label(m, 8)
    assert root[2, 1] == 8  # the hole's root is (1, 3); above it lies class 3
    want = m.copy()
    want[m == 0] = 3
    assert np.array_equal(ccl_ref.clean(m, 0, 5, 8), want)
    assert np.array_equal(ccl_ref.clean(m, 0, 4, 8), m)


def test_batches_are_labelled_image_by_image():
    g = np.random.default_rng(5)
    maps = (g.random((3, 9, 11)) < 0.5).astype(np.int32)
    root = ccl_ref.label(maps, 8)
    for n in range(3):
        assert np.array_equal(root[n], ccl_ref.label(maps[n], 8))
    table = ccl_ref.components(maps, 8)
    assert table[:, 0].tolist() == sorted(table[:, 0].tolist())
    assert np.array_equal(table[table[:, 0] == 1][:, 1:], ccl_ref.components(maps[1], 8)[:, 1:])
    assert np.array_equal(ccl_ref.stats(root)[:, 2], ccl_ref.stats(root[2]))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("C,density", [(2, 0.41), (2, 0.59), (5, 0.5)])
def test_reference_matches_scipy_per_class(C, density, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(100 * C + connectivity)
    m = np.where(g.random((40, 53)) < density, g.integers(1, C, (40, 53)), 0).astype(np.int32)
    root = ccl_ref.label(m, connectivity)
    area = ccl_ref.stats(root)[0].reshape(-1)
    cross, full = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    for k in range(C):
        conn = connectivity if k else 12 - connectivity
        lab, n = ndimage.label(m == k, cross if conn == 4 else full)
        sel = m == k
        pairs = set(zip(lab[sel].tolist(), root[sel].tolist()))
        assert len(pairs) == n == len({r for _, r in pairs})  # the same partition
        sizes = np.bincount(lab[sel], minlength=n + 1)
        for l, r in pairs:
            assert area[r] == sizes[l]


# ---- 2. predict's flags --------------------------------------------------------------------------------
def test_check_clean_and_flags():
    import predict

    a = predict.parse_args([])
    assert (a.min_area, a.max_hole, a.connectivity, a.components) == (0, 0, 8, False)
    a = predict.parse_args(["--min-area", "30", "--max-hole", "12", "--connectivity", "4", "--components"])
    assert (a.min_area, a.max_hole, a.connectivity, a.components) == (30, 12, 4, True)
    with pytest.raises(SystemExit):
        predict.parse_args(["--connectivity", "6"])
    predict.check_clean(0, 0, 8)
    predict.check_clean(5, 7, 4)
    for bad in ((-1, 0, 8), (0, -3, 8), (0, 0, 6), (0, 0, 0)):
        with pytest.raises(ValueError):
            predict.check_clean(*bad)


# ---- 3. the C ABI's argument checks ----------------------------------------------------------------------
def _raw():
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    return lib.load()


# unetseg_ccl_label(cls, N, H, W, connectivity, root), the text the message must contain
BAD_LABEL = [
    ((None, 1, 4, 4, 8, PTR), "null"),
    ((PTR, 1, 4, 4, 8, None), "null"),
    ((PTR, 1, 4, 4, 3, PTR), "connectivity"),
    ((PTR, 1, 4, 4, 0, PTR), "connectivity"),
    ((PTR, 0, 4, 4, 8, PTR), "bad shape"),
    ((PTR, 1, -4, 4, 8, PTR), "bad shape"),
    ((PTR, 1, 4, 0, 8, PTR), "bad shape"),
    ((PTR, 1, 65536, 32768, 8, PTR), "2^31 - 1"),  # H * W = 2^31
    ((PTR, 1, 65536, 65536, 4, PTR), "2^31 - 1"),
    ((PTR, 2 ** 31 - 1, 46340, 46340, 8, PTR), "64-bit"),
]


@pytest.mark.parametrize("args,msg", BAD_LABEL)
def test_label_argument_errors_reported_without_device(args, msg):
    from unetseg_hip import lib

    raw = _raw()
    assert raw.unetseg_ccl_label(*args, None) != 0
    err = raw.unetseg_last_error().decode()
    assert "ccl_label" in err and msg in err, err
    with pytest.raises(RuntimeError, match=msg.replace("^", r"\^")):
        lib.lib.ccl_label(*args, None)


def test_stats_and_filter_argument_errors_reported_without_device():
    raw = _raw()

    def refused(rc, *texts):
        err = raw.unetseg_last_error().decode()
        assert rc != 0 and all(t in err for t in texts), err

    refused(raw.unetseg_ccl_stats(None, 1, 4, 4, PTR, None), "ccl_stats", "null")
    refused(raw.unetseg_ccl_stats(PTR, 1, 4, 4, None, None), "ccl_stats", "null")
    refused(raw.unetseg_ccl_stats(PTR, 1, 65536, 32768, PTR, None), "ccl_stats", "2^31 - 1")
    out = PTR + 64
    refused(raw.unetseg_ccl_filter(PTR, PTR, None, 1, 4, 4, 1, 5, out, None), "ccl_filter", "null")
    refused(raw.unetseg_ccl_filter(PTR, PTR, PTR, 1, 4, 4, 1, 5, PTR, None), "ccl_filter", "out must not be cls")
    refused(raw.unetseg_ccl_filter(PTR, PTR, PTR, 1, 4, 4, 3, 5, out, None), "ccl_filter", "step")
    refused(raw.unetseg_ccl_filter(PTR, PTR, PTR, 1, 4, 4, 2, -1, out, None), "ccl_filter", "threshold")
    refused(raw.unetseg_ccl_filter(PTR, PTR, PTR, 1, 0, 4, 2, 5, out, None), "ccl_filter", "bad shape")
    refused(raw.unetseg_ccl_tile(None, None), "ccl_tile", "null")


def test_tile_query_needs_no_device():
    from unetseg_hip import ccl

    _raw()
    tw, th = ccl.tile()
    assert tw >= 1 and th >= 1 and 2 * max(tw, th) + 1 <= 200  # the GPU tests' seam cases stay small


def test_clean_refuses_bad_thresholds_before_touching_the_map():
    from unetseg_hip import ccl

    for bad in ((-1, 0, 8), (0, -1, 8), (0, 0, 5)):
        with pytest.raises(ValueError):
            ccl.clean(None, *bad)
