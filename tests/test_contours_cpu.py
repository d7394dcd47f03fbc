"""CPU: the contour contract on its sequential reference (tests/contours_ref.py), the host half of
unetseg_hip/contours.py (polygons, simplify, labelme), predict.py's polygon flags and the argument checks of the
new C-ABI entry points through the built library (no launch).

The reference self-checks are what make it a yardstick for tests/test_gpu_contours.py: painting the labelme
document of a map at epsilon 0 gives the map back; the signed areas of a component's loops sum to its pixel count;
there is one outer loop per component; a binary map has one hole per enclosed background component.
"""
import ctypes
import os

import numpy as np
import pytest

import ccl_ref
import contours_ref as ref


def _c():
    from unetseg_hip import contours

    return contours


def _maps(H, W):
    return ref.size_cases(H, W) + [np.ones((H, W), np.int32), np.zeros((H, W), np.int32), ref.checkerboard(H, W)]


def _roundtrip(m, conn, loops, vertices):
    c = _c()
    H, W = m.shape
    doc = c.labelme(c.polygons(loops, vertices), H, W, "a.png", epsilon=0)
    assert doc["imageHeight"] == H and doc["imageWidth"] == W and doc["imageData"] is None
    assert np.array_equal(ref.rasterise(ref.labelme_shapes(doc), H, W), m)


@pytest.mark.parametrize("H,W", ref.CPU_SIZES)
@pytest.mark.parametrize("conn", [4, 8])
def test_reference_invariants(H, W, conn):
    for m in _maps(H, W):
        loops, vertices = ref.trace(m, conn)
        assert loops.dtype == np.int32 and vertices.dtype == np.int32
        _roundtrip(m, conn, loops, vertices)
        comps = ccl_ref.components(m, conn)
        outer = loops[loops[:, 3] == 0]
        assert len(outer) == len(comps)  # one outer loop per component, in the same order
        root = ccl_ref.label(m, conn)
        st = ccl_ref.stats(root).reshape(4, -1)
        assert np.array_equal(outer[:, 1], comps[:, 1])
        for r in outer[:, 2]:
            mine = loops[loops[:, 2] == r]
            assert mine[:, 6].sum() == st[0, r]  # signed areas sum to the pixel count
            assert mine[0, 3] == 0 and (mine[1:, 3] == 1).all() and (mine[1:, 6] < 0).all() and mine[0, 6] > 0
        assert loops[:, 5].sum() == len(vertices)
        assert np.array_equal(loops[:, 4], np.cumsum(loops[:, 5]) - loops[:, 5])
        assert (loops[:, 7] >= 4).all() and (loops[:, 5] >= 4).all() and (loops[:, 5] % 2 == 0).all()
        if m.max() <= 1:  # binary: holes are the enclosed background components of the dual connectivity
            enclosed = 0
            for r in np.flatnonzero(ccl_ref.is_root(root).reshape(-1)):
                y, x = divmod(int(r), W)
                if m[y, x] == 0 and y > 0 and st[1, r] < H - 1 and st[2, r] > 0 and st[3, r] < W - 1:
                    enclosed += 1
            assert (loops[:, 3] == 1).sum() == enclosed


def linked_rings():
    """two rings of classes 1 and 2 that cross at two saddles: part of each lies inside the other's hole, so no
    order of whole-loop shapes repaints the map"""
    m = np.zeros((12, 12), np.int32)
    m[1, 1:8] = m[1:4, 7] = m[4:8, 8] = m[7, 4:9] = m[6, 1:4] = m[1:7, 1] = 1
    m[4, 4:8] = m[3, 8:11] = m[3:11, 10] = m[10, 3:11] = m[7:11, 3] = m[4:7, 4] = 2
    assert m[3:5, 7:9].tolist() == [[1, 2], [2, 1]] and m[6:8, 3:5].tolist() == [[1, 2], [2, 1]]
    return m


def test_crossing_classes_are_repainted():
    c = _c()
    m = linked_rings()
    loops, vertices = ref.trace(m, 8)
    polys = c.polygons(loops, vertices)
    assert c._crossed(polys)  # some component reaches into a later one's hole
    _roundtrip(m, 8, loops, vertices)
    plain = sum(1 + len(p["holes"]) for p in polys)
    doc = c.labelme(polys, *m.shape, "a.png", epsilon=0)
    extra = doc["shapes"][plain:]
    assert len(extra) == len(c._crossed(polys)) and all(s["label"] != "_background_" for s in extra)
    assert [s["group_id"] for s in extra] == c._crossed(polys)
    # each extra shape covers its component's pixels and nothing else
    root = ccl_ref.label(m, 8)
    for s in extra:
        alone = ref.rasterise([(1, s["points"])], *m.shape)
        assert np.array_equal(alone == 1, root == polys[s["group_id"]]["root"])
    # without a crossing the layout is the plain one: one shape per loop
    for conn, mm in ((4, m), (8, (m == 1).astype(np.int32)), (4, ref.noise(33, 33, 0.59, 5, seed=2))):
        pl = c.polygons(*ref.trace(mm, conn))
        assert c._crossed(pl) == []
        assert len(c.labelme(pl, *mm.shape, "a.png", epsilon=0)["shapes"]) == sum(1 + len(p["holes"]) for p in pl)
    # a keyhole path alone: a ring with its hole
    ring = np.ones((3, 3), np.int32)
    ring[1, 1] = 0
    pr = c.polygons(*ref.trace(ring, 8))[0]
    assert np.array_equal(ref.rasterise([(1, c._keyhole(pr["outer"], pr["holes"]))], 3, 3), ring)


def test_saddle_tables():
    m = np.array([[1, 0], [0, 1]], np.int32)
    loops, vertices = ref.trace(m, 8)
    assert loops.tolist() == [[0, 1, 0, 0, 0, 8, 2, 8]]
    assert vertices.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    loops, vertices = ref.trace(m, 4)
    assert loops.tolist() == [[0, 1, 0, 0, 0, 4, 1, 4], [0, 1, 3, 0, 4, 4, 1, 4]]
    assert vertices.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1], [1, 1], [2, 1], [2, 2], [1, 2]]


def test_ring_and_batch_tables():
    ring = np.ones((3, 3), np.int32)
    ring[1, 1] = 0
    loops, vertices = ref.trace(ring, 8)
    # the hole's leader is the bottom side of (0, 1): crack id 6; it runs anticlockwise
    assert loops.tolist() == [[0, 1, 0, 0, 0, 4, 9, 12], [0, 1, 0, 1, 4, 4, -1, 4]]
    assert vertices.tolist() == [[0, 0], [3, 0], [3, 3], [0, 3], [2, 1], [1, 1], [1, 2], [2, 2]]
    batch = np.stack([ring, np.zeros((3, 3), np.int32), 2 * ring])
    loops, vertices = ref.trace(batch, 4)
    assert loops[:, 0].tolist() == [0, 0, 2, 2] and loops[:, 1].tolist() == [1, 1, 2, 2]
    assert loops[:, 4].tolist() == [0, 4, 8, 12] and len(vertices) == 16
    polys = _c().polygons(loops, vertices)
    assert [(p["image"], p["class"], p["area"], p["perimeter"], len(p["holes"])) for p in polys] == \
        [(0, 1, 8, 16, 1), (2, 2, 8, 16, 1)]


def test_special_maps_roundtrip():
    for m in (ref.spiral(21), ref.rings(), ref.comb()):
        for conn in (4, 8):
            loops, vertices = ref.trace(m, conn)
            _roundtrip(m, conn, loops, vertices)
    sp = ref.spiral(21)
    assert len(ref.trace(sp, 4)[0]) == 1 and sp.sum() > 21 * 21 // 3  # one long loop
    assert (ref.trace(ref.rings(), 8)[0][:, 3] == 1).sum() == 4  # every ring has its hole


def test_labelme_document():
    c = _c()
    m = ref.rings()
    polys = c.polygons(*ref.trace(m, 8))
    doc = c.labelme(polys, 29, 29, "x.png", class_names=["bg", "thread", "fill", "dot"], epsilon=0)
    assert set(doc) == {"version", "flags", "shapes", "imagePath", "imageData", "imageHeight", "imageWidth"}
    labels = [s["label"] for s in doc["shapes"]]
    assert labels == ["thread", "_background_", "fill", "_background_", "thread", "_background_", "dot",
                      "_background_", "thread"]
    assert [s["group_id"] for s in doc["shapes"]] == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert all(s["shape_type"] == "polygon" and len(s["points"]) >= 3 for s in doc["shapes"])
    assert np.array_equal(ref.rasterise(ref.labelme_shapes(doc, ["bg", "thread", "fill", "dot"]), 29, 29), m)
    with pytest.raises(ValueError):
        c.labelme(polys, 29, 29, "x.png", class_names=["bg", "thread"])
    with pytest.raises(ValueError):
        c.labelme(polys, 29, 29, "x.png", epsilon=-1)


# ---- simplify ----------------------------------------------------------------------------------------------------
def _dist_to_polyline(p, ring):
    best = np.inf
    for a, b in zip(ring, np.roll(ring, -1, 0)):
        ab = b - a
        den = ab @ ab
        t = np.clip((p - a) @ ab / den, 0, 1) if den > 0 else 0.0
        best = min(best, np.hypot(*(p - (a + t * ab))))
    return best


def test_simplify():
    c = _c()
    loops, vertices = ref.trace(ref.noise(37, 130, 0.59, 2, seed=4), 4)
    big = loops[np.argsort(-loops[:, 5])[:6]]
    for _, _, _, _, first, count, _, _ in big.tolist():
        pts = vertices[first:first + count]
        assert c.simplify(pts, 0) is pts and c.simplify(pts, -1.0) is pts
        assert c.simplify(pts.tolist(), 0) == pts.tolist()
        prev = count
        for eps in (0.5, 1.0, 2.5, 1000.0):
            kept = c.simplify(pts, eps)
            assert 3 <= len(kept) <= prev and kept.dtype == pts.dtype
            prev = len(kept)
            assert (kept[0] == pts[0]).all()
            # a subsequence of the input, and every dropped vertex lies within eps of the kept loop
            it = iter(pts.tolist())
            assert all(any(k == q for q in it) for k in kept.tolist())
            ring = kept.astype(np.float64)
            for p in pts.astype(np.float64):
                assert _dist_to_polyline(p, ring) <= eps + 1e-9
    sq = [[0, 0], [4, 0], [4, 4], [0, 4]]
    assert len(c.simplify(sq, 100.0)) == 3  # never below a triangle
    assert c.simplify(sq, 1.0) == sq
    assert c.simplify([[0, 0], [2, 0], [4, 0], [4, 4], [0, 4]], 0.5) == sq


# ---- predict's flags ---------------------------------------------------------------------------------------------
def test_predict_flags():
    import predict

    a = predict.parse_args([])
    assert a.polygons is False and a.polygon_epsilon == 1.0 and a.class_names is None
    a = predict.parse_args(["--polygons", "--polygon-epsilon", "0", "--class-names", "bg, thread,fill"])
    assert a.polygons is True and a.polygon_epsilon == 0.0
    assert predict.parse_class_names(a.class_names) == ["bg", "thread", "fill"]
    assert predict.parse_class_names(None) is None
    predict.check_polygons(0.0, None, 3)
    predict.check_polygons(2.5, ["bg", "a", "b"], 3)
    with pytest.raises(ValueError):
        predict.check_polygons(-0.5, None, 3)
    with pytest.raises(ValueError):
        predict.check_polygons(1.0, ["bg", "a", "b", "c"], 3)
    polys = _c().polygons(*ref.trace(ref.rings(), 8))
    table = ccl_ref.components(ref.rings(), 8)
    rows = predict.components_json(table, polys)
    assert [r["perimeter"] for r in rows] == [p["perimeter"] for p in polys]
    assert [r["area"] for r in rows] == [p["area"] for p in polys]
    assert "perimeter" not in predict.components_json(table)[0]
    doc = predict.polygons_json(polys, 29, 29, "a.jpg", ["bg", "thread"], 0.0)
    assert [s["label"] for s in doc["shapes"]][:3] == ["thread", "_background_", "class_2"]


# ---- the C ABI's argument checks -----------------------------------------------------------------------------------
def _raw():
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    return lib.load()


def test_cabi_refuses_bad_arguments():
    raw = _raw()
    ptr = 4096  # never dereferenced: every call below is refused before a launch
    M = 1000
    size = raw.unetseg_contours_workspace(M)
    assert size > 0 and raw.unetseg_contours_workspace(0) == 0 and raw.unetseg_contours_workspace(2**31) == 0
    assert raw.unetseg_contours_workspace(2 * M) > size
    at = (ctypes.c_int64 * 8)()
    assert raw.unetseg_contours_layout(M, ctypes.addressof(at)) == 0
    assert list(at) == sorted(at) and at[7] < size
    assert raw.unetseg_contours_layout(M, None) != 0 and raw.unetseg_contours_layout(0, ctypes.addressof(at)) != 0
    assert raw.unetseg_contours_tile(None, None) != 0

    def refused(rc, word):
        assert rc == 1 and word in raw.unetseg_last_error(), raw.unetseg_last_error()

    refused(raw.unetseg_contours_mask(None, 1, 8, 8, ptr, ptr, None), b"null")
    refused(raw.unetseg_contours_mask(ptr, 1, 8, 8, None, ptr, None), b"null")
    refused(raw.unetseg_contours_mask(ptr, -1, 8, 8, ptr, ptr, None), b"bad shape")
    refused(raw.unetseg_contours_mask(ptr, 1, 32768, 32768, ptr, ptr, None), b"2^29")
    refused(raw.unetseg_contours_mask(ptr, 1, 1, 2**29 + 1, ptr, ptr, None), b"2^29")
    link = lambda *a: raw.unetseg_contours_link(*a)  # noqa: E731
    refused(link(ptr, ptr, None, 1, 64, 64, 8, M, ptr, ptr, size, None), b"null")
    refused(link(ptr, ptr, ptr, 1, 64, 64, 3, M, ptr, ptr, size, None), b"connectivity 3")
    refused(link(ptr, ptr, ptr, 1, 32768, 32768, 8, M, ptr, ptr, size, None), b"2^29")
    refused(link(ptr, ptr, ptr, 1, 64, 64, 8, M, ptr, ptr, size - 1, None), b"too small")
    refused(link(ptr, ptr, ptr, 1, 64, 64, 8, M, ptr, None, size, None), b"null workspace")
    refused(link(ptr, ptr, ptr, 1, 64, 64, 8, M, ptr, ptr + 4, size, None), b"aligned")
    refused(link(ptr, ptr, ptr, 1, 64, 64, 8, 0, ptr, ptr, size, None), b"cracks")
    refused(link(ptr, ptr, ptr, 1, 4, 4, 8, M, ptr, ptr, size, None), b"4 sides")
    refused(raw.unetseg_contours_rank(1, 64, 64, M, ptr, size - 1, None), b"too small")
    refused(raw.unetseg_contours_rank(1, 32768, 32768, M, ptr, size, None), b"2^29")
    refused(raw.unetseg_contours_rank(1, 64, 64, 2**31, ptr, size, None), b"cracks")
    emit = lambda *a: raw.unetseg_contours_emit(*a)  # noqa: E731
    refused(emit(None, ptr, 1, 64, 64, M, ptr, ptr, 3, ptr, ptr, 12, ptr, size, None), b"null")
    refused(emit(ptr, ptr, 1, 64, 64, M, None, ptr, 3, ptr, ptr, 12, ptr, size, None), b"null")
    refused(emit(ptr, ptr, 1, 64, 64, M, ptr, ptr, -1, ptr, ptr, 12, ptr, size, None), b"negative")
    refused(emit(ptr, ptr, 1, 64, 64, M, ptr, ptr, 3, ptr, ptr, 12, ptr, size - 1, None), b"too small")
    # an empty batch is no error and launches nothing
    assert raw.unetseg_contours_mask(ptr, 0, 8, 8, ptr, ptr, None) == 0
    assert raw.unetseg_contours_rank(0, 8, 8, M, None, 0, None) == 0
