"""GPU: ``contours.trace`` (csrc/contours.hip, unetseg_hip/contours.py) against tests/contours_ref.py, bit for bit.

Everything is integer, so every comparison is equality: the ``loops`` table, the ``vertices`` array and their
dtypes.  The input must stay what it was and two runs must give the same bytes.  Sizes come from ``ccl.tile()`` and
``contours.tile()`` so that a change of either tile moves the cases with it.
"""
import numpy as np
import pytest
import torch

import contours_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _c():
    from unetseg_hip import contours

    return contours


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def check(m, conns=(4, 8)):
    """trace of one map or batch against the reference, under each connectivity; returns the last device result"""
    c = _c()
    for conn in conns:
        want_l, want_v = ref.trace(m, conn)
        d = dev(m)
        loops, vertices = c.trace(d, conn)
        assert loops.dtype == torch.int32 and vertices.dtype == torch.int32
        assert loops.device.type == "cuda" and vertices.device.type == "cuda"
        assert tuple(loops.shape) == want_l.shape and tuple(vertices.shape) == want_v.shape
        assert np.array_equal(loops.cpu().numpy(), want_l)
        assert np.array_equal(vertices.cpu().numpy(), want_v)
        again = c.trace(d, conn)
        assert torch.equal(again[0], loops) and torch.equal(again[1], vertices)
        assert np.array_equal(d.cpu().numpy(), m)
    return loops, vertices


def test_tile_query():
    tw, th = _c().tile()
    assert tw == 64 and th > 0


@pytest.mark.parametrize("H,W", ref.CPU_SIZES + ref.GPU_SIZES)
def test_sizes(H, W):
    for m in ref.size_cases(H, W):
        check(m)


@pytest.mark.parametrize("which,axis", [("ccl", "H"), ("ccl", "W"), ("contours", "H"), ("contours", "W")])
def test_sizes_around_the_tiles(which, axis):
    from unetseg_hip import ccl

    tw, th = ccl.tile() if which == "ccl" else _c().tile()
    for H, W in ref.tile_sizes(th if axis == "H" else tw, axis):
        check(ref.noise(H, W, 0.59, 2, seed=1), (4,))
        check(ref.noise(H, W, 0.41, 5, seed=2), (8,))


@pytest.mark.parametrize("H,W", [(1, 1), (33, 33), (65, 130)])
def test_full_empty_checkerboard(H, W):
    loops, vertices = check(np.ones((H, W), np.int32))
    assert loops.tolist() == [[0, 1, 0, 0, 0, 4, H * W, 2 * (H + W)]]
    assert vertices.tolist() == [[0, 0], [W, 0], [W, H], [0, H]]
    loops, vertices = check(np.zeros((H, W), np.int32))
    assert tuple(loops.shape) == (0, 8) and tuple(vertices.shape) == (0, 2)
    cb = ref.checkerboard(H, W)
    loops, _ = check(cb, (4,))
    assert len(loops) == cb.sum() and (loops[:, 5] == 4).all()  # every pixel is its own loop
    loops, _ = check(cb, (8,))
    assert (loops[:, 3] == 0).sum() == 1  # one component, every enclosed background pixel a hole


def test_spiral_longest_loop():
    from unetseg_hip import ccl

    T = max(ccl.tile() + _c().tile())
    m = ref.spiral(2 * T + 1)
    loops, _ = check(m, (4,))
    assert len(loops) == 1 and loops[0, 7].item() == 2 * int(m.sum()) + 2
    check(m, (8,))


def test_rings_comb_and_saddle():
    loops, _ = check(ref.rings())
    assert (loops[:, 3] == 1).sum().item() == 4
    check(ref.comb())
    check(ref.comb(67, 131))
    m = np.array([[1, 0], [0, 1]], np.int32)
    loops, vertices = check(m, (8,))
    assert loops.tolist() == [[0, 1, 0, 0, 0, 8, 2, 8]]
    assert vertices.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    loops, vertices = check(m, (4,))
    assert loops.tolist() == [[0, 1, 0, 0, 0, 4, 1, 4], [0, 1, 3, 0, 4, 4, 1, 4]]


def test_batch_with_an_empty_image():
    H, W = 70, 67
    batch = np.stack([ref.noise(H, W, 0.59, 3, seed=7), np.zeros((H, W), np.int32), ref.noise(H, W, 0.41, 2, seed=8)])
    loops, _ = check(batch)
    assert set(loops[:, 0].tolist()) == {0, 2}
    c = _c()
    empty = c.trace(torch.zeros(0, 8, 8, dtype=torch.int32, device=DEV))
    assert tuple(empty[0].shape) == (0, 8) and tuple(empty[1].shape) == (0, 2)
    with pytest.raises(ValueError):
        c.trace(dev(batch), 6)
    with pytest.raises(ValueError):
        c.trace(dev(batch).long())


@pytest.mark.parametrize("conn", [4, 8])
def test_labelme_from_the_device_result_repaints_the_map(conn):
    c = _c()
    for m in (ref.noise(37, 130, 0.59, 2, seed=3), ref.noise(65, 65, 0.50, 2, seed=5), ref.rings()):
        H, W = m.shape
        doc = c.labelme(c.polygons(*c.trace(dev(m), conn)), H, W, "a.png", epsilon=0)
        assert np.array_equal(ref.rasterise(ref.labelme_shapes(doc), H, W), m)


def test_predict_tiled_polygons_end_to_end():
    """predict_labels_tiled with a stub model and polygons=True: the JSON's shapes repaint the returned label map"""
    import predict
    from augment_data import make_image

    def model(x):  # three classes from the colour channels: any callable is accepted
        return torch.stack([x[:, 0] * 4, x[:, 1] * 4 + 0.3, x[:, 2] * 4 + 0.1], 1)

    image = make_image(np.random.default_rng(11), 96, 96)
    labels, table, polys = predict.predict_labels_tiled(model, image, DEV, tile=64, overlap=16, min_area=4,
                                                        connectivity=4, components=True, polygons=True)
    assert labels.shape == (96, 96) and len(polys) == len(table) > 0
    doc = predict.polygons_json(polys, 96, 96, "a.png", None, 0.0)
    assert np.array_equal(ref.rasterise(ref.labelme_shapes(doc), 96, 96), labels)
    rows = predict.components_json(table, polys)
    assert all(r["perimeter"] >= 4 and r["area"] == p["area"] for r, p in zip(rows, polys))
    plain = predict.predict_labels_tiled(model, image, DEV, tile=64, overlap=16, min_area=4, connectivity=4)
    assert np.array_equal(plain, labels)
