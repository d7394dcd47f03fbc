"""GPU: connected-component labelling, stats, component table and cleanup (csrc/ccl.hip,
unetseg_hip/ccl.py, the cleanup flags of predict.py) against tests/ccl_ref.py, bit for bit.

Every case compares the whole label map, the area plane everywhere and the box planes at the roots,
the component table, and a cleaned map: integers, so equality and no tolerance.

Sizes: 1 x 1, single rows and columns, 2 x 2, then 31 .. 65 and 129 around one and two 64-wide tiles,
two rectangles with both edges off the tile, and T - 1, T, T + 1, 2 T + 1 on each axis from
``ccl.tile()``, so that a change of the tile moves the cases with it.  Noise at the densities 0.41 and
0.59 sits at the 8- and 4-connected percolation thresholds, where components are large and tortuous;
the spiral filling a (2 T + 1)^2 square is the longest chain of joins that size can hold.
"""
import json
import os

import numpy as np
import pytest
import torch

import ccl_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
FIXED = [(1, 1), (1, 70), (70, 1), (2, 2), (31, 31), (33, 33), (63, 63), (64, 64), (65, 65), (129, 129), (37, 130),
         (130, 37)]
AROUND_TILE = ["T-1", "T", "T+1", "2T+1"]
DENSITIES = [0.30, 0.41, 0.50, 0.59, 0.70]


def _ccl():
    from unetseg_hip import ccl

    return ccl


def around(name, t):
    return {"T-1": t - 1, "T": t, "T+1": t + 1, "2T+1": 2 * t + 1}[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def check(cls, connectivity, min_area=3, max_hole=3):
    """label, stats, components and clean of one map (or batch) against the reference; returns the reference root"""
    ccl = _ccl()
    cls = np.ascontiguousarray(cls, np.int32)
    d = dev(cls)
    root = ccl.label(d, connectivity)
    want_root = ccl_ref.label(cls, connectivity)
    assert root.dtype == torch.int32 and root.shape == d.shape
    assert np.array_equal(root.cpu().numpy(), want_root)
    st = ccl.stats(root).cpu().numpy()
    want_st = ccl_ref.stats(want_root)
    at = ccl_ref.is_root(want_root)
    assert st.shape == want_st.shape == (4, *cls.shape)
    assert np.array_equal(st[0], want_st[0])  # the area everywhere: 0 away from the roots
    assert np.array_equal(st[:, at], want_st[:, at])
    table = ccl.components(d, connectivity)
    assert table.dtype == torch.int32 and table.is_cuda
    assert np.array_equal(table.cpu().numpy(), ccl_ref.components(cls, connectivity))
    got = ccl.clean(d, min_area, max_hole, connectivity)
    assert np.array_equal(got.cpu().numpy(), ccl_ref.clean(cls, min_area, max_hole, connectivity))
    assert np.array_equal(d.cpu().numpy(), cls)  # the input is left alone
    return want_root


def noise(seed, H, W, density, C):
    g = np.random.default_rng(seed)
    return np.where(g.random((H, W)) < density, g.integers(1, C, (H, W)), 0).astype(np.int32)


def run_noise(H, W, C, connectivity):
    for i, density in enumerate(DENSITIES):
        check(noise(1000 * H + 10 * W + i, H, W, density, C), connectivity)


# ---- 1. noise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("H,W", FIXED, ids=lambda v: str(v))
def test_noise_fixed_sizes(H, W, C, connectivity):
    run_noise(H, W, C, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("axis", ["rows", "columns"])
@pytest.mark.parametrize("name", AROUND_TILE)
def test_noise_around_the_tile(name, axis, C, connectivity):
    tw, th = _ccl().tile()
    if axis == "rows":
        run_noise(around(name, th), 70, C, connectivity)
    else:
        run_noise(70, around(name, tw), C, connectivity)


# ---- 2. shapes that stress the joins -------------------------------------------------------------------
def spiral(n):
    """a one-pixel-wide clockwise spiral of ones from the top-left corner inwards, one pixel between its arms"""
    a = np.zeros((n, n), np.int32)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1
    while True:
        moved = False
        while True:
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or a[ny, nx]:
                break
            ay, ax = ny + dy, nx + dx
            if 0 <= ay < n and 0 <= ax < n and a[ay, ax]:
                break
            y, x = ny, nx
            a[y, x] = 1
            moved = True
        if not moved:
            return a
        dy, dx = dx, -dy


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("complement", [False, True])
def test_spiral(complement, connectivity):
    tw, th = _ccl().tile()
    a = spiral(2 * max(tw, th) + 1)
    assert 0.45 < a.mean() < 0.55
    root = check(1 - a if complement else a, connectivity)
    assert len(np.unique(root)) == 2  # one arm of each class, however it is cut into tiles


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine_comb(connectivity):
    tw, th = _ccl().tile()
    H, W = 2 * th + 1, 2 * tw + 1
    a = np.zeros((H, W), np.int32)
    a[0::2] = 1
    a[1::4, W - 1] = 1
    a[3::4, 0] = 1
    root = check(a, connectivity)
    assert (root[a == 1] == 0).all()
    # the comb: the teeth hang on a spine in the last row, each gap a background component of its own
    b = np.zeros((H, W), np.int32)
    b[:, 0::2] = 1
    b[H - 1] = 1
    root = check(b, connectivity)
    assert (root[b == 1] == 0).all() and len(np.unique(root)) == 1 + W // 2


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("value", [0, 1])
def test_constant_maps(value, connectivity):
    tw, th = _ccl().tile()
    root = check(np.full((2 * th + 1, 2 * tw + 1), value, np.int32), connectivity)
    assert not root.any()


@pytest.mark.parametrize("anti", [False, True])
def test_two_pixels_meeting_across_a_tile_corner(anti):
    ccl = _ccl()
    tw, th = ccl.tile()
    a = np.zeros((2 * th, 2 * tw), np.int32)
    if anti:
        a[th - 1, tw], a[th, tw - 1] = 1, 1
    else:
        a[th - 1, tw - 1], a[th, tw] = 1, 1
    assert len(ccl.components(dev(a), 8)) == 1 and len(ccl.components(dev(a), 4)) == 2
    check(a, 8)
    check(a, 4)
    # the same for two background pixels in a foreground map, where the connectivities swap
    assert len(np.unique(check(1 - a, 4))) == 2 and len(np.unique(check(1 - a, 8))) == 3


@pytest.mark.parametrize("connectivity", [4, 8])
def test_u_whose_arms_meet_in_a_third_tile(connectivity):
    tw, th = _ccl().tile()
    a = np.zeros((2 * th, 2 * tw), np.int32)
    a[0:th + 6, 5] = 2
    a[3:th + 6, tw + 5] = 2
    a[th + 5, 5:tw + 6] = 2
    root = check(a, connectivity)
    assert (root[a == 2] == 5).all()  # the right arm's tile learns of the left arm's top through the seams only


def test_batch_against_single_images():
    ccl = _ccl()
    tw, th = ccl.tile()
    H, W = th + 7, 2 * tw + 3
    maps = np.stack([noise(1, H, W, 0.41, 5), noise(2, H, W, 0.59, 2), spiral(max(H, W))[:H, :W]])
    for connectivity in (4, 8):
        check(maps, connectivity)
        d = dev(maps)
        root = ccl.label(d, connectivity)
        st = ccl.stats(root)
        table = ccl.components(d, connectivity).cpu().numpy()
        for n in range(3):
            one = ccl.label(d[n], connectivity)
            assert torch.equal(root[n], one)
            assert torch.equal(st[0, n], ccl.stats(one)[0])
            single = ccl.components(d[n], connectivity).cpu().numpy()
            assert np.array_equal(table[table[:, 0] == n][:, 1:], single[:, 1:])


# ---- 3. clean ------------------------------------------------------------------------------------------
def dev_clean(a, *args):
    return _ccl().clean(dev(a), *args).cpu().numpy()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_clean_thresholds_pin_the_strict_less_than(connectivity):
    tw, th = _ccl().tile()
    a = np.zeros((th + 9, tw + 9), np.int32)
    a[2:4, 3:6] = 1                      # a block of 6 inside one tile
    a[th - 1:th + 1, tw - 2:tw + 1] = 3  # a block of 6 on the tile corner
    a[10, 20] = 2                        # a single pixel
    frame = np.ones_like(a)              # the same blocks as holes of a foreground map
    frame[a != 0] = 0
    for m in (a, frame):
        for min_area, max_hole in ((1, 1), (2, 2), (6, 6), (7, 7), (0, 7), (7, 0), (1, 2), (2, 1)):
            got = dev_clean(m, min_area, max_hole, connectivity)
            assert np.array_equal(got, ccl_ref.clean(m, min_area, max_hole, connectivity)), (min_area, max_hole)
    assert np.array_equal(dev_clean(a, 1, 0, connectivity), a)
    assert np.array_equal(dev_clean(a, 2, 0, connectivity), np.where(a == 2, 0, a))
    assert np.array_equal(dev_clean(a, 6, 0, connectivity), np.where(a == 2, 0, a))
    assert not dev_clean(a, 7, 0, connectivity).any()
    assert np.array_equal(dev_clean(frame, 0, 6, connectivity), np.where(a == 2, 1, frame))
    assert dev_clean(frame, 0, 7, connectivity).all()


def test_clean_leaves_a_hole_on_the_border():
    a = np.ones((70, 70), np.int32)
    a[0, 30] = 0         # on the top border
    a[20:23, 69] = 0     # on the right border
    a[69, 0] = 0         # the corner
    a[40:42, 0:2] = 0    # on the left border
    a[30, 30] = 0        # the one true hole
    want = a.copy()
    want[30, 30] = 1
    assert np.array_equal(ccl_ref.clean(a, 0, 50, 8), want)
    assert np.array_equal(dev_clean(a, 0, 50, 8), want)
    # a background pixel diagonal to a border hole joins it at connectivity 4 (background 8) only
    a[1, 31] = 0
    for connectivity, filled in ((8, 1), (4, 0)):
        got = dev_clean(a, 0, 50, connectivity)
        assert np.array_equal(got, ccl_ref.clean(a, 0, 50, connectivity))
        assert got[1, 31] == filled and got[0, 30] == 0


def test_clean_removes_the_speck_before_it_fills_the_pinhole():
    tw, th = _ccl().tile()
    a = np.ones((th + 5, tw + 5), np.int32)
    a[th - 2:th + 1, tw - 2:tw + 1] = 0  # a 3 x 3 pinhole across the tile corner
    a[th - 1, tw - 1] = 1                # with a speck at its centre
    hole = a.copy()
    hole[th - 1, tw - 1] = 0
    assert np.array_equal(dev_clean(a, 2, 9, 8), hole)  # the hole is 9 once the speck is gone: not < 9
    assert dev_clean(a, 2, 10, 8).all()
    assert dev_clean(a, 0, 9, 8).all()                  # unremoved, the speck leaves a ring of 8
    assert np.array_equal(dev_clean(a, 0, 8, 8), a)
    for args in ((2, 9, 8), (2, 10, 8), (0, 9, 8), (2, 9, 4), (0, 9, 4)):
        assert np.array_equal(dev_clean(a, *args), ccl_ref.clean(a, *args)), args


def test_clean_fills_a_multiclass_hole_with_the_class_above_its_root():
    a = np.full((70, 70), 2, np.int32)
    a[:, 35:] = 3
    a[:, 50:] = 4
    a[20, 40] = 0          # the root of the hole, under class 3
    a[21, 30:41] = 0       # the hole then runs left under class 2
    a[50:52, 48:52] = 0    # a hole astride 3 | 4 whose root lies under 3
    a[60, 60] = 7
    want = a.copy()
    want[20, 40] = 3
    want[21, 30:41] = 3
    want[50:52, 48:52] = 3
    assert np.array_equal(ccl_ref.clean(a, 0, 20, 8), want)
    assert np.array_equal(dev_clean(a, 0, 20, 8), want)
    want[60, 60] = 0  # the speck of class 7 becomes a hole of one, which takes class 4
    want[60, 60] = 4
    assert np.array_equal(dev_clean(a, 2, 20, 8), want)
    assert np.array_equal(ccl_ref.clean(a, 2, 20, 8), want)


def test_clean_with_both_thresholds_off_returns_the_input():
    d = dev(noise(9, 40, 50, 0.5, 3))
    keep = d.clone()
    for args in ((0, 0, 8), (0, 0, 4), (1, 1, 8)):
        assert torch.equal(_ccl().clean(d, *args), keep)
    assert torch.equal(d, keep)


def test_wrong_inputs_are_refused():
    ccl = _ccl()
    with pytest.raises(ValueError, match="int32"):
        ccl.label(torch.zeros(4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="GPU"):
        ccl.label(torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="connectivity"):
        ccl.label(torch.zeros(4, 4, dtype=torch.int32, device=DEV), 6)


# ---- 4. predict ----------------------------------------------------------------------------------------
def stub_model(C, tile, seed=3):
    """a callable returning the same fixed logits for every tile: blocky noise, so that the label map has
    components of many sizes"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(1, C, tile // 4, tile // 4, generator=g)
    fine = torch.randn(1, C, tile, tile, generator=g)
    fixed = (torch.nn.functional.interpolate(coarse, size=(tile, tile), mode="nearest") + 0.8 * fine).to(DEV)
    return lambda x: fixed.expand(x.shape[0], -1, -1, -1)


def test_tiled_prediction_cleans_on_the_device():
    import predict
    from augment_data import make_image

    image = make_image(np.random.default_rng(2), 150, 100)
    model = stub_model(3, 64)
    kw = dict(tile=64, overlap=16)
    plain = predict.predict_labels_tiled(model, image, DEV, **kw)
    assert plain.shape == (100, 150) and len(np.unique(plain)) == 3
    for min_area, max_hole, connectivity in ((6, 5, 8), (6, 0, 8), (0, 5, 4), (12, 12, 4)):
        got = predict.predict_labels_tiled(model, image, DEV, min_area=min_area, max_hole=max_hole,
                                           connectivity=connectivity, **kw)
        want = ccl_ref.clean(plain, min_area, max_hole, connectivity)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert (got != plain).any()
    got, table = predict.predict_labels_tiled(model, image, DEV, min_area=6, max_hole=5, components=True, **kw)
    assert np.array_equal(table, ccl_ref.components(ccl_ref.clean(plain, 6, 5, 8), 8))
    assert np.array_equal(predict.predict_labels_tiled(model, image, DEV, min_area=0, max_hole=0, **kw), plain)


def test_components_json_and_default_bytes(tmp_path):
    import predict
    from augment_data import make_image

    path = tmp_path / "a.png"
    image = make_image(np.random.default_rng(4), 130, 90)
    image.save(path)
    model = stub_model(3, 64, seed=8)
    kw = dict(mix_type=True, device=DEV, tile=64, overlap=16)
    folders = [tmp_path / n for n in ("plain", "explicit", "cleaned")]
    for f in folders:
        os.mkdir(f)
    plain = predict.detect_image(str(path), model, 3, str(folders[0]), **kw)
    explicit = predict.detect_image(str(path), model, 3, str(folders[1]), min_area=0, max_hole=0, connectivity=8,
                                    components=False, **kw)
    cleaned = predict.detect_image(str(path), model, 3, str(folders[2]), min_area=8, max_hole=6, connectivity=8,
                                   components=True, **kw)
    assert open(plain, "rb").read() == open(explicit, "rb").read()
    assert open(plain, "rb").read() != open(cleaned, "rb").read()
    assert os.listdir(folders[0]) == ["a_mask.png"] and sorted(os.listdir(folders[2])) == ["a_components.json",
                                                                                         "a_mask.png"]
    labels = predict.predict_labels_tiled(model, predict.cvtColor(image), DEV, tile=64, overlap=16)
    table = ccl_ref.components(ccl_ref.clean(labels, 8, 6, 8), 8)
    want = [{"class": int(r[1]), "area": int(r[2]), "bbox": [int(r[4]), int(r[3]), int(r[6]), int(r[5])]} for r in table]
    got = json.load(open(folders[2] / "a_components.json"))
    assert got == want and len(got) > 3 and min(c["area"] for c in got) >= 8


def test_predict_cli_with_cleanup(tmp_path):
    import predict
    from augment_data import make_image
    from model.model_factory import build_model

    torch.manual_seed(99)
    wpath = tmp_path / "w.pth"
    torch.save(build_model("unet_plain", num_classes=3).state_dict(), wpath)
    path = tmp_path / "a.png"
    make_image(np.random.default_rng(1), 96, 70).save(path)
    base = ["--data_path", str(path), "--weights", str(wpath), "--num-classes", "2", "--model", "unet_plain",
            "--out-dir", str(tmp_path / "run")]
    first = predict.predict(predict.parse_args(base))
    second = predict.predict(predict.parse_args(base + ["--min-area", "0", "--max-hole", "0", "--connectivity", "8"]))
    assert open(first[0], "rb").read() == open(second[0], "rb").read()
    assert not os.path.exists(first[0].replace("_mask.png", "_components.json"))
    for extra in (["--tile", "0"], ["--tile", "64", "--overlap", "16", "--tta", "hflip"]):
        saved = predict.predict(predict.parse_args(base + extra + ["--min-area", "9", "--max-hole", "9", "--connectivity",
                                                                   "4", "--components"]))
        rows = json.load(open(saved[0].replace("_mask.png", "_components.json")))
        assert all(set(r) == {"class", "area", "bbox"} and r["area"] >= 9 and r["class"] in (1, 2) for r in rows)
        assert all(0 <= r["bbox"][0] <= r["bbox"][2] < 96 and 0 <= r["bbox"][1] <= r["bbox"][3] < 70 for r in rows)
    with pytest.raises(ValueError, match="min-area"):
        predict.predict(predict.parse_args(base + ["--min-area", "-2"]))
