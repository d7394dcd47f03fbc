"""GPU: tiled full-resolution inference (csrc/tiles.hip, predict.predict_labels_tiled).

The reference for the blend is written here in numpy float64 from the formulas of utils/tiling.py:
tile origins i * (t - o), the float32 window w(u) = min(1, (u + 1) / (o + 1), (t - u) / (o + 1)),
probability = sum_i w_i softmax(logits_i) / sum_i w_i over the covering tiles.

Bounds.  The fp32 path is one exp, sums of at most 21 terms and at most 4 weighted adds per value, so
its rounding is of order 1e-6; probabilities must sit within 1e-5 (absolute) of the float64
reference, a decade of margin, and lie in [0, 1].  Labels must equal the reference argmax wherever
the reference's top two probabilities differ by more than 1e-5; at most 0.1 % of the pixels may be
excluded that way, which is asserted on the reference alone first.  The gather is bit-exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
PROB_TOL = 1e-5
MARGIN = 1e-5
MAX_UNSURE = 1e-3


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- float64 / numpy references ---------------------------------------------------------------
def ref_gather(img, t, o, fill=128):
    """[n][3][t][t] float32, bit for bit what the kernel must write"""
    from utils import tiling

    H, W = img.shape[:2]
    nx, ny = tiling.grid(H, W, t, o)
    out = np.empty((nx * ny, 3, t, t), np.float32)
    for i in range(nx * ny):
        y0, x0 = tiling.tile_origin(i, H, W, t, o)
        tile = np.full((t, t, 3), fill, np.uint8)
        h, w = min(t, H - y0), min(t, W - x0)
        tile[:h, :w] = img[y0:y0 + h, x0:x0 + w]
        out[i] = np.transpose(tile.astype(np.float32) / np.float32(255), (2, 0, 1))
    return out


def ref_blend(logits, H, W, t, o):
    """float64 [C][H][W] blended probabilities of logits [n][C][t][t]"""
    from utils import tiling

    logits = np.asarray(logits, np.float64)
    nx, ny = tiling.grid(H, W, t, o)
    assert logits.shape[0] == nx * ny
    win = np.asarray(tiling.window(t, o), np.float64)
    num = np.zeros((logits.shape[1], H, W))
    den = np.zeros((H, W))
    for i in range(nx * ny):
        y0, x0 = tiling.tile_origin(i, H, W, t, o)
        h, w = min(t, H - y0), min(t, W - x0)
        e = np.exp(logits[i] - logits[i].max(0, keepdims=True))
        p = e / e.sum(0, keepdims=True)
        wt = np.outer(win[:h], win[:w])
        num[:, y0:y0 + h, x0:x0 + w] += wt * p[:, :h, :w]
        den[y0:y0 + h, x0:x0 + w] += wt
    assert (den > 0).all()
    return num / den


def check_against_reference(probs, labels, ref):
    """the bounds of the module docstring; prints each figure before it asserts"""
    srt = np.sort(ref, 0)
    sure = (srt[-1] - srt[-2]) > MARGIN
    unsure = 1.0 - sure.mean()
    print(f"unsure share {unsure:.2e} (cap {MAX_UNSURE:.0e})")
    assert unsure <= MAX_UNSURE  # the reference alone
    err = np.abs(probs.astype(np.float64) - ref).max()
    print(f"max |prob - ref| {err:.3e} (bound {PROB_TOL:.0e}); range [{probs.min():.3e}, {probs.max():.8f}]")
    assert err <= PROB_TOL
    assert probs.min() >= 0.0 and probs.max() <= 1.0
    want = ref.argmax(0)
    bad = int((labels[sure] != want[sure]).sum())
    print(f"label mismatches off the margin: {bad}")
    assert bad == 0


# ---- device helpers -----------------------------------------------------------------------------
def dev_gather(img_d, H, W, t, o, ranges, fill=128):
    from unetseg_hip.lib import lib

    n = sum(nt for _, nt in ranges)
    out = torch.full((n, 3, t, t), float("nan"), dtype=torch.float32, device=DEV)
    for t0, nt in ranges:
        lib.tile_gather(img_d.data_ptr(), H, W, t, o, t0, nt, fill, out[t0:].data_ptr(), _stream())
    return out


def dev_blend(lg_d, H, W, t, o, batch):
    """(acc, probs, labels) with the tiles accumulated in ranges of ``batch``"""
    from unetseg_hip.lib import lib
    from utils import tiling

    n, C = lg_d.shape[:2]
    acc = torch.zeros(C, H, W, dtype=torch.float32, device=DEV)
    for t0, nt in tiling.ranges(n, batch):
        lib.tile_accum(lg_d[t0:].data_ptr(), C, H, W, t, o, t0, nt, acc.data_ptr(), _stream())
    probs = torch.full((C, H, W), float("nan"), dtype=torch.float32, device=DEV)
    labels = torch.full((H, W), -1, dtype=torch.int32, device=DEV)
    lib.tile_finish(acc.data_ptr(), C, H, W, t, o, probs.data_ptr(), labels.data_ptr(), _stream())
    return acc, probs, labels


def n_tiles(H, W, t, o):
    from utils import tiling

    nx, ny = tiling.grid(H, W, t, o)
    return nx * ny


def random_logits(seed, n, C, t):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn(n, C, t, t, generator=g)


# ---- gather ---------------------------------------------------------------------------------------
# the last case has a tile that is no multiple of 4 (the one-value-per-lane kernel, not the float4 one)
@pytest.mark.parametrize("H,W,t,o", [(37, 53, 16, 4), (10, 9, 16, 4), (32, 48, 16, 0), (29, 41, 10, 3)])
def test_gather_bit_exact(H, W, t, o):
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img_d = torch.from_numpy(img).to(DEV)
    n = n_tiles(H, W, t, o)
    want = ref_gather(img, t, o)
    one = dev_gather(img_d, H, W, t, o, [(0, n)]).cpu().numpy()
    assert one.tobytes() == want.tobytes()
    # the fill region: everything outside the image is exactly 128 / 255
    if H % t or W % t or o:
        assert (want == np.float32(128) / np.float32(255)).any()
    if n > 1:
        two = dev_gather(img_d, H, W, t, o, [(0, 1), (1, n - 1)]).cpu().numpy()
        assert two.tobytes() == one.tobytes()
    other_fill = dev_gather(img_d, H, W, t, o, [(0, n)], fill=0).cpu().numpy()
    assert other_fill.tobytes() == ref_gather(img, t, o, fill=0).tobytes()


def test_gather_every_byte_value():
    """float(v) / 255.0f for all 256 byte values, against numpy's float32 division"""
    img = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) // 3
    img = img.astype(np.uint8)
    got = dev_gather(torch.from_numpy(img).to(DEV), 16, 16, 16, 0, [(0, 1)]).cpu().numpy()
    assert got.tobytes() == ref_gather(img, 16, 0).tobytes()
    assert len(np.unique(got)) == 256


# ---- blend ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 21])
@pytest.mark.parametrize("H,W,t,o", [(37, 53, 16, 4), (37, 53, 16, 8), (37, 53, 16, 0), (10, 9, 16, 4)])
def test_blend_matches_float64(C, H, W, t, o):
    n = n_tiles(H, W, t, o)
    lg = random_logits(100 * C + o + H, n, C, t)
    ref = ref_blend(lg.numpy(), H, W, t, o)
    _, probs, labels = dev_blend(lg.to(DEV), H, W, t, o, batch=n)
    check_against_reference(probs.cpu().numpy(), labels.cpu().numpy(), ref)


@pytest.mark.parametrize("C", [2, 32])
def test_blend_other_tile_and_class_count(C):
    """a tile that is no multiple of the wave or of 4, more columns than one 256-lane block, C at its cap"""
    H, W, t, o = 23, 300, 10, 5
    n = n_tiles(H, W, t, o)
    lg = random_logits(7 + C, n, C, t)
    ref = ref_blend(lg.numpy(), H, W, t, o)
    _, probs, labels = dev_blend(lg.to(DEV), H, W, t, o, batch=7)
    check_against_reference(probs.cpu().numpy(), labels.cpu().numpy(), ref)


def test_finish_without_probs():
    from unetseg_hip.lib import lib

    H, W, t, o, C = 37, 53, 16, 4, 5
    lg = random_logits(3, n_tiles(H, W, t, o), C, t).to(DEV)
    acc, _, labels = dev_blend(lg, H, W, t, o, batch=4)
    only = torch.full((H, W), -1, dtype=torch.int32, device=DEV)
    lib.tile_finish(acc.data_ptr(), C, H, W, t, o, None, only.data_ptr(), _stream())
    assert torch.equal(only, labels)


# ---- tie rule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 21])
def test_tie_goes_to_lowest_class(C):
    H, W, t, o = 37, 53, 16, 4
    n = n_tiles(H, W, t, o)
    flat = torch.full((n, C, t, t), 0.75, device=DEV)
    _, probs, labels = dev_blend(flat, H, W, t, o, batch=n)
    assert (labels == 0).all()
    assert np.abs(probs.cpu().numpy() - 1.0 / C).max() <= PROB_TOL


def test_unique_maximum_wins_everywhere():
    H, W, t, o, C = 37, 53, 16, 8, 21
    n = n_tiles(H, W, t, o)
    lg = torch.zeros(n, C, t, t, device=DEV)
    lg[:, 3] = 0.5
    _, _, labels = dev_blend(lg, H, W, t, o, batch=n)
    assert (labels == 3).all()  # the 37 x 53 grid with o = t / 2 has pixels in 4 tiles


# ---- split invariance -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,t,o", [(2, 16, 4), (21, 16, 8)])
def test_split_invariance(C, t, o):
    H, W = 37, 53
    n = n_tiles(H, W, t, o)
    lg = random_logits(11 + C, n, C, t).to(DEV)
    acc1, probs1, labels1 = dev_blend(lg, H, W, t, o, batch=n)
    for batch in (1, 3, 4):  # 4 does not divide a tile row: ranges that start and end mid-row
        acc, probs, labels = dev_blend(lg, H, W, t, o, batch=batch)
        assert torch.equal(acc.view(torch.int32), acc1.view(torch.int32)), batch
        assert torch.equal(probs.view(torch.int32), probs1.view(torch.int32)), batch
        assert torch.equal(labels, labels1), batch


# ---- offsets past 2^31 ------------------------------------------------------------------------------
def test_offsets_past_2_31():
    """the last tile of a 33000 x 33000 image: byte offsets into the image and element offsets into
    the second accumulator plane both exceed 2^31"""
    from unetseg_hip.lib import lib
    from utils import tiling

    H = W = 33000
    t, o, C = 64, 16, 2
    nx, ny = tiling.grid(H, W, t, o)
    last = nx * ny - 1
    y0, x0 = tiling.tile_origin(last, H, W, t, o)
    h, w = H - y0, W - x0
    assert (y0 * W + x0) * 3 > 2 ** 31 and H * W + y0 * W + x0 > 2 ** 31 and 0 < h < t and 0 < w < t
    g = torch.Generator().manual_seed(5)
    corner = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
    img = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    img[y0:, x0:] = corner.to(DEV)
    x = torch.full((1, 3, t, t), float("nan"), dtype=torch.float32, device=DEV)
    lib.tile_gather(img.data_ptr(), H, W, t, o, last, 1, 128, x.data_ptr(), _stream())
    want = np.full((t, t, 3), 128, np.uint8)
    want[:h, :w] = corner.numpy()
    want = np.transpose(want.astype(np.float32) / np.float32(255), (2, 0, 1))
    assert x[0].cpu().numpy().tobytes() == want.tobytes()
    del img
    lg = random_logits(9, 1, C, t)
    acc = torch.zeros(C, H, W, dtype=torch.float32, device=DEV)
    lib.tile_accum(lg.to(DEV).data_ptr(), C, H, W, t, o, last, 1, acc.data_ptr(), _stream())
    got = acc[:, y0:, x0:].cpu().numpy()
    win = np.asarray(tiling.window(t, o), np.float64)
    l64 = lg[0].numpy().astype(np.float64)
    p = np.exp(l64 - l64.max(0)) / np.exp(l64 - l64.max(0)).sum(0)
    ref = np.outer(win[:h], win[:w]) * p[:, :h, :w]
    assert np.abs(got - ref).max() <= PROB_TOL
    assert float(acc.sum()) == pytest.approx(float(got.astype(np.float64).sum()), rel=1e-4)  # nothing written elsewhere


# ---- predict_labels_tiled -------------------------------------------------------------------------
def _stub(x):
    return torch.stack([x[:, 0] - x[:, 1], x[:, 1] - x[:, 0]], 1)


@pytest.mark.parametrize("t,o", [(16, 4), (16, 8), (16, 0)])
def test_pointwise_stub_equals_whole_image_argmax(t, o):
    import predict

    H, W = 37, 53
    rng = np.random.default_rng(t + o)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[..., 1] = (img[..., 0].astype(np.int64) + rng.integers(1, 256, (H, W))) % 256  # r != g everywhere
    assert (img[..., 0] != img[..., 1]).all()
    want = (img[..., 1] > img[..., 0]).astype(np.int32)
    assert 0 < want.sum() < H * W
    got = {}
    for batch in (1, 8):
        got[batch] = predict.predict_labels_tiled(_stub, img, DEV, tile=t, overlap=o, tile_batch=batch)
        assert got[batch].dtype == np.int32 and got[batch].shape == (H, W)
        np.testing.assert_array_equal(got[batch], want)
    labels, probs = predict.predict_labels_tiled(_stub, img, DEV, tile=t, overlap=o, tile_batch=8, return_probs=True)
    np.testing.assert_array_equal(labels, want)
    assert probs.shape == (2, H, W) and probs.dtype == np.float32
    assert np.abs(probs.sum(0) - 1.0).max() <= 2 * PROB_TOL


def test_single_channel_model_refused():
    import predict

    img = np.zeros((20, 20, 3), np.uint8)
    with pytest.raises(ValueError, match="C=1"):
        predict.predict_labels_tiled(lambda x: x[:, :1], img, DEV, tile=16, overlap=4)
    with pytest.raises(ValueError):
        predict.predict_labels_tiled(_stub, img, DEV, tile=16, overlap=9)
    with pytest.raises(ValueError, match="RGB"):
        predict.predict_labels_tiled(_stub, img[..., 0], DEV, tile=16, overlap=4)


@pytest.fixture(scope="module")
def plain_model():
    from model.model_factory import build_model

    torch.manual_seed(1234)
    return build_model("unet_plain", num_classes=2).to(DEV).eval()


@pytest.mark.parametrize("bf16", [False, True])
def test_real_model_pipeline(plain_model, bf16):
    """predict_labels_tiled against the numpy blend of the logits the same model returns for the same
    gathered tiles (the pipeline is under test, not the model: with bf16 the logits are the model's own
    bf16-autocast logits)"""
    import predict
    from augment_data import make_image

    H, W, t, o = 96, 80, 64, 32
    image = make_image(np.random.default_rng(8), W, H)
    img = np.array(image, np.uint8)
    n = n_tiles(H, W, t, o)
    assert n == 4
    x = dev_gather(torch.from_numpy(img).to(DEV), H, W, t, o, [(0, n)])
    assert x.cpu().numpy().tobytes() == ref_gather(img, t, o).tobytes()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        lg = plain_model(x)
    assert tuple(lg.shape) == (n, 2, t, t)
    ref = ref_blend(lg.float().cpu().numpy(), H, W, t, o)
    labels, probs = predict.predict_labels_tiled(plain_model, image, DEV, tile=t, overlap=o, bf16=bf16,
                                                 return_probs=True)
    assert labels.shape == (H, W) and labels.dtype == np.int32
    check_against_reference(probs, labels, ref)
    np.testing.assert_array_equal(
        predict.predict_labels_tiled(plain_model, image, DEV, tile=t, overlap=o, bf16=bf16), labels)


# ---- command line ---------------------------------------------------------------------------------
def test_cli_flags_round_trip():
    import predict

    a = predict.parse_args([])
    assert (a.tile, a.overlap, a.tile_batch, a.bf16) == (0, 64, 8, False)
    a = predict.parse_args(["--tile", "64"])
    assert (a.tile, a.overlap, a.tile_batch, a.bf16) == (64, 64, 8, False)
    a = predict.parse_args(["--tile", "512", "--overlap", "32", "--tile-batch", "4", "--bf16"])
    assert (a.tile, a.overlap, a.tile_batch, a.bf16) == (512, 32, 4, True)


@pytest.mark.parametrize("argv,msg", [(["--tile", "48"], "multiple of 32"),
                                      (["--overlap", "40", "--tile", "64"], "overlap"),
                                      (["--tile", "64"], "overlap"),  # the default overlap of 64 exceeds 64 // 2
                                      (["--tile", "-32"], "multiple of 32"),
                                      (["--tile", "64", "--overlap", "16", "--tile-batch", "0"], "tile-batch")])
def test_cli_refuses_bad_tiling(tmp_path, argv, msg):
    import predict

    args = predict.parse_args(argv + ["--out-dir", str(tmp_path / "run"), "--weights", str(tmp_path / "none.pth")])
    with pytest.raises(ValueError, match=msg):
        predict.predict(args)
    assert not (tmp_path / "run").exists()  # refused before anything is created


def test_cli_tile_selects_the_path(tmp_path, monkeypatch):
    """--tile 0 takes the label map from predict_labels (the letterbox path), --tile T from
    predict_labels_tiled with the command line's options"""
    import predict
    from augment_data import make_image
    from PIL import Image

    path = tmp_path / "a.png"
    make_image(np.random.default_rng(0), 40, 30).save(path)
    calls = []

    def letterbox_path(model, image, device):
        calls.append(("letterbox",))
        return np.zeros((30, 40), np.int32)

    def tiled_path(model, image, device, **kw):
        calls.append(("tiled", kw))
        return np.ones((30, 40), np.int32)

    monkeypatch.setattr(predict, "predict_labels", letterbox_path)
    monkeypatch.setattr(predict, "predict_labels_tiled", tiled_path)
    out0 = tmp_path / "o0"
    out0.mkdir()
    saved = predict.detect_image(str(path), None, 2, str(out0), mix_type=False, device=DEV)
    assert calls == [("letterbox",)]
    assert np.asarray(Image.open(saved)).max() == 0  # class 0's palette colour everywhere
    saved = predict.detect_image(str(path), None, 2, str(out0), mix_type=False, device=DEV, tile=64, overlap=16,
                                 tile_batch=2, bf16=True)
    assert calls[1] == ("tiled", dict(tile=64, overlap=16, tile_batch=2, bf16=True))
    assert (np.asarray(Image.open(saved)) == np.array([128, 0, 0], np.uint8)).all()
    assert saved.endswith("a_mask.png")

    # predict() hands the command line's options through
    calls.clear()
    monkeypatch.setattr(predict, "load_model", lambda *a, **k: None)
    wpath = tmp_path / "w.pth"
    wpath.write_bytes(b"")
    base = ["--data_path", str(path), "--weights", str(wpath), "--num-classes", "1", "--out-dir", str(tmp_path / "run")]
    predict.predict(predict.parse_args(base + ["--tile", "0"]))
    predict.predict(predict.parse_args(base + ["--tile", "64", "--overlap", "32", "--tile-batch", "3"]))
    assert calls == [("letterbox",), ("tiled", dict(tile=64, overlap=32, tile_batch=3, bf16=False))]
