"""GPU: hard skeleton (thinning), the clDice counts and their way into the evaluate loops and predict.py
(csrc/skeleton.hip, unetseg_hip/skeleton.py) against tests/skeleton_ref.py, bit for bit.

Everything is integer, so every comparison is equality.  Sizes come from ``skeleton.tile()`` so that a change
of the tile or of the passes per launch moves the cases with it: single pixels, rows and columns, maps one
pixel off the tile on either axis (structures straddle the seams, widths that are and are not a multiple of
four take the word and the byte copy path), maps that need many launches, a batch whose images stop at
different launches, several classes, and every ``max_passes`` around the passes per launch.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import skeleton_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _s():
    from unetseg_hip import skeleton

    return skeleton


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def check(cls, max_passes=None):
    """thin of one map or batch against the reference, the flags included; returns the reference skeleton"""
    s = _s()
    cls = np.ascontiguousarray(cls, np.int32)
    want, want_unc = ref.thin(cls, max_passes)
    got, unc = s.thin(dev(cls), max_passes, return_unconverged=True)
    assert got.dtype == torch.int32 and got.shape == cls.shape
    assert unc.dtype == torch.int32 and unc.shape == (1 if cls.ndim == 2 else cls.shape[0],)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(unc.cpu(), torch.from_numpy(want_unc))
    assert torch.equal(s.thin(dev(cls), max_passes), got)
    return want


def mixed(H, W, seed, classes=1):
    """blobs, bars and noise in one map, so that thick and thin structures cross every seam"""
    rng = np.random.default_rng(seed)
    a = ref.random_map(1, H, W, rng, classes)
    lines = ref.thin_lines(H, W) if min(H, W) >= 8 else np.zeros((H, W), np.int32)
    a = np.where(lines != 0, lines if classes == 1 else (lines * (1 + (np.arange(W)[None, :] * classes // W))), a)
    speck = rng.random((H, W)) < 0.03
    return np.where(speck, 1, a).astype(np.int32)


def test_tile_query():
    tw, th, k = _s().tile()
    assert tw > 0 and th > 0 and k > 0


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (2, 2)])
def test_tiny_maps(H, W):
    check(np.ones((H, W), np.int32))
    check(np.zeros((H, W), np.int32))


@pytest.mark.parametrize("case", ["th-1 x tw+1", "th+3 x 2tw+1", "2th+1 x tw-1"])
def test_structures_across_the_seams(case):
    tw, th, _ = _s().tile()
    H, W = {"th-1 x tw+1": (th - 1, tw + 1), "th+3 x 2tw+1": (th + 3, 2 * tw + 1), "2th+1 x tw-1": (2 * th + 1, tw - 1)}[case]
    want = check(mixed(H, W, H * 7 + W))
    assert (want != 0).any()
    check(np.ones((H, W), np.int32))


def test_word_path_across_the_seams():
    """widths that are a multiple of four are staged and written as 32-bit words"""
    tw, th, _ = _s().tile()
    check(mixed(th + 5, 2 * tw + 4, 11))
    check(mixed(2 * th, tw, 12))
    check(mixed(9, 8, 13))


def test_many_launches_full_map_and_disc():
    _, _, k = _s().tile()
    full = np.ones((70, 45), np.int32)
    assert ref.thin_image(full)[1] > 3 * k  # the case spans several launches
    check(full)
    disc = ref.disc(64, 30)
    assert ref.thin_image(disc)[1] > 3 * k
    check(disc)


def test_batch_whose_images_stop_at_different_launches():
    H, W = 70, 45
    batch = np.stack([np.zeros((H, W), np.int32), np.ones((H, W), np.int32), ref.thin_lines(H, W)])
    passes = [ref.thin_image(m)[1] for m in batch]
    assert passes[0] == 1 and passes[2] < passes[1]
    want = check(batch)
    for n in range(3):  # and an image does not see its neighbours in the batch
        assert np.array_equal(check(batch[n]), want[n])


def test_three_classes():
    tw, th, _ = _s().tile()
    a = mixed(th + 9, tw + 14, 5, classes=3)
    assert set(np.unique(a)) == {0, 1, 2, 3}
    want = check(a)
    for c in (1, 2, 3):  # each class as if it were alone
        assert np.array_equal(want == c, ref.thin_image((a == c).astype(np.int32))[0] == 1)
    # values outside 1 .. 255 are background; 255 is a class
    odd = a.copy()
    odd[a == 1], odd[a == 2] = 255, 256
    odd[0, 0] = -7
    got = check(odd)
    assert not (got == 256).any() and (got == 255).any() and got[0, 0] == 0


def test_max_passes_around_the_passes_per_launch():
    _, _, k = _s().tile()
    full = np.ones((70, 45), np.int32)
    for p in sorted({0, 1, k - 1, k, k + 1, 2 * k, 2 * k + 1}):
        check(full, p)
        want, unc = ref.thin(full, p)
        assert unc[0] == (1 if p > 0 else 0)  # the full map is far from done at any of these
    assert np.array_equal(ref.thin(full, 0)[0], full)
    # the cap that cuts off only the empty pass, and the one that lets it run
    need = ref.thin_image(full)[1]
    check(full, need - 1)
    check(full, need)
    assert ref.thin(full, need - 1)[1][0] == 1 and ref.thin(full, need)[1][0] == 0


def test_non_contiguous_and_2d_input():
    s = _s()
    a = mixed(40, 90, 21)
    wide = dev(np.concatenate([a, a[:, ::-1]], 1))
    view = wide[:, :90]
    assert not view.is_contiguous()
    got = s.thin(view)
    assert got.shape == (40, 90) and torch.equal(got.cpu(), torch.from_numpy(ref.thin(a)[0]))
    stack = dev(np.stack([a, a[::-1], np.zeros_like(a)]))
    assert torch.equal(s.thin(stack[::2]).cpu(), torch.from_numpy(ref.thin(np.stack([a, np.zeros_like(a)]))[0]))


def test_refusals():
    s = _s()
    good = dev(np.ones((4, 4), np.int32))
    with pytest.raises(ValueError):
        s.thin(good.long())
    with pytest.raises(ValueError):
        s.thin(good.cpu())
    with pytest.raises(ValueError):
        s.thin(good.view(1, 1, 4, 4))
    with pytest.raises(ValueError, match="max_passes"):
        s.thin(good, -1)
    with pytest.raises(ValueError, match="class"):
        s.counts(good, good, c=0)
    with pytest.raises(ValueError, match="ignore_index"):
        s.counts(good, good, c=2, ignore_index=2)
    with pytest.raises(ValueError, match="differ"):
        s.counts(good, dev(np.ones((4, 5), np.int32)))
    with pytest.raises(ValueError, match="out must"):
        s.counts(good, good, out=torch.zeros(5, dtype=torch.int64, device=DEV))


def pair(seed, N, H, W, classes=2, ignore=None):
    rng = np.random.default_rng(seed)
    t = np.stack([mixed(H, W, seed * 10 + n, classes) for n in range(N)])
    p = np.stack([np.roll(m, (1, 2), (0, 1)) for m in t])  # near the target, not on it
    p = np.where(rng.random(p.shape) < 0.02, 0, p).astype(np.int32)
    if ignore is not None:
        t = np.where(rng.random(t.shape) < 0.1, ignore, t).astype(np.int32)
    return p, t


def test_counts_classes_ignore_and_accumulation():
    s = _s()
    p1, t1 = pair(1, 2, 70, 45, ignore=5)
    p2, t2 = pair(2, 3, 70, 45, ignore=5)
    for c in (1, 2):
        w1, w2 = ref.counts(p1, t1, c, 5), ref.counts(p2, t2, c, 5)
        assert w1[1] > 0 and w1[3] > 0 and 0 < w1[0] < w1[1] and w1[4] == 0 and w1[5] == 2  # the case says something
        got = s.counts(dev(p1), dev(t1), c, ignore_index=5)
        assert got.dtype == torch.int64 and got.tolist() == w1
        back = s.counts(dev(p2), dev(t2), c, ignore_index=5, out=got)
        assert back is got and got.tolist() == [a + b for a, b in zip(w1, w2)]
        assert s.metrics_from_counts(got) == ref.metrics_from_counts(got.tolist())
    # without ignore_index the value 5 is just another class
    assert s.counts(dev(p1), dev(t1), 1).tolist() == ref.counts(p1, t1, 1)
    assert ref.counts(p1, t1, 1) != ref.counts(p1, t1, 1, 5)


def test_counts_report_unconverged_images():
    s = _s()
    _, _, k = s.tile()
    t = np.stack([np.ones((70, 45), np.int32), ref.thin_lines(70, 45), np.zeros((70, 45), np.int32)])
    p = np.stack([ref.thin_lines(70, 45), np.ones((70, 45), np.int32), np.zeros((70, 45), np.int32)])
    want = ref.counts(p, t, 1, max_passes=k + 1)
    assert want[4] == 2 and want[5] == 3
    got = s.counts(dev(p), dev(t), 1, max_passes=k + 1)
    assert got.tolist() == want
    with pytest.raises(RuntimeError, match="2 of 3"):
        s.metrics_from_counts(got)
    acc = s.Accumulator({"max_passes": k + 1})
    acc.add(dev(p), dev(t))
    with pytest.raises(RuntimeError, match="max_passes"):
        acc.metrics()


def test_accumulator_means_over_classes_with_a_target_skeleton():
    s = _s()
    p, t = pair(3, 2, 70, 45, classes=2)
    acc = s.Accumulator({}, classes=(1, 2, 3))  # class 3 is nowhere: it does not enter the mean
    acc.add(dev(p), dev(t).long())
    per = [ref.metrics_from_counts(ref.counts(p, t, c)) for c in (1, 2)]
    assert acc.metrics() == {k: sum(m[k] for m in per) / 2 for k in s.KEYS}
    assert acc.out.tolist() == [ref.counts(p, t, c) for c in (1, 2, 3)]


def test_two_streams_give_the_same_bits():
    s = _s()
    tw, th, _ = s.tile()
    a = dev(np.stack([mixed(th + 3, 2 * tw + 1, 31), np.ones((th + 3, 2 * tw + 1), np.int32)]))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append(s.thin(a, return_unconverged=True))
        st.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


class Tiny(torch.nn.Module):
    """a small real model whose k-th answer also carries the k-th prior, so that its prediction is near the target"""

    def __init__(self, net, priors):
        super().__init__()
        self.net, self.priors, self.k = net, priors, 0

    def forward(self, x):
        out = self.net(x) + self.priors[self.k]
        self.k += 1
        return out


def test_evaluate_binary_reports_the_reference_metrics():
    from model.model_factory import build_model
    from unetseg_hip.boundary import labels_from_logits
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_binary

    s = _s()
    torch.manual_seed(5)
    net = build_model("unet_plain", num_classes=2).to(DEV).eval()
    batches, priors = [], []
    for k in range(2):
        x, y = make_batch(2, 64, seed=70 + k)
        near = torch.from_numpy(np.stack([np.roll(m, (1, 2), (0, 1)) for m in y.numpy()])).float()
        prior = torch.zeros(2, 2, 64, 64)
        prior[:, 1] = 8.0 * (near - 0.5)
        batches.append((x, y, None))
        priors.append(prior.to(DEV))
    want = [0] * 6
    with torch.no_grad():
        model = Tiny(net, priors)
        for x, y, _ in batches:
            pred = labels_from_logits(model(x.to(DEV))).cpu().numpy()
            want = [a + b for a, b in zip(want, ref.counts(pred, y.numpy().astype(np.int32), 1))]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None)
        none = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, skeleton=None)
        met = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, skeleton={})
        both = evaluate_binary(Tiny(net, priors), batches, DEV, "bce", None, skeleton={"max_passes": 40},
                               boundary={"tolerance": 2.0, "biou_d": None})
    assert set(plain) == {"Dice", "IoU", "Precision", "Recall", "Accuracy", "Loss"} and none == plain
    assert set(met) == set(plain) | set(s.KEYS)
    assert {k: met[k] for k in plain} == plain
    want_m = ref.metrics_from_counts(want)
    assert {k: met[k] for k in s.KEYS} == want_m == {k: both[k] for k in s.KEYS}
    assert 0.0 < want_m["clDice"] < 1.0 and want[3] > 0  # the case says something
    assert "Boundary F1" in both


def test_evaluate_multitask_and_multiclass_take_the_option():
    from model.unet_multitask import MultiTaskLoss
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate, evaluate_multitask

    s = _s()

    class Fixed(torch.nn.Module):
        def __init__(self, outs):
            super().__init__()
            self.outs, self.k = outs, 0

        def forward(self, x):
            self.k += 1
            return self.outs[self.k - 1]

    x, y, c = make_batch(2, 64, seed=81, with_cls=True)
    near = torch.from_numpy(np.stack([np.roll(m, (2, 1), (0, 1)) for m in y.numpy()])).float()
    seg = (6.0 * (near - 0.5)).view(2, 1, 64, 64).to(DEV)
    cls_logits = torch.zeros(2, 3, device=DEV)
    batches = [(x, y.float().view(2, 1, 64, 64), None, c)]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss())
        met = evaluate_multitask(Fixed([(seg, cls_logits)]), batches, DEV, MultiTaskLoss(), skeleton={})
    pred = (seg[:, 0] > 0).cpu().numpy().astype(np.int32)
    assert {k: met[k] for k in plain} == plain and set(met) == set(plain) | set(s.KEYS)
    assert {k: met[k] for k in s.KEYS} == ref.metrics_from_counts(ref.counts(pred, y.numpy().astype(np.int32), 1))

    # multiclass: three classes and the ignored value num_classes; the mean over the classes with a target skeleton
    p, t = pair(9, 2, 64, 64, classes=2, ignore=3)
    logits = torch.full((2, 3, 64, 64), -4.0)
    logits.scatter_(1, torch.from_numpy(p).long().unsqueeze(1), 4.0)
    tgt = torch.from_numpy(t).long()
    onehot = torch.nn.functional.one_hot(tgt, 4).float()
    mc = [(torch.zeros(2, 3, 64, 64), tgt, onehot)]
    with contextlib.redirect_stdout(io.StringIO()):
        plain = evaluate(Fixed([logits.to(DEV)]), mc, DEV, True, False, 3)
        met = evaluate(Fixed([logits.to(DEV)]), mc, DEV, True, False, 3, skeleton={})
    assert {k: met[k] for k in plain} == plain and set(met) == set(plain) | set(s.KEYS)
    per = [ref.metrics_from_counts(ref.counts(p, t, c_, 3)) for c_ in (1, 2)]
    assert {k: met[k] for k in s.KEYS} == {k: sum(m[k] for m in per) / 2 for k in s.KEYS}


def stub_model(C, tile, seed=3):
    """a callable returning the same fixed logits for every tile: blocky noise, so that the label map has regions"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(1, C, tile // 8, tile // 8, generator=g)
    fixed = (torch.nn.functional.interpolate(coarse, size=(tile, tile), mode="nearest")
             + 0.3 * torch.randn(1, C, tile, tile, generator=g)).to(DEV)
    return lambda x: fixed.expand(x.shape[0], -1, -1, -1)


def test_predict_skeleton_png_and_component_column(tmp_path):
    import ccl_ref
    import predict
    from augment_data import make_image
    from PIL import Image

    path = tmp_path / "a.png"
    image = make_image(np.random.default_rng(4), 130, 90)
    image.save(path)
    model = stub_model(3, 64, seed=8)
    kw = dict(mix_type=True, device=DEV, tile=64, overlap=16)
    folders = [tmp_path / n for n in ("plain", "skel")]
    for f in folders:
        os.mkdir(f)
    plain = predict.detect_image(str(path), model, 3, str(folders[0]), min_area=8, max_hole=6, components=True, **kw)
    saved = predict.detect_image(str(path), model, 3, str(folders[1]), min_area=8, max_hole=6, components=True,
                                 skeleton=True, **kw)
    assert sorted(os.listdir(folders[0])) == ["a_components.json", "a_mask.png"]
    assert sorted(os.listdir(folders[1])) == ["a_components.json", "a_mask.png", "a_skeleton.png"]
    assert open(plain, "rb").read() == open(saved, "rb").read()  # the mask is what it was
    labels = predict.predict_labels_tiled(model, predict.cvtColor(image), DEV, tile=64, overlap=16)
    cleaned = ccl_ref.clean(labels, 8, 6, 8)
    want = ref.thin(cleaned)[0]
    assert (want != 0).sum() > 20
    png = np.array(Image.open(folders[1] / "a_skeleton.png"))
    assert png.shape == (90, 130, 3)
    colors = np.array(predict.colors_for(3), np.uint8)
    colors[0] = 0
    assert np.array_equal(png, colors[want])
    assert np.array_equal(png.any(-1), want != 0)
    rows = json.load(open(folders[1] / "a_components.json"))
    old = json.load(open(folders[0] / "a_components.json"))
    assert [{k: v for k, v in r.items() if k != "skeleton_px"} for r in rows] == old
    assert sum(r["skeleton_px"] for r in rows) == int((want != 0).sum())
    assert all(1 <= r["skeleton_px"] <= r["area"] for r in rows)
    # per component: the table is ordered by root index, as the roots of the non-zero pixels are when sorted
    root = ccl_ref.label(cleaned, 8)
    roots = np.unique(root[cleaned != 0])
    assert len(roots) == len(rows)
    assert [r["skeleton_px"] for r in rows] == [int(((want != 0) & (root == q)).sum()) for q in roots]


def test_predict_cli_with_skeleton(tmp_path):
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
    saved = predict.predict(predict.parse_args(base + ["--skeleton"]))
    assert open(first[0], "rb").read() == open(saved[0], "rb").read()
    assert not os.path.exists(first[0].replace("_mask.png", "_skeleton.png"))
    assert os.path.exists(saved[0].replace("_mask.png", "_skeleton.png"))
    with pytest.raises(ValueError, match="connectivity"):
        args = predict.parse_args(base + ["--skeleton"])
        args.connectivity = 6
        predict.predict(args)
