"""numpy / Python restatement of the object-level counts (csrc/objects.hip, unetseg_hip/objects.py) on top of
``ccl_ref.label``: a dict of pairs and the literal definitions, the integer comparisons and the
``floor(inter * 2**32 / union)`` term in Python ints.

For a class ``c`` an object is a component of class ``c`` of a map whose pixels with target ``ignore_index`` were
set to 0 first (in both maps); a predicted object p and a target object g (named by their roots) overlap when
some pixel has pred == c, target == c, root_pred == p and root_target == g; inter(p, g) counts those pixels and
union = area_p + area_g - inter.
"""
import numpy as np

import ccl_ref

N_COUNTS = 20
KEYS = ("PQ", "SQ", "Object F1", "Object Precision", "Object Recall", "Object F1@[.5:.95]", "Detection Recall",
        "False Object Rate", "Split Rate", "Merge Rate")


def _batch(pred, target, ignore_index):
    """both maps as [N][H][W] int32 copies with the ignored pixels zeroed"""
    p, t = np.array(pred, np.int32), np.array(target, np.int32)
    assert p.shape == t.shape and p.ndim in (2, 3)
    if p.ndim == 2:
        p, t = p[None], t[None]
    if ignore_index is not None:
        ign = t == ignore_index
        p[ign] = 0
        t[ign] = 0
    return p, t


def _image(p, t, c, connectivity):
    """(area of every predicted object by root, the same of the target objects, inter by (root_pred, root_target))"""
    rp, rt = ccl_ref.label(p, connectivity).reshape(-1), ccl_ref.label(t, connectivity).reshape(-1)
    pf, tf = p.reshape(-1), t.reshape(-1)
    area_p, area_t, inter = {}, {}, {}
    for i in range(pf.size):
        if pf[i] == c:
            area_p[int(rp[i])] = area_p.get(int(rp[i]), 0) + 1
        if tf[i] == c:
            area_t[int(rt[i])] = area_t.get(int(rt[i]), 0) + 1
        if pf[i] == c and tf[i] == c:
            k = (int(rp[i]), int(rt[i]))
            inter[k] = inter.get(k, 0) + 1
    return area_p, area_t, inter


def counts(pred, target, c=1, connectivity=8, ignore_index=None):
    """the twenty counts as a list of Python ints"""
    out = [0] * N_COUNTS
    P, T = _batch(pred, target, ignore_index)
    if P.size == 0:
        return out
    for p, t in zip(P, T):
        area_p, area_t, inter = _image(p, t, c, connectivity)
        out[0] += len(area_t)
        out[1] += len(area_p)
        deg_p, deg_t = dict.fromkeys(area_p, 0), dict.fromkeys(area_t, 0)
        for (a, b), n in inter.items():
            deg_p[a] += 1
            deg_t[b] += 1
            union = area_p[a] + area_t[b] - n
            for k in range(10, 20):
                out[6 + k - 10] += 20 * n > k * union
            if 2 * n > union:
                out[16] += (n << 32) // union
        out[2] += sum(d >= 1 for d in deg_t.values())
        out[3] += sum(d >= 1 for d in deg_p.values())
        out[4] += sum(d >= 2 for d in deg_t.values())
        out[5] += sum(d >= 2 for d in deg_p.values())
        out[17] += len(inter)
        out[19] += 1
    return out


def pairs(pred, target, c=1, connectivity=8, ignore_index=None):
    """int32 [K][6]: (image, root_pred, root_target, inter, area_pred, area_target), ordered by (image,
    root_target, root_pred)"""
    rows = []
    P, T = _batch(pred, target, ignore_index)
    if P.size:
        for n, (p, t) in enumerate(zip(P, T)):
            area_p, area_t, inter = _image(p, t, c, connectivity)
            rows += [(n, a, b, inter[a, b], area_p[a], area_t[b]) for a, b in sorted(inter, key=lambda k: (k[1], k[0]))]
    return np.array(rows, np.int32).reshape(-1, 6)


def distinct_pairs(pred, target, c=1, connectivity=8, ignore_index=None):
    """the largest number of distinct overlapping pairs in one image"""
    P, T = _batch(pred, target, ignore_index)
    return max((len(_image(p, t, c, connectivity)[2]) for p, t in zip(P, T)), default=0)


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def metrics(counts):
    """the ten keys from twenty counts, float64"""
    c = [int(v) for v in counts]
    assert len(c) == N_COUNTS
    n_gt, n_pred, tp = c[0], c[1], c[6]
    fp, fn = n_pred - tp, n_gt - tp
    S = c[16] / 2**32
    f1 = [_ratio(2 * c[6 + j], n_pred + n_gt) for j in range(10)]
    return {"PQ": _ratio(S, tp + (fp + fn) / 2), "SQ": _ratio(S, tp), "Object F1": f1[0],
            "Object Precision": _ratio(tp, n_pred), "Object Recall": _ratio(tp, n_gt),
            "Object F1@[.5:.95]": sum(f1) / 10, "Detection Recall": _ratio(c[2], n_gt),
            "False Object Rate": 1.0 - _ratio(c[3], n_pred) if n_pred > 0 else 0.0,
            "Split Rate": _ratio(c[4], n_gt), "Merge Rate": _ratio(c[5], n_pred)}


def class_mean(rows):
    """the mean per key over the count rows that have a target object; zeros without one"""
    per = [metrics(r) for r in rows if r[0] > 0]
    if not per:
        return dict.fromkeys(KEYS, 0.0)
    if len(per) == 1:
        return per[0]
    return {k: sum(m[k] for m in per) / len(per) for k in KEYS}


# ---- the maps the GPU tests run (tests/test_gpu_objects.py) and the CPU tests check the capacity claim on -------
FIXED_SIZES = [(1, 1), (1, 70), (70, 1), (2, 2), (63, 63), (64, 64), (65, 65), (129, 129), (37, 130), (130, 37)]
FLIP_SHAPES = [(65, 65), (37, 130)]
FLIP_CASES = [(d, f, conn) for d in (0.30, 0.41, 0.59) for f in (0.02, 0.10) for conn in (4, 8)]


def tile_sizes(T, axis):
    """T - 1, T, T + 1, 2 T + 1 on one axis, an odd size that is no multiple of anything on the other"""
    return [(v, 37) if axis == "H" else (37, v) for v in (T - 1, T, T + 1, 2 * T + 1)]


def noise(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.int32)


def flip_noise(H, W, density, flips, seed):
    """(pred, target): target noise of the density, pred = target with the share `flips` of the pixels flipped"""
    t = noise(H, W, density, seed)
    flip = np.random.default_rng(seed + 1).random((H, W)) < flips
    return np.where(flip, 1 - t, t).astype(np.int32), t


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) % 2 == 0).astype(np.int32)


def stripes(H, W):
    """(pred, target): one-pixel-wide horizontal stripes against vertical ones"""
    y, x = np.mgrid[0:H, 0:W]
    return (y % 2 == 0).astype(np.int32), (x % 2 == 0).astype(np.int32)


def multiclass(N, H, W, classes, seed):
    """(pred, target) of blocky regions of the classes 0 .. classes, pred a perturbed copy of target"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes + 1, (N, (H + 5) // 6, (W + 5) // 6))
    t = np.repeat(np.repeat(coarse, 6, 1), 6, 2)[:, :H, :W].astype(np.int32)
    p = np.where(rng.random(t.shape) < 0.08, rng.integers(0, classes + 1, t.shape), np.roll(t, 1, 2)).astype(np.int32)
    return p, t


def size_map(H, W):
    return flip_noise(H, W, 0.41, 0.10, 1000 * H + W)


def all_maps(tiles):
    """every (name, pred, target, connectivity, class, ignore_index) of the GPU file; tiles: the (tw, th) of
    ccl.tile() and objects.tile()"""
    sizes = list(FIXED_SIZES)
    for tw, th in tiles:
        sizes += tile_sizes(th, "H") + tile_sizes(tw, "W")
    for H, W in dict.fromkeys(sizes):
        for conn in (4, 8):
            yield (f"size {H}x{W} c{conn}", *size_map(H, W), conn, 1, None)
    for H, W in FLIP_SHAPES:
        for k, (d, f, conn) in enumerate(FLIP_CASES):
            yield (f"flip {H}x{W} {d} {f} c{conn}", *flip_noise(H, W, d, f, 50 + k), conn, 1, None)
        for conn in (4, 8):
            yield (f"independent {H}x{W} c{conn}", noise(H, W, 0.5, 7), noise(H, W, 0.45, 8), conn, 1, None)
    for n in (65, 129):
        for conn in (4, 8):
            yield (f"checkerboard {n} c{conn}", checkerboard(n, n), checkerboard(n, n), conn, 1, None)
    yield ("ones 129", np.ones((129, 129), np.int32), np.ones((129, 129), np.int32), 8, 1, None)
    for conn in (4, 8):
        yield (f"stripes c{conn}", *stripes(66, 70), conn, 1, None)
    p, t = multiclass(2, 65, 70, 4, 3)
    for c in (1, 2, 3, 4):
        yield (f"multiclass {c}", p, t, 8, c, None)
