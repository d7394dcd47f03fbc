"""numpy / Python restatement of the boundary semantics (csrc/boundary.hip, unetseg_hip/boundary.py).

Written for clarity and independence from the kernels, not for speed: the edge map by shifted
comparisons, the distance transform as a column pass followed by a brute-force minimum over every
column of the row (int64, no window, no envelope), the counts by numpy histograms, and the metrics
restated from their definitions.  tests/test_boundary_cpu.py holds this file to scipy and to
hand-written maps; tests/test_gpu_boundary.py holds the kernels to this file, integer for integer.
"""
import math

import numpy as np

INF = 1 << 30


def _batched(a):
    a = np.asarray(a)
    return (a[None], True) if a.ndim == 2 else (a, False)


def edges(cls, c=1, ignore=None):
    """uint8 like cls: class-c pixels with an in-image, non-ignored edge neighbour of another class"""
    m, squeeze = _batched(cls)
    own = m == c
    if ignore is not None:
        own = own & (m != ignore)
    other = m != c  # a neighbour that can make an edge
    if ignore is not None:
        other = other & (m != ignore)
    near = np.zeros(m.shape, bool)
    near[:, 1:, :] |= other[:, :-1, :]   # the neighbour above
    near[:, :-1, :] |= other[:, 1:, :]   # below
    near[:, :, 1:] |= other[:, :, :-1]   # left
    near[:, :, :-1] |= other[:, :, 1:]   # right; nothing comes in over the frame
    e = (own & near).astype(np.uint8)
    return e[0] if squeeze else e


def _sqdist_one(s):
    H, W = s.shape
    g = np.full((H, W), INF, np.int64)  # squared distance to the nearest site of the own column
    for x in range(W):
        ys = np.flatnonzero(s[:, x])
        if len(ys):
            g[:, x] = (np.abs(np.arange(H)[:, None] - ys[None, :]).min(1).astype(np.int64)) ** 2
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2  # [x][x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (g[y][None, :] + dx2).min(1)  # INF + dx2 stays far above any real distance in int64
    return np.minimum(out, INF).astype(np.int32)


def sqdist(sites):
    """int32 like sites: exact squared Euclidean distance to the nearest non-zero pixel of the same image"""
    s, squeeze = _batched(np.asarray(sites) != 0)
    out = np.stack([_sqdist_one(im) for im in s])
    return out[0] if squeeze else out


def counts(pred, target, c=1, K=4096, biou_d2=None, ignore=None, biou_d=None):
    """int64 [2 (K + 2) + 2]: the two histograms, then intersection and union; biou_d2 given, or from
    biou_d (pixels), or from 2 % of the diagonal"""
    p, _ = _batched(pred)
    t, _ = _batched(target)
    N, H, W = p.shape
    if biou_d2 is None:
        if biou_d is None:
            biou_d = default_biou_d(H, W, K)
        biou_d2 = biou_d * biou_d
    eP, eG = edges(p, c, ignore), edges(t, c, ignore)
    dP, dG = sqdist(eP), sqdist(eG)
    out = np.zeros(2 * (K + 2) + 2, np.int64)
    out[:K + 2] = np.bincount(np.minimum(dG[eP == 1], K + 1), minlength=K + 2)
    out[K + 2:2 * K + 4] = np.bincount(np.minimum(dP[eG == 1], K + 1), minlength=K + 2)
    keep = np.ones(t.shape, bool) if ignore is None else t != ignore
    Pd = (p == c) & (dP <= biou_d2) & keep
    Gd = (t == c) & (dG <= biou_d2) & keep
    out[2 * K + 4] = int((Pd & Gd).sum())
    out[2 * K + 5] = int((Pd | Gd).sum())
    return out


def default_biou_d(H, W, K=4096):
    d = int(round(0.02 * math.sqrt(H * H + W * W)))
    return max(1, min(d, int(math.floor(math.sqrt(K)))))


def metrics_from_counts(c, K, tolerance=2.0):
    c = np.asarray(c, dtype=np.int64)
    assert c.shape == (2 * (K + 2) + 2,)
    assert tolerance * tolerance <= K
    hp, hg = c[:K + 2], c[K + 2:2 * K + 4]
    n_p, n_g = int(hp.sum()), int(hg.sum())
    within = np.arange(K + 2) <= tolerance * tolerance  # the overflow bin K + 1 is never within
    within[K + 1] = False
    if n_p:
        prec = float(hp[within].sum()) / n_p
    else:
        prec = 1.0 if n_g == 0 else 0.0
    if n_g:
        rec = float(hg[within].sum()) / n_g
    else:
        rec = 1.0 if n_p == 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    inter, union = int(c[2 * K + 4]), int(c[2 * K + 5])
    biou = inter / union if union else 1.0
    pooled = np.cumsum(hp + hg)
    if n_p + n_g == 0:
        hd95 = 0.0
    else:
        b = int(np.argmax(100 * pooled >= 95 * (n_p + n_g)))  # the first bin that reaches 95 %
        hd95 = math.inf if b == K + 1 else math.sqrt(b)
    return {"Boundary Precision": prec, "Boundary Recall": rec, "Boundary F1": f1, "Boundary IoU": biou,
            "HD95": hd95}
