"""numpy restatement of the thinning rule, the counts and the metrics of unetseg_hip/skeleton.py
(include/unetseg_hip.h, "hard skeleton"): Guo & Hall's algorithm A1 per class, as vectorised shifts on a
zero-padded copy.  Nothing here is shared with the kernel or with skeleton.py."""
import numpy as np

MAX_CLASS = 255


def default_max_passes(H, W):
    return min(H, W) // 2 + 8


def _neighbours(a):
    """the eight [H,W] bool maps "that neighbour lies inside the image and has my class", P2 .. P9"""
    H, W = a.shape
    p = np.zeros((H + 2, W + 2), a.dtype)
    p[1:-1, 1:-1] = a
    fg = a != 0

    def at(dy, dx):
        return fg & (p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == a)

    #        P2         P3         P4        P5        P6        P7         P8         P9
    return (at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1))


def subiteration(a, second):
    """(the map after one subiteration, the number of pixels it deleted)"""
    P2, P3, P4, P5, P6, P7, P8, P9 = _neighbours(a)
    i = lambda b: b.astype(np.int32)  # noqa: E731
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N1 = i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8)
    N2 = i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9)
    N = np.minimum(N1, N2)
    m = ((P2 | P3 | ~P5) & P4) if second else ((P6 | P7 | ~P9) & P8)
    kill = (a != 0) & (C == 1) & (N >= 2) & (N <= 3) & ~m
    out = a.copy()
    out[kill] = 0
    return out, int(kill.sum())


def thin_image(a, max_passes=None):
    """a [H,W] integer -> (skeleton, passes executed, unconverged): passes run until one deletes nothing (that
    one is counted) or ``max_passes`` have run; unconverged iff the last pass executed deleted a pixel.  Values
    outside 0 .. 255 count as background."""
    a = np.asarray(a)
    H, W = a.shape
    cap = default_max_passes(H, W) if max_passes is None else int(max_passes)
    cur = np.where((a >= 1) & (a <= MAX_CLASS), a, 0).astype(np.int32)
    passes, deleted = 0, 0
    while passes < cap:
        cur, d1 = subiteration(cur, False)
        cur, d2 = subiteration(cur, True)
        passes += 1
        deleted = d1 + d2
        if deleted == 0:
            break
    return cur, passes, int(passes > 0 and deleted > 0)


def thin(cls, max_passes=None):
    """[H,W] or [N,H,W] -> (skeletons of the same shape, unconverged int32 [N])"""
    a = np.asarray(cls)
    batch = a[None] if a.ndim == 2 else a
    res = [thin_image(m, max_passes) for m in batch]
    sk = np.stack([r[0] for r in res]).astype(np.int32).reshape(a.shape)
    return sk, np.array([r[2] for r in res], np.int32)


def counts(pred, target, c=1, ignore_index=None, max_passes=None):
    """the six counts of unetseg_skel_counts as a list of ints; pred, target [N,H,W]"""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 2:
        pred, target = pred[None], target[None]
    valid = np.ones(target.shape, bool) if ignore_index is None else target != ignore_index
    p, t = np.where(valid, pred, 0), np.where(valid, target, 0)
    sp, up = thin(p, max_passes)
    st, ut = thin(t, max_passes)
    return [int(((sp == c) & (t == c) & valid).sum()), int(((sp == c) & valid).sum()),
            int(((st == c) & (p == c) & valid).sum()), int(((st == c) & valid).sum()), int(((up | ut) != 0).sum()),
            int(pred.shape[0])]


def metrics_from_counts(c):
    c0, c1, c2, c3, c4, c5 = (int(v) for v in c)
    if c4 > 0:
        raise RuntimeError(f"{c4} of {c5} images not converged")
    tprec = c0 / c1 if c1 > 0 else (1.0 if c3 == 0 else 0.0)
    tsens = c2 / c3 if c3 > 0 else (1.0 if c1 == 0 else 0.0)
    cl = 2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0 else 0.0
    return {"clDice": cl, "Skeleton Precision": tprec, "Skeleton Recall": tsens}


# ---- seeded maps of the three kinds the rule was chosen on -----------------------------------------------
def _smooth(a, rounds):
    for _ in range(rounds):
        p = np.pad(a, 1, mode="edge")
        a = sum(p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3)) / 9.0
    return a


def random_map(kind, H, W, rng, classes=1):
    """kind 0: random noise, 1: smoothed blobs, 2: dilated points; values 0 .. classes"""
    if kind == 0:
        m = rng.random((H, W)) < rng.uniform(0.2, 0.8)
    elif kind == 1:
        m = _smooth(rng.random((H, W)), 3) > 0.5
    else:
        m = np.zeros((H, W), bool)
        for _ in range(max(1, H * W // 60)):
            y, x, r = rng.integers(0, H), rng.integers(0, W), rng.integers(0, 4)
            m[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    lab = m.astype(np.int32)
    if classes > 1:
        lab = lab * rng.integers(1, classes + 1, (H, W)).astype(np.int32)
        if kind != 0:  # classes in vertical bands, so that regions stay regions
            bands = (np.arange(W) * classes // max(W, 1)) + 1
            lab = m.astype(np.int32) * bands[None, :].astype(np.int32)
    return lab


def disc(size, r):
    yy, xx = np.mgrid[:size, :size]
    c = (size - 1) / 2.0
    return (((yy - c) ** 2 + (xx - c) ** 2) <= r * r).astype(np.int32)


def thin_lines(H, W):
    """a few bars three pixels wide and some one pixel wide, crossing"""
    a = np.zeros((H, W), np.int32)
    a[H // 4:H // 4 + 3, 2:W - 2] = 1
    a[2:H - 2, W // 3:W // 3 + 3] = 1
    a[H // 2, :] = 1
    for i in range(min(H, W) - 4):
        a[2 + i, 2 + i:4 + i] = 1
    return a

