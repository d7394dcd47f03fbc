"""numpy reference of the score histogram (csrc/curve.hip) and of the curve metrics (unetseg_hip/curve.py).

The histogram side follows the kernel's contract with the caller's edge array: ``z`` is formed with one fp32
subtraction, the bin is ``np.searchsorted(edges, z, side="left")`` (the number of edges below ``z``; an equal
value stays in the lower bin) with NaN mapped to bin 0.  The metric side never sees a histogram: it works on
the individual pixels' quantised scores (their bins) and labels by sorting, cumulative sums and the rank
statistic, in float64.
"""
from fractions import Fraction

import numpy as np


def z_of(outputs):
    """fp32 [B, P]: o0 of a one-channel head, o1 - o0 (fp32) of a two-channel one; outputs [B, nch, H, W]"""
    o = np.asarray(outputs, dtype=np.float32)
    o = o.reshape(o.shape[0], o.shape[1], -1)
    with np.errstate(all="ignore"):  # inf - inf and overflow are cases, not mistakes
        return o[:, 0] if o.shape[1] == 1 else (o[:, 1] - o[:, 0]).astype(np.float32)


def int_target(targets, ignore_index=None):
    """int64, flat: a float target is class 1 where it equals 1, ``ignore_index`` kept (losses._prep)"""
    t = np.asarray(targets)
    if np.issubdtype(t.dtype, np.floating):
        lab = (t == 1).astype(np.int64)
        if ignore_index is not None:
            lab = np.where(t == ignore_index, np.int64(ignore_index), lab)
        t = lab
    return t.astype(np.int64).reshape(-1)


def bins_of(z, edges):
    """the bin of every score: the number of edges below it, NaN -> 0"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    b = np.searchsorted(np.asarray(edges, dtype=np.float32), z, side="left")
    b[np.isnan(z)] = 0
    return b.astype(np.int64)


def scores(outputs, targets, edges, ignore_index=None):
    """(bins, labels) of the valid pixels: int64 arrays; label = (target == 1)"""
    b = bins_of(z_of(outputs), edges)
    t = int_target(targets, ignore_index)
    assert b.shape == t.shape, (b.shape, t.shape)
    valid = np.ones(t.shape, bool) if ignore_index is None else t != ignore_index
    return b[valid], (t[valid] == 1).astype(np.int64)


def hist(outputs, targets, edges, ignore_index=None):
    """int64 [2, K]: row = (target == 1), column = bin"""
    K = len(edges) + 1
    b, y = scores(outputs, targets, edges, ignore_index)
    return np.stack([np.bincount(b[y == 0], minlength=K), np.bincount(b[y == 1], minlength=K)]).astype(np.int64)


def confusion_at(bins, labels, k):
    """(tp, fp, fn, tn) of the prediction bin >= k"""
    pred = bins >= k
    pos = labels == 1
    return (int((pred & pos).sum()), int((pred & ~pos).sum()), int((~pred & pos).sum()), int((~pred & ~pos).sum()))


def _div(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def metrics(bins, labels, K, ece_bins=10, threshold_k=None):
    """the keys of curve.metrics_from_counts from per-pixel quantised scores, brute force"""
    bins, labels = np.asarray(bins, np.int64), np.asarray(labels, np.int64)
    n, P = len(bins), int(labels.sum())
    N = n - P
    # best IoU: every threshold counted on the pixels; exact comparison, the tie to the k nearest K / 2, then lower
    best = None
    for k in range(1, K):
        tp, fp, fn, _ = confusion_at(bins, labels, k)
        iou = Fraction(tp, tp + fp + fn) if tp + fp + fn else Fraction(0)
        key = (-iou, abs(2 * k - K), k)
        if best is None or key < best[0]:
            best = (key, k, tp, fp, fn)
    _, kb, tp, fp, fn = best
    out = {"Best Threshold": kb / K, "Best IoU": _div(tp, tp + fp + fn), "Best F1": _div(2 * tp, 2 * tp + fp + fn)}
    tp, fp, fn, _ = confusion_at(bins, labels, K // 2)
    out["IoU@0.5"] = _div(tp, tp + fp + fn)
    # AP: scores sorted descending, one step per group of equal scores
    ap = 0.0
    if P > 0:
        order = np.argsort(-bins, kind="stable")
        sb, sy = bins[order], labels[order]
        ctp = np.cumsum(sy)
        ends = np.nonzero(np.append(sb[1:] != sb[:-1], True))[0]  # the last pixel of every group
        prev = 0
        for e in ends:
            t = int(ctp[e])
            ap += (t - prev) / P * (t / (e + 1))
            prev = t
    out["AP"] = ap
    # AUROC: Mann-Whitney U from average ranks
    if P > 0 and N > 0:
        uniq, inv, cnt = np.unique(bins, return_inverse=True, return_counts=True)
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])  # pixels ranked before the group
        avg_rank = first + (cnt + 1) / 2.0
        ranks = avg_rank[inv]
        u = ranks[labels == 1].sum() - P * (P + 1) / 2.0
        out["AUROC"] = float(u) / (float(P) * float(N))
    else:
        out["AUROC"] = 0.5
    # ECE over ece_bins equal-width probability groups, confidence = the fine-bin midpoint
    ece = 0.0
    if n > 0:
        conf = (bins + 0.5) / K
        grp = bins // (K // ece_bins)
        for m in range(ece_bins):
            sel = grp == m
            nm = int(sel.sum())
            if nm:
                ece += nm / n * abs(labels[sel].mean() - conf[sel].mean())
    out["ECE"] = ece
    if threshold_k is not None:
        tp, fp, fn, _ = confusion_at(bins, labels, threshold_k)
        out.update({"IoU@T": _div(tp, tp + fp + fn), "F1@T": _div(2 * tp, 2 * tp + fp + fn),
                    "Precision@T": _div(tp, tp + fp), "Recall@T": _div(tp, tp + fn)})
    return out


def expand(hist):
    """(bins, labels) of a histogram's pixels, for feeding ``metrics`` from hand-written counts"""
    h = np.asarray(hist, np.int64)
    K = h.shape[1]
    bins = np.concatenate([np.repeat(np.arange(K), h[0]), np.repeat(np.arange(K), h[1])])
    labels = np.concatenate([np.zeros(int(h[0].sum()), np.int64), np.ones(int(h[1].sum()), np.int64)])
    return bins, labels
