"""Operating-point and calibration metrics of the binary head from a score histogram on the HIP path
(csrc/curve.hip).

Every binary decision of the project is taken at probability 0.5 (``losses.binary_confusion``,
``classmap.labels_from_logits``).  ``hist`` bins the logit ``z`` (``o0`` of a one-channel head, ``o1 - o0`` of a
two-channel one) of every valid pixel against a fixed table of K - 1 logit thresholds, ``edges``, separately for
positive (target == 1) and negative pixels.  Threshold k stands for probability k / K: its edge is
``theta_k = logit(k / K)``, the prediction at it is ``z > theta_k``, which is ``bin >= k``, and k = K / 2 is the
project's 0.5 rule (``theta == 0.0``).  The kernel only compares ``z`` with the table (no ``exp``), so the counts
are integers that a CPU reference holding the same table reproduces exactly, and they are bitwise reproducible.
``hist`` runs on the current stream, never waits on the host and accumulates, so a split costs one host read;
``table`` and ``metrics_from_counts`` read the confusion counts at every threshold, the best-IoU threshold, AP,
AUROC and the calibration error from it on the host.
"""
from __future__ import annotations

import math

import torch

from .classmap import _ignore, _out_counts, _stream
from .lib import lib
from .losses import _prep

KEYS = ("Best Threshold", "Best IoU", "Best F1", "IoU@0.5", "AP", "AUROC", "ECE")
#: the additional keys of ``metrics_from_counts(..., threshold=t)``
KEYS_AT = ("IoU@T", "F1@T", "Precision@T", "Recall@T")
#: the largest K (unetseg_curve_max_bins)
MAX_BINS = 4096

_EDGES = {}


def _check_bins(K):
    K = int(K)
    if not 2 <= K <= MAX_BINS or K % 2:
        raise ValueError(f"K must be even and lie in 2 .. {MAX_BINS}, got {K}")
    return K


def edges(K=1000, device=None):
    """fp32 [K - 1] on ``device`` (None: the host): ``theta_k = float32(log(k / (K - k)))`` for k = 1 .. K - 1,
    computed in float64 on the host; entry k - 1 holds theta_k.  K is even, so ``theta_{K/2} == 0.0`` exactly
    and the curve contains the 0.5 rule; the upper half is the negation of the lower, so the table is
    antisymmetric bit for bit.  Cached per (K, device): do not write to it."""
    K = _check_bins(K)
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    e = _EDGES.get((K, device))
    if e is None:
        lower = torch.tensor([math.log(k / (K - k)) for k in range(1, K // 2)], dtype=torch.float64).to(torch.float32)
        e = torch.cat([lower, torch.zeros(1, dtype=torch.float32), -lower.flip(0)]).to(device)
        _EDGES[(K, device)] = e
    return e


def _threshold_k(threshold, K):
    """the k of a threshold on the grid k / K, 1 <= k <= K - 1"""
    k = round(float(threshold) * K)
    if not 1 <= k <= K - 1 or abs(float(threshold) * K - k) > 1e-9 * K:
        raise ValueError(f"threshold {threshold} is not k / {K} for an integer 1 <= k <= {K - 1}")
    return k


def hist(outputs, targets, K=1000, ignore_index=None, out=None):
    """device int64 [2, K] (+)= the score histogram of logits ``outputs`` [B,1,H,W] or [B,2,H,W]: row 1 counts the
    pixels whose target is 1, row 0 every other valid pixel, column = the number of ``edges(K)`` below the
    pixel's ``z``.  ``outputs`` and ``targets`` are read as ``losses.binary_confusion`` reads them (a float target
    is class 1 where it equals 1, ``ignore_index`` kept); pixels whose target is ``ignore_index`` are skipped.
    ``out`` is added to and returned when given.  Runs on the current stream without a host sync."""
    K = _check_bins(K)
    if not torch.is_tensor(outputs) or outputs.dim() != 4 or outputs.shape[1] not in (1, 2):
        raise ValueError("outputs must be logits [B,1,H,W] or [B,2,H,W]")
    o, tgt, _ = _prep(outputs, targets, ignore_index)
    B, nch, Pn = o.shape[0], o.shape[1], o.shape[2] * o.shape[3]
    if tgt.numel() != B * Pn or tgt.device != o.device:
        raise ValueError(f"targets {tuple(targets.shape)} on {tgt.device} do not match outputs {tuple(outputs.shape)} "
                         f"on {o.device}")
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != (2, K) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 [2, {K}] tensor on {o.device}")
    flat = _out_counts(None if out is None else out.view(-1), 2 * K, o.device)
    if B * Pn == 0:  # an empty batch has no storage to point at
        return flat.view(2, K) if out is None else out
    lib.curve_hist(o.data_ptr(), nch, tgt.data_ptr(), B, Pn, _ignore(ignore_index), edges(K, o.device).data_ptr(), K,
                   flat.data_ptr(), _stream(o))
    return flat.view(2, K) if out is None else out


def labels_at(outputs, threshold, K=1000):
    """int32 [B,H,W] class map of logits [B,1,H,W] or [B,2,H,W] at ``threshold`` = k / K (an integer
    1 <= k <= K - 1, else ValueError): ``z > theta_k``, the rule ``table`` counts at row k, in torch ops on the
    tensor's device.  At threshold 0.5 it equals ``classmap.labels_from_logits``."""
    K = _check_bins(K)
    k = _threshold_k(threshold, K)
    if not torch.is_tensor(outputs) or outputs.dim() != 4 or outputs.shape[1] not in (1, 2):
        raise ValueError("outputs must be logits [B,1,H,W] or [B,2,H,W]")
    o = outputs.detach().float()
    z = o[:, 0] if o.shape[1] == 1 else o[:, 1] - o[:, 0]
    return (z > edges(K, o.device)[k - 1]).to(torch.int32)


def _rows(hist):
    """(neg, pos, K): the two histogram rows as lists of ints"""
    h = hist.tolist() if hasattr(hist, "tolist") else hist
    if len(h) != 2 or len(h[0]) != len(h[1]):
        raise ValueError("hist must be [2, K]")
    neg, pos = [int(v) for v in h[0]], [int(v) for v in h[1]]
    return neg, pos, _check_bins(len(neg))


def _suffix(row):
    """s[k] = sum(row[k:]) for k = 0 .. len(row)"""
    s = [0] * (len(row) + 1)
    for b in range(len(row) - 1, -1, -1):
        s[b] = s[b + 1] + row[b]
    return s


def table(hist):
    """host: the integer rows ``(k, tp, fp, fn, tn)`` for k = 0 .. K of a ``hist`` array (tensor, array or nested
    list): the confusion counts of the prediction ``bin >= k`` (``z > theta_k``), suffix sums of the two histogram
    rows.  k = 0 predicts everything positive, k = K nothing."""
    neg, pos, K = _rows(hist)
    tp, fp = _suffix(pos), _suffix(neg)
    return [(k, tp[k], fp[k], tp[0] - tp[k], fp[0] - fp[k]) for k in range(K + 1)]


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def metrics_from_counts(hist, ece_bins=10, threshold=None):
    """host, float64: the ``KEYS`` from a ``hist`` array.

    * ``Best Threshold`` k / K, ``Best IoU``, ``Best F1``: the k in 1 .. K - 1 with the largest
      IoU = tp / (tp + fp + fn) (F1 = 2 IoU / (1 + IoU) is monotone in it, so one argmax serves both); a tie goes
      to the k nearest K / 2, then to the lower k; IoU and F1 with an empty union are 0.
    * ``IoU@0.5``: the same expression at k = K / 2, the project's decision rule.
    * ``AP`` = sum over k = K - 1 .. 0 of (R_k - R_{k+1}) Prec_k with R_K = 0: the step-wise average precision of
      the bin-quantised score; 0 without a positive.
    * ``AUROC`` = sum_b pos[b] (neg_below[b] + neg[b] / 2) / (P N): Mann-Whitney with the ties inside a bin counted
      half; 0.5 when there is no positive or no negative.
    * ``ECE`` = sum_m (n_m / n) |pos_m / n_m - conf_m| over ``ece_bins`` equal-width probability groups (K must be
      a multiple of ``ece_bins``), with conf_m the count-weighted mean of the fine-bin midpoints (b + 1/2) / K.
      This is the reliability of the foreground probability, not of the top-label confidence, and the midpoint
      stands for the pixel's true sigmoid to within 1 / (2 K).  0 without a pixel.

    With ``threshold`` = k / K also ``IoU@T``, ``F1@T``, ``Precision@T`` and ``Recall@T`` at that k (0 for an
    empty denominator).  Counts are compared as integers, so neither the argmax nor a tie depends on rounding."""
    neg, pos, K = _rows(hist)
    M = int(ece_bins)
    if M < 1 or K % M:
        raise ValueError(f"K = {K} must be a multiple of ece_bins = {ece_bins}")
    tp, fp = _suffix(pos), _suffix(neg)
    P, N = tp[0], fp[0]

    def iou_parts(k):  # numerator and denominator; tp + fn = P
        return tp[k], P + fp[k]

    best = None  # (numerator, denominator > 0, tie key, k)
    for k in range(1, K):
        a, b = iou_parts(k)
        if b == 0:  # an empty union counts as 0
            a, b = 0, 1
        key = (abs(2 * k - K), k)
        if best is None or a * best[1] > best[0] * b or (a * best[1] == best[0] * b and key < best[2]):
            best = (a, b, key, k)
    kb = best[3]
    out = {"Best Threshold": kb / K, "Best IoU": _ratio(*iou_parts(kb)),
           "Best F1": _ratio(2 * tp[kb], tp[kb] + P + fp[kb]), "IoU@0.5": _ratio(*iou_parts(K // 2))}
    out["AP"] = sum(pos[k] * _ratio(tp[k], tp[k] + fp[k]) for k in range(K - 1, -1, -1)) / P if P > 0 else 0.0
    if P > 0 and N > 0:
        below, u2 = 0, 0  # u2 = 2 * the rank statistic
        for b in range(K):
            u2 += pos[b] * (2 * below + neg[b])
            below += neg[b]
        out["AUROC"] = float(u2) / (2.0 * float(P) * float(N))
    else:
        out["AUROC"] = 0.5
    n, w, dev = P + N, K // M, 0  # dev = 2 K sum_m |pos_m - sum_b n_b (b + 1/2) / K|
    for m in range(M):
        pm = sum(pos[m * w:(m + 1) * w])
        sm = sum((pos[b] + neg[b]) * (2 * b + 1) for b in range(m * w, (m + 1) * w))
        dev += abs(2 * K * pm - sm)
    out["ECE"] = float(dev) / (2.0 * K * n) if n > 0 else 0.0
    if threshold is not None:
        k = _threshold_k(threshold, K)
        out["IoU@T"] = _ratio(*iou_parts(k))
        out["F1@T"] = _ratio(2 * tp[k], tp[k] + P + fp[k])
        out["Precision@T"] = _ratio(tp[k], tp[k] + fp[k])
        out["Recall@T"] = _ratio(tp[k], P)
    return out


class Accumulator:
    """the score histogram of an evaluation loop: one device array, added to per batch, read once.

    ``options`` is the entry points' ``curve`` dict: ``{"bins": K (default 1000), "ece_bins": M (default 10),
    "threshold": t or None}``; ``t`` must be k / K.  ``out`` is the device int64 [2, K] histogram (None before the
    first batch): a data-parallel caller can all-reduce it before ``metrics``."""

    def __init__(self, options, ignore_index=None):
        unknown = set(options) - {"bins", "ece_bins", "threshold"}
        if unknown:
            raise ValueError(f"unknown curve options {sorted(unknown)}")
        self.K = _check_bins(options.get("bins", 1000))
        self.ece_bins = int(options.get("ece_bins", 10))
        if self.ece_bins < 1 or self.K % self.ece_bins:
            raise ValueError(f"bins = {self.K} must be a multiple of ece_bins = {self.ece_bins}")
        self.threshold = options.get("threshold")
        if self.threshold is not None:
            _threshold_k(self.threshold, self.K)
        self.ignore_index = ignore_index
        self.out = None
        self._host = None

    @property
    def keys(self):
        """the keys ``metrics`` returns, in its order"""
        return KEYS + (KEYS_AT if self.threshold is not None else ())

    def add(self, logits, targets):
        """logits [B,1,H,W] or [B,2,H,W] and targets as ``hist`` takes them"""
        if self.out is None:
            self.out = torch.zeros(2, self.K, dtype=torch.int64, device=logits.device)
        self._host = None
        hist(logits, targets, self.K, self.ignore_index, self.out)

    def counts(self):
        """the histogram on the host (nested lists); the one host read, shared by ``metrics`` and ``table``"""
        if self._host is None:
            self._host = self.out.tolist() if self.out is not None else [[0] * self.K, [0] * self.K]
        return self._host

    def metrics(self):
        return metrics_from_counts(self.counts(), self.ece_bins, self.threshold)

    def table(self):
        return table(self.counts())


def write_csv(path, rows):
    """``curve.csv``: one line per row of ``table``: threshold k / K, tp, fp, fn, tn, precision, recall, iou (a
    ratio with an empty denominator is 0)"""
    import csv

    K = len(rows) - 1
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(["threshold", "tp", "fp", "fn", "tn", "precision", "recall", "iou"])
        for k, tp, fp, fn, tn in rows:
            w.writerow([repr(k / K), tp, fp, fn, tn, repr(_ratio(tp, tp + fp)), repr(_ratio(tp, tp + fn)),
                        repr(_ratio(tp, tp + fp + fn))])


def write_threshold(path, metrics, K):
    """``threshold.json``: ``{"threshold", "bins", "iou", "iou_at_half"}`` from a ``metrics_from_counts`` dict: the
    best-IoU threshold of the split the metrics were counted on, what it scores and what 0.5 scores"""
    import json

    with open(path, "w", encoding="utf-8") as f:
        json.dump({"threshold": metrics["Best Threshold"], "bins": int(K), "iou": metrics["Best IoU"],
                   "iou_at_half": metrics["IoU@0.5"]}, f, indent=2)
