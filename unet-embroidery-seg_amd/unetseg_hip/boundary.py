"""Boundary quality of class maps on the HIP path (csrc/boundary.hip).

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU.  ``edges`` marks the pixels of a class that
touch another class inside the image, ``sqdist`` is the exact squared Euclidean distance transform of a
site map, and ``counts`` reduces a prediction / target pair to two edge-distance histograms and the
Boundary-IoU intersection and union.  ``metrics_from_counts`` reads boundary precision / recall / F1 at a
pixel tolerance, Boundary IoU (Cheng et al., CVPR 2021) and the 95th-percentile Hausdorff distance from
such counts on the host.  All of it is integer and bitwise reproducible; ``edges``, ``sqdist`` and
``counts`` run on the current stream and never wait on the host, and ``counts`` accumulates, so a split
costs one host read.
"""
from __future__ import annotations

import ctypes
import math

import torch

from .classmap import ClassCounts, _ignore, _map, _out_counts, _stream
from .classmap import labels_from_logits  # noqa: F401  (the name callers and INTEGRATION.md use)
from .lib import lib

#: ``sqdist`` of an image without a site (UNETSEG_EDT_INF)
INF = 1 << 30
#: largest K (a squared distance) ``counts`` takes
MAX_K = 65536

KEYS = ("Boundary Precision", "Boundary Recall", "Boundary F1", "Boundary IoU", "HD95")


def chunk():
    """the distance transform works on column segments and row chunks of this many pixels, so its seams
    lie at the multiples"""
    n = ctypes.c_int(0)
    lib.edt_chunk(ctypes.addressof(n))
    return n.value


def edges(cls, c=1, ignore_index=None):
    """uint8, the shape of ``cls``: 1 where the pixel has class ``c`` and one of its four edge neighbours
    lies inside the image, is not ``ignore_index`` and has another class.  The image frame is no
    boundary, and a pixel that is ``ignore_index`` is never an edge pixel."""
    m = _map(cls)
    N, H, W = m.shape
    out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
    lib.boundary_edges(m.data_ptr(), N, H, W, int(c), _ignore(ignore_index), out.data_ptr(), _stream(m))
    return out.view(cls.shape)


def sqdist(sites):
    """int32, the shape of ``sites`` (uint8 or bool, non-zero = site): the exact squared Euclidean distance
    to the nearest site of the same image, ``INF`` everywhere in an image without one"""
    s = _map(sites, "sites", (torch.uint8, torch.bool))
    if s.dtype == torch.bool:
        s = s.view(torch.uint8)
    N, H, W = s.shape
    d2 = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    lib.edt_sqdist(s.data_ptr(), N, H, W, d2.data_ptr(), _stream(s))
    return d2.view(sites.shape)


def default_biou_d(H, W, K=4096):
    """the Boundary-IoU paper's 2 % of the image diagonal in pixels, within [1, floor(sqrt(K))]"""
    return max(1, min(round(0.02 * math.sqrt(H * H + W * W)), math.isqrt(K)))


def counts(pred, target, c=1, K=4096, biou_d=None, ignore_index=None, out=None):
    """device int64 [2 (K + 2) + 2] (+)= the boundary counts of class ``c`` of the int32 maps ``pred`` and
    ``target`` (same shape), with eP / eG their edge maps and dP / dG the distance transforms of those:

    * ``[0 .. K+1]``: the histogram of ``min(dG, K + 1)`` over the edge pixels of ``pred`` (bin K + 1: further
      than K, or the target has no edge);
    * ``[K+2 .. 2K+3]``: the same of ``dP`` over the edge pixels of ``target``;
    * ``[2K+4]``, ``[2K+5]``: intersection and union of {pred == c, dP <= biou_d^2} and
      {target == c, dG <= biou_d^2}, without the pixels whose target is ``ignore_index``.

    ``K`` is a squared distance; ``biou_d`` is in pixels, None = ``default_biou_d(H, W, K)``.  ``out`` is
    added to and returned when given."""
    p, t = _map(pred, "pred"), _map(target, "target")
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f"pred {tuple(p.shape)} on {p.device} and target {tuple(t.shape)} on {t.device} differ")
    N, H, W = p.shape
    K = int(K)
    if not 0 <= K <= MAX_K:
        raise ValueError(f"K must lie in 0 .. {MAX_K}, got {K}")
    d = default_biou_d(H, W, K) if biou_d is None else int(biou_d)
    if d < 0 or d * d > K:
        raise ValueError(f"biou_d = {d} px needs 0 <= biou_d^2 <= K = {K}")
    out = _out_counts(out, 2 * (K + 2) + 2, p.device)
    ign = _ignore(ignore_index)
    eP, eG = edges(p, c, ignore_index), edges(t, c, ignore_index)
    dP, dG = sqdist(eP), sqdist(eG)
    lib.boundary_counts(p.data_ptr(), t.data_ptr(), eP.data_ptr(), eG.data_ptr(), dP.data_ptr(), dG.data_ptr(), N, H,
                        W, int(c), ign, K, d * d, out.data_ptr(), _stream(p))
    return out


def metrics_from_counts(counts, K, tolerance=2.0):
    """host, float64: the five ``KEYS`` from a ``counts`` array (tensor, array or list) taken with this K.

    Precision / recall: the share of prediction / target edge pixels whose squared distance to the other
    side's edge is at most ``tolerance``^2; a side without edge pixels scores 1.0 when the other has none
    either and 0.0 otherwise.  F1 = 2 P R / (P + R), 0 when P + R == 0.  Boundary IoU =
    intersection / union, 1.0 when the union is empty.  HD95: the two histograms pooled, sqrt of the
    smallest bin whose cumulative count reaches 95 % of all edge pixels; ``math.inf`` when that is the
    overflow bin, 0.0 without any edge pixel."""
    K = int(K)
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    if len(c) != 2 * (K + 2) + 2:
        raise ValueError(f"counts has {len(c)} entries, K = {K} needs {2 * (K + 2) + 2}")
    t2 = float(tolerance) ** 2
    if tolerance < 0 or t2 > K:
        raise ValueError(f"tolerance^2 = {t2} must lie in 0 .. K = {K}")
    hp, hg = c[:K + 2], c[K + 2:2 * K + 4]
    inter, union = c[2 * K + 4], c[2 * K + 5]
    n_p, n_g = sum(hp), sum(hg)
    last = min(int(math.floor(t2)), K)  # bins 0 .. last are within the tolerance

    def share(h, n, n_other):
        if n == 0:
            return 1.0 if n_other == 0 else 0.0
        return float(sum(h[:last + 1])) / float(n)

    prec, rec = share(hp, n_p, n_g), share(hg, n_g, n_p)
    f1 = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    biou = float(inter) / float(union) if union > 0 else 1.0
    total, hd95 = n_p + n_g, 0.0
    if total > 0:
        cum = 0
        for b in range(K + 2):
            cum += hp[b] + hg[b]
            if 100 * cum >= 95 * total:  # integers: no rounding at the boundary
                hd95 = math.inf if b == K + 1 else math.sqrt(b)
                break
    return {"Boundary Precision": prec, "Boundary Recall": rec, "Boundary F1": f1, "Boundary IoU": biou,
            "HD95": hd95}


class Accumulator(ClassCounts):
    """the boundary counts of an evaluation loop (``ClassCounts``).

    ``options`` is the entry points' ``boundary`` dict: ``{"tolerance": px (default 2.0), "biou_d": px or
    None / 0 (2 % of the diagonal), "K": squared distance (default 4096)}``.  A class counts in the mean when it
    has a target edge pixel in the split."""

    FAMILY, OPTIONS, KEYS = "boundary", ("tolerance", "biou_d", "K"), KEYS

    def __init__(self, options, classes=(1,), ignore_index=None):
        super().__init__(options, classes, ignore_index)
        self.tolerance = float(options.get("tolerance", 2.0))
        self.biou_d = options.get("biou_d") or None
        self.K = int(options.get("K", 4096))
        if self.tolerance < 0 or self.tolerance ** 2 > self.K:
            raise ValueError(f"tolerance^2 = {self.tolerance ** 2} must lie in 0 .. K = {self.K}")

    @property
    def N(self):
        return 2 * (self.K + 2) + 2

    def count(self, pred, tgt):
        for c, out in zip(self.classes, self.out):
            counts(pred, tgt, c, self.K, self.biou_d, self.ignore_index, out)

    def has_target(self, row):
        return sum(row[self.K + 2:2 * self.K + 4]) > 0

    def read(self, row):
        return metrics_from_counts(row, self.K, self.tolerance)
