"""Object-level agreement of class maps on the HIP path (csrc/objects.hip): how many objects were found, how
many predicted objects are spurious, how often one object is cut in two or two are fused.

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU.  Both maps are labelled with ``ccl.label``'s kernels
at ``connectivity``; for a class ``c`` in 1 .. 255 an *object* is a component of class ``c``.  A predicted object p
and a target object g *overlap* when some pixel has ``pred == c``, ``target == c`` and lies in both; ``inter`` is
the number of such pixels and ``union = area_p + area_g - inter``.  ``counts`` reduces a prediction / target pair
to twenty integers, ``pairs`` lists the overlapping pairs, and ``metrics_from_counts`` reads Panoptic Quality
(Kirillov et al., CVPR 2019: a pair with IoU > 0.5 is a match, and such matches are unique, so no assignment step
exists), object precision / recall / F1, the F1 averaged over the IoU thresholds 0.5 .. 0.95, and the split and
merge rates on the host.  All of it is integer and bitwise reproducible; ``counts`` runs on the current stream and
never waits on the host, its number of launches depends on the shape only, and it accumulates, so a split costs
one host read.
"""
from __future__ import annotations

import ctypes

import torch

from . import ccl
from .classmap import ClassCounts, _check_class, _out_counts, _pair, _stream
from .lib import lib

KEYS = ("PQ", "SQ", "Object F1", "Object Precision", "Object Recall", "Object F1@[.5:.95]", "Detection Recall",
        "False Object Rate", "Split Rate", "Merge Rate")
#: entries of a ``counts`` array
N_COUNTS = 20


def tile():
    """(tw, th): a block of the pair kernel gathers the runs of a tile of this size before it touches the table"""
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    lib.objects_tile(ctypes.addressof(tw), ctypes.addressof(th))
    return tw.value, th.value


def workspace_bytes(N, H, W):
    """bytes of the workspace of an [N,H,W] pair of maps (roots, stats, pair table, degree planes)"""
    return lib.objects_workspace(int(N), int(H), int(W))


def _connectivity(connectivity):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    return int(connectivity)


class _Labelled:
    """a pair of maps [N,H,W] (ignored pixels already 0 in both) with its workspace, labelled and measured"""

    def __init__(self, pm, tm, connectivity):
        self.p, self.t = pm, tm
        self.shape = N, H, W = pm.shape
        self.size = workspace_bytes(N, H, W)
        if self.size == 0:
            raise ValueError(f"objects: shape {tuple(pm.shape)} is too large")
        self.ws = torch.empty(self.size, dtype=torch.uint8, device=pm.device)
        lib.objects_label(pm.data_ptr(), tm.data_ptr(), N, H, W, connectivity, self.ws.data_ptr(), self.size,
                          _stream(pm))

    def pairs(self, c, aggregate=True):
        """fill the pair table of class ``c``"""
        N, H, W = self.shape
        lib.objects_pairs(self.p.data_ptr(), self.t.data_ptr(), N, H, W, c, int(bool(aggregate)), self.ws.data_ptr(),
                          self.size, _stream(self.p))

    def match(self, c, out):
        """out += the counts of class ``c`` from its pair table"""
        N, H, W = self.shape
        lib.objects_match(self.p.data_ptr(), self.t.data_ptr(), N, H, W, c, out.data_ptr(), self.ws.data_ptr(),
                          self.size, _stream(self.p))

    def table(self):
        """(keys int64 [N,cap] with -1 = empty, inter int32 [N,cap], area planes int32 [2,N,H*W]) as views"""
        N, H, W = self.shape
        at = (ctypes.c_int64 * 6)()
        lib.objects_layout(N, H, W, ctypes.addressof(at))
        _, stats, keys, vals, _, cap = (int(v) for v in at)
        T = N * H * W
        k = self.ws[keys:keys + N * cap * 8].view(torch.int64).view(N, cap)
        v = self.ws[vals:vals + N * cap * 4].view(torch.int32).view(N, cap)
        st = self.ws[stats:stats + 8 * T * 4].view(torch.int32).view(2, 4, N, H * W)
        return k, v, st[:, 0]


def counts(pred, target, c=1, connectivity=8, ignore_index=None, out=None):
    """device int64 [20] (+)= the object counts of class ``c`` of the int32 maps ``pred`` and ``target`` (same
    shape), whose pixels with target ``ignore_index`` are set to 0 in both first:

    * ``[0]``, ``[1]`` target objects, predicted objects;
    * ``[2]``, ``[3]`` target objects that overlap a predicted object, predicted objects that overlap a target one;
    * ``[4]`` target objects overlapped by two or more predicted objects (splits), ``[5]`` predicted objects that
      overlap two or more target objects (merges);
    * ``[6 + j]``, j = 0 .. 9: pairs with IoU > 0.5 + j / 20, decided as ``20 inter > (10 + j) union`` in integers;
    * ``[16]`` the sum over the pairs with IoU > 0.5 of ``floor(inter * 2**32 / union)``;
    * ``[17]`` distinct overlapping pairs, ``[18]`` pair-table insertions that found no slot (0 unless there is a
      bug; ``metrics_from_counts`` raises on it), ``[19]`` the number of images.

    ``out`` is added to and returned when given.  An empty batch adds nothing."""
    c = _check_class(c, ignore_index)
    connectivity = _connectivity(connectivity)
    _, _, pm, tm = _pair(pred, target, ignore_index)
    out = _out_counts(out, N_COUNTS, pm.device)
    if pm.numel() == 0:
        return out
    lab = _Labelled(pm, tm, connectivity)
    lab.pairs(c)
    lab.match(c, out)
    return out


def pairs(pred, target, c=1, connectivity=8, ignore_index=None):
    """int32 [K,6] on the device: (image, root_pred, root_target, inter, area_pred, area_target) of every
    overlapping pair of objects of class ``c``, ordered by (image, root_target, root_pred); a root is the smallest
    raster index ``y * W + x`` of its object (``ccl.label``).  The compaction is torch (it sizes its result on the
    host)."""
    c = _check_class(c, ignore_index)
    connectivity = _connectivity(connectivity)
    _, _, pm, tm = _pair(pred, target, ignore_index)
    if pm.numel() == 0:
        return torch.zeros(0, 6, dtype=torch.int32, device=pm.device)
    lab = _Labelled(pm, tm, connectivity)
    lab.pairs(c)
    keys, inter, area = lab.table()
    image, slot = torch.nonzero(keys != -1, as_tuple=True)
    key = keys[image, slot]
    rp, rt = key >> 32, key & 0xFFFFFFFF
    rows = torch.stack([image, rp, rt, inter[image, slot].long(), area[0][image, rp].long(),
                        area[1][image, rt].long()], 1)
    for col in (1, 2, 0):  # stable sorts, the least significant column first
        rows = rows[torch.sort(rows[:, col], stable=True).indices]
    return rows.to(torch.int32)


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def metrics_from_counts(counts):
    """host, float64: the ten ``KEYS`` from a ``counts`` array (tensor, array or list).

    With tp = c6 (pairs with IoU > 0.5), fp = n_pred - tp, fn = n_gt - tp and S = c16 / 2**32 (the sum of the
    matched IoUs): Object Precision = tp / n_pred, Object Recall = tp / n_gt, Object F1 = 2 tp / (n_pred + n_gt),
    SQ = S / tp, PQ = S / (tp + (fp + fn) / 2); Object F1@[.5:.95] is the mean of the F1 at the ten thresholds;
    Detection Recall = c2 / n_gt (any overlap), False Object Rate = 1 - c3 / n_pred, Split Rate = c4 / n_gt, Merge
    Rate = c5 / n_pred.  Every ratio with a zero denominator is 0.0 (the False Object Rate without a predicted
    object too).  The counts are pooled over the split, like every other metric here.  Raises RuntimeError when a
    pair-table insertion was dropped: the counts are then wrong, not approximate."""
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    if len(c) != N_COUNTS:
        raise ValueError(f"counts has {len(c)} entries, not {N_COUNTS}")
    if c[18] > 0:
        raise RuntimeError(f"{c[18]} insertions found no slot in the pair table of {c[19]} images: the capacity "
                           "bound of csrc/objects.hip does not hold, which is a bug")
    n_gt, n_pred, tp = c[0], c[1], c[6]
    S = (c[16] & (2**64 - 1)) / 2**32
    fp, fn = n_pred - tp, n_gt - tp
    return {"PQ": _ratio(S, tp + (fp + fn) / 2), "SQ": _ratio(S, tp), "Object F1": _ratio(2 * tp, n_pred + n_gt),
            "Object Precision": _ratio(tp, n_pred), "Object Recall": _ratio(tp, n_gt),
            "Object F1@[.5:.95]": sum(_ratio(2 * c[6 + j], n_pred + n_gt) for j in range(10)) / 10,
            "Detection Recall": _ratio(c[2], n_gt),
            "False Object Rate": 1.0 - _ratio(c[3], n_pred) if n_pred > 0 else 0.0,
            "Split Rate": _ratio(c[4], n_gt), "Merge Rate": _ratio(c[5], n_pred)}


class Accumulator(ClassCounts):
    """the object counts of an evaluation loop (``ClassCounts``).

    ``options`` is the entry points' ``objects`` dict: ``{"connectivity": 4 or 8 (default 8), "min_area": int
    (default 0)}``.  ``min_area`` > 1 passes the prediction through ``ccl.clean(pred, min_area, 0, connectivity)``
    first, the cleanup of ``predict.py --min-area``, so the numbers are those of the map that would be shipped.  The
    two labellings and stats of a batch are done once and shared by the classes.  A class counts in the mean when
    it has a target object in the split."""

    FAMILY, OPTIONS, N, KEYS = "objects", ("connectivity", "min_area"), N_COUNTS, KEYS

    def __init__(self, options, classes=(1,), ignore_index=None):
        super().__init__(options, [_check_class(c, ignore_index) for c in classes], ignore_index)
        self.connectivity = _connectivity(options.get("connectivity", 8))
        self.min_area = int(options.get("min_area", 0) or 0)
        if self.min_area < 0:
            raise ValueError(f"min_area must not be negative, got {self.min_area}")

    def count(self, pred, tgt):
        if self.min_area > 1:
            pred = ccl.clean(pred, self.min_area, 0, self.connectivity)
        _, _, pm, tm = _pair(pred, tgt, self.ignore_index)
        if pm.numel() == 0:
            return
        lab = _Labelled(pm, tm, self.connectivity)
        for c, out in zip(self.classes, self.out):
            lab.pairs(c)
            lab.match(c, out)

    def guard(self, row):  # a dropped insertion is a bug whatever the class
        if row[18] > 0:
            metrics_from_counts(row)

    def has_target(self, row):
        return row[0] > 0

    read = staticmethod(metrics_from_counts)
