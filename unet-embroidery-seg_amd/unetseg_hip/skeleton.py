"""Hard skeleton of class maps and the clDice metric on the HIP path (csrc/skeleton.hip).

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU; class 0 is background and the classes are
1 .. 255 (any other value counts as background).  ``thin`` is Guo & Hall's two-subiteration parallel
thinning (CACM 32(3), 1989, algorithm A1; the rule stands in include/unetseg_hip.h), per class: a neighbour
counts only when it has the pixel's own class, so one run thins every class of a map as if it were alone.
``counts`` reduces a prediction / target pair to the six integers the clDice metric (Shit et al., CVPR
2021, section 3: topology precision and sensitivity on *hard* skeletons) is read from, and
``metrics_from_counts`` reads it on the host.  All of it is integer and bitwise reproducible; ``thin`` and
``counts`` run on the current stream and never wait on the host, the number of launches depends on the
shape and ``max_passes`` only, and ``counts`` accumulates, so a split costs one host read.
"""
from __future__ import annotations

import ctypes

import torch

from .classmap import MAX_CLASS  # noqa: F401  (the largest class value ``thin`` keeps)
from .classmap import ClassCounts, _check_class, _ignore, _map, _out_counts, _pair, _stream
from .lib import lib

KEYS = ("clDice", "Skeleton Precision", "Skeleton Recall")


def tile():
    """(tw, th, K): thinning works on tiles of tw x th pixels, so its seams lie at their multiples, and one
    launch runs K passes"""
    tw, th, k = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib.skel_tile(ctypes.addressof(tw), ctypes.addressof(th), ctypes.addressof(k))
    return tw.value, th.value, k.value


def default_max_passes(H, W):
    """``min(H, W) // 2 + 8``: a pass peels one pixel off every side of a region, so a region as wide as the
    image is gone after about ``min(H, W) / 2``; the passes measured on full maps, discs and smoothed blobs
    stayed at least 4 below this cap (tests/test_skeleton_cpu.py).  No bound is proved: an image that is still
    losing pixels at the cap is reported, never passed over"""
    return min(int(H), int(W)) // 2 + 8


def _passes(max_passes, H, W):
    p = default_max_passes(H, W) if max_passes is None else int(max_passes)
    if p < 0:
        raise ValueError(f"max_passes must not be negative, got {p}")
    return p


def thin(cls, max_passes=None, return_unconverged=False):
    """int32, the shape of ``cls``: ``cls`` with the pixels that thinning deletes set to 0.

    A pass is the two subiterations; an image is done after the first pass that deletes nothing or after
    ``max_passes`` passes (None: ``default_max_passes(H, W)``; 0 runs no pass).  With ``return_unconverged``
    also an int32 [N] device tensor: 1 where the image's last pass still deleted a pixel."""
    m = _map(cls)
    N, H, W = m.shape
    p = _passes(max_passes, H, W)
    out = torch.empty_like(m)
    unc = torch.empty(N, dtype=torch.int32, device=m.device) if return_unconverged else None
    size = lib.skel_workspace(N, H, W)
    if size == 0:
        raise ValueError(f"thin: shape {tuple(m.shape)} is too large")
    ws = torch.empty(size, dtype=torch.uint8, device=m.device)
    lib.skel_thin(m.data_ptr(), N, H, W, p, out.data_ptr(), unc.data_ptr() if unc is not None else None,
                  ws.data_ptr(), size, _stream(m))
    out = out.view(cls.shape)
    return (out, unc) if return_unconverged else out


def _thin_pair(pm, tm, max_passes):
    """both maps thinned in one call on the stacked 2N images: (skel_pred, skel_target, unconv_pred, unconv_target)"""
    N = pm.shape[0]
    sk, unc = thin(torch.cat([pm, tm], 0), max_passes, return_unconverged=True)
    return sk[:N], sk[N:], unc[:N], unc[N:]


def _counts(p, t, thinned, c, ign, out):
    sp, st, up, ut = thinned
    N, H, W = p.shape
    lib.skel_counts(p.data_ptr(), t.data_ptr(), sp.data_ptr(), st.data_ptr(), up.data_ptr(), ut.data_ptr(), N, H, W, c,
                    ign, out.data_ptr(), _stream(p))
    return out


def counts(pred, target, c=1, ignore_index=None, max_passes=None, out=None):
    """device int64 [6] (+)= the skeleton counts of class ``c`` of the int32 maps ``pred`` and ``target`` (same
    shape), with S(.) the hard skeleton (``thin``) of a map whose ignored pixels were set to 0 first:

    * ``[0]`` #(S(pred) == c and target == c), ``[1]`` #(S(pred) == c);
    * ``[2]`` #(S(target) == c and pred == c), ``[3]`` #(S(target) == c);
    * ``[4]`` the number of images one of whose two thinnings had not converged after ``max_passes``;
    * ``[5]`` the number of images.

    Pixels whose target is ``ignore_index`` are outside the domain.  ``out`` is added to and returned when
    given."""
    c = _check_class(c, ignore_index)
    ign = _ignore(ignore_index)
    p, t, pm, tm = _pair(pred, target, ignore_index)
    out = _out_counts(out, 6, p.device)
    return _counts(pm, t, _thin_pair(pm, tm, max_passes), c, ign, out)


def metrics_from_counts(counts):
    """host, float64: the three ``KEYS`` from a ``counts`` array (tensor, array or list).

    Skeleton Precision (the paper's Tprec) = c0 / c1, the share of the prediction's skeleton that lies in the
    target; Skeleton Recall (Tsens) = c2 / c3, the share of the target's skeleton that lies in the prediction;
    a side with an empty skeleton scores 1.0 when the other is empty too and 0.0 otherwise.  clDice =
    2 Tprec Tsens / (Tprec + Tsens), 0 when the sum is 0.  The counts are pooled over the split, like every
    other metric here, not averaged per image.  Raises RuntimeError when an image had not converged: a
    metric on a half-thinned map is wrong, not approximate."""
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    if len(c) != 6:
        raise ValueError(f"counts has {len(c)} entries, not 6")
    c0, c1, c2, c3, c4, c5 = c
    if c4 > 0:
        raise RuntimeError(f"thinning had not converged on {c4} of {c5} images when the pass cap was reached; "
                           "raise the max_passes option (--skeleton-max-passes)")
    tprec = float(c0) / float(c1) if c1 > 0 else (1.0 if c3 == 0 else 0.0)
    tsens = float(c2) / float(c3) if c3 > 0 else (1.0 if c1 == 0 else 0.0)
    cl = 2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0 else 0.0
    return {"clDice": cl, "Skeleton Precision": tprec, "Skeleton Recall": tsens}


class Accumulator(ClassCounts):
    """the skeleton counts of an evaluation loop (``ClassCounts``).

    ``options`` is the entry points' ``skeleton`` dict: ``{"max_passes": int or None}`` (None:
    ``default_max_passes``).  The two thinnings of a batch are done once and shared by the classes.  A class counts
    in the mean when its target skeleton is non-empty in the split."""

    FAMILY, OPTIONS, N, KEYS = "skeleton", ("max_passes",), 6, KEYS

    def __init__(self, options, classes=(1,), ignore_index=None):
        super().__init__(options, [_check_class(c, ignore_index) for c in classes], ignore_index)
        self.max_passes = options.get("max_passes")
        if self.max_passes is not None and int(self.max_passes) < 0:
            raise ValueError(f"max_passes must not be negative, got {self.max_passes}")

    def count(self, pred, tgt):
        p, t, pm, tm = _pair(pred, tgt, self.ignore_index)
        thinned = _thin_pair(pm, tm, self.max_passes)
        for c, out in zip(self.classes, self.out):
            _counts(pm, t, thinned, c, _ignore(self.ignore_index), out)

    def guard(self, row):  # an unconverged image spoils every class's counts
        if row[4] > 0:
            metrics_from_counts(row)

    def has_target(self, row):
        return row[3] > 0

    read = staticmethod(metrics_from_counts)
