"""What the class-map metric families share: the argument checks of an int32 class map, the decision rule that
turns logits into one, and ``ClassCounts``, the per-class count accumulator of an evaluation loop.

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU.  ``boundary``, ``skeleton``, ``objects``, ``curve`` and
``ccl`` take their helpers from here and from nowhere else; a new per-class family subclasses ``ClassCounts``
("Adding a metric family").
"""
from __future__ import annotations

import torch

#: the largest class value ``skeleton.thin`` and the object kernels keep
MAX_CLASS = 255


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _map(t, what="cls", dtypes=(torch.int32,)):
    """the map as a contiguous [N,H,W] view"""
    if not torch.is_tensor(t) or t.dtype not in dtypes or not t.is_cuda or t.dim() not in (2, 3):
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what} must be a {names} [H,W] or [N,H,W] tensor on the GPU, got "
                         f"{t.dtype if torch.is_tensor(t) else type(t)} "
                         f"{tuple(t.shape) if torch.is_tensor(t) else ''}")
    t = t.contiguous()
    return t.unsqueeze(0) if t.dim() == 2 else t


def _ignore(ignore_index):
    if ignore_index is None:
        return -1
    if int(ignore_index) == -1:
        raise ValueError("ignore_index -1 stands for None in the kernels; use another value")
    return int(ignore_index)


def _out_counts(out, n, device):
    """the array a ``counts`` adds to: ``out`` checked, or zeros when it is None"""
    if out is None:
        return torch.zeros(n, dtype=torch.int64, device=device)
    if (not torch.is_tensor(out) or out.dtype != torch.int64 or out.device != device or out.dim() != 1
            or out.numel() != n or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 [{n}] tensor on {device}")
    return out


def _int_target(target, ignore_index):
    """an evaluation loop's target [B,H,W] or [B,1,H,W] as int32 [B,H,W]; a float target is read as
    ``losses.binary_confusion`` reads it: class 1 where it equals 1, ``ignore_index`` kept"""
    tgt = target.detach()
    if tgt.is_floating_point():
        lab = (tgt == 1).to(torch.int32)
        if ignore_index is not None:
            lab = torch.where(tgt == ignore_index, torch.full_like(lab, int(ignore_index)), lab)
        tgt = lab
    if tgt.dim() == 4 and tgt.shape[1] == 1:
        tgt = tgt[:, 0]
    return tgt.to(torch.int32)


def _class_mean(rows, several, has_target, read, keys):
    """an accumulator's metrics from its per-class count rows: ``read(row)`` of the one class, or with
    ``several`` classes the mean per key over the rows that ``has_target``; 0.0 when none is left"""
    if several:
        rows = [r for r in rows if has_target(r)]
    per = [read(r) for r in rows]
    if not per:
        return dict.fromkeys(keys, 0.0)
    if len(per) == 1:
        return per[0]
    return {k: sum(m[k] for m in per) / len(per) for k in keys}


def _check_class(c, ignore_index):
    c = int(c)
    if not 1 <= c <= MAX_CLASS:
        raise ValueError(f"class must lie in 1 .. {MAX_CLASS}, got {c}")
    if ignore_index is not None and int(ignore_index) == c:
        raise ValueError(f"ignore_index is the counted class {c}")
    return c


def _pair(pred, target, ignore_index):
    """pred and target as [N,H,W], with the pixels whose target is ``ignore_index`` set to 0 in both"""
    p, t = _map(pred, "pred"), _map(target, "target")
    if p.shape != t.shape or p.device != t.device:
        raise ValueError(f"pred {tuple(p.shape)} on {p.device} and target {tuple(t.shape)} on {t.device} differ")
    if ignore_index is None:
        return p, t, p, t
    valid = t != int(ignore_index)
    zero = torch.zeros_like(t)
    return p, t, torch.where(valid, p, zero), torch.where(valid, t, zero)


def labels_from_logits(outputs):
    """int32 [B,H,W] class map of logits [B,C,H,W]: C >= 2 the argmax with a tie going to the lower class,
    C == 1 ``logit > 0``: the rule of ``losses.binary_confusion`` (argmax with the tie to class 0, and
    sigmoid > 0.5, which a zero logit does not pass)"""
    if not torch.is_tensor(outputs) or outputs.dim() != 4:
        raise ValueError("outputs must be logits [B,C,H,W]")
    out = outputs.detach().float()
    if out.shape[1] == 1:
        return (out[:, 0] > 0).to(torch.int32)
    best, lab = out[:, 0], torch.zeros(out[:, 0].shape, dtype=torch.int32, device=out.device)
    for k in range(1, out.shape[1]):  # strictly greater: a tie keeps the lower class
        take = out[:, k] > best
        best = torch.where(take, out[:, k], best)
        lab = torch.where(take, torch.full_like(lab, k), lab)
    return lab


class ClassCounts:
    """the counts of one metric family over an evaluation loop: one device row of ``N`` int64 per class, added to
    per batch, read once.  ``out`` is that [len(classes), N] tensor (None before the first batch): a data-parallel
    caller can all-reduce it before ``metrics``.

    A family sets ``FAMILY`` (its name in messages), ``OPTIONS`` (the keys its options dict may hold), ``N`` and
    ``KEYS``, parses its options after ``super().__init__``, and gives ``count(pred, tgt)`` (add a batch of int32
    maps to ``out``), ``has_target(row)`` and ``read(row)``; ``guard(row)`` may raise on a row that must not be
    read."""

    FAMILY = ""
    OPTIONS = ()
    N = 0
    KEYS = ()

    def __init__(self, options, classes=(1,), ignore_index=None):
        unknown = set(options) - set(self.OPTIONS)
        if unknown:
            raise ValueError(f"unknown {self.FAMILY} options {sorted(unknown)}")
        self.classes = tuple(classes)
        self.ignore_index = ignore_index
        self.out = None

    @property
    def keys(self):
        return self.KEYS

    def add(self, pred, target):
        """pred int32 [B,H,W] (``labels_from_logits``); target [B,H,W] or [B,1,H,W] on the same device, integer,
        or float read as ``losses.binary_confusion`` reads it: class 1 where it equals 1, ``ignore_index`` kept"""
        tgt = _int_target(target, self.ignore_index)
        if self.out is None:
            self.out = torch.zeros(len(self.classes), self.N, dtype=torch.int64, device=pred.device)
        self.count(pred, tgt)

    def guard(self, row):
        pass

    def metrics(self):
        """the family's keys after one host read; with several classes the mean over those that ``has_target`` in
        the split, 0.0 without one"""
        rows = self.out.tolist() if self.out is not None else [[0] * self.N for _ in self.classes]
        for r in rows:  # a spoilt row spoils the split, whatever its class
            self.guard(r)
        return _class_mean(rows, len(self.classes) > 1, self.has_target, self.read, self.KEYS)
