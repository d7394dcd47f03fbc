"""The optional metric families of an evaluation loop as one object: boundary, skeleton (clDice), curve and objects.

``MetricSet`` is built from the four option values of the entry points (None = off) and is all a loop knows of
them: ``add`` per batch, ``metrics`` once after the loop.
"""
from __future__ import annotations

from .boundary import Accumulator as Boundary
from .classmap import labels_from_logits
from .curve import Accumulator as Curve
from .objects import Accumulator as Objects
from .skeleton import Accumulator as Skeleton


class MetricSet:
    """``boundary``, ``skeleton``, ``objects``: the options dict of the family's ``Accumulator`` or None; ``curve``:
    the same, or a ``curve.Accumulator`` that is taken as it is, so the caller can read its ``table()`` after the
    loop.  ``classes`` and ``ignore_index`` go to the per-class families; the curve takes ``ignore_index``."""

    def __init__(self, boundary=None, skeleton=None, curve=None, objects=None, classes=(1,), ignore_index=None):
        if curve is not None and not isinstance(curve, Curve):
            curve = Curve(curve, ignore_index)
        self.curve = curve
        # the families in the order of their keys; a new ``ClassCounts`` family is one more pair
        families = ((Boundary, boundary), (Skeleton, skeleton), (None, curve), (Objects, objects))
        self.accs = [options if family is None else family(options, classes, ignore_index)
                     for family, options in families if options is not None]

    @property
    def keys(self):
        """the key tuples of the families that are on, in the order of ``metrics``"""
        return tuple(a.keys for a in self.accs)

    def add(self, logits, targets):
        """a batch: one class map of the logits for the per-class families that are on, the raw logits for the
        curve; nothing is launched for a family that is off"""
        counted = [a for a in self.accs if a is not self.curve]
        if counted:
            pred = labels_from_logits(logits)
            for a in counted:
                a.add(pred, targets)
        if self.curve is not None:
            self.curve.add(logits, targets)

    def metrics(self):
        """one dict of every family's keys (one host read each)"""
        out = {}
        for a in self.accs:
            out.update(a.metrics())
        return out
