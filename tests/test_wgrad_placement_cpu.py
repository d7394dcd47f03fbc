"""Where the op layer runs a conv's weight gradient (ops._wgrad_place), on a SimpleNamespace context: no GPU,
no launch, no library.  The rule is written out here independently of the code:

* DEFERRED (held until the flush marker) iff WG_DEFER_HW is non-zero, the backward overlaps (ctx.side), the
  forward recorded a marker that has not run yet, the output has >= WG_DEFER_HW pixels per image, the filter is
  larger than 1x1 and the conv reads a virtual concat;
* else SERIAL (compute stream, after the data gradient) iff the layer recorded at forward time is in
  WG_SERIAL_LAYERS;
* else SIDE.

Also here: the four retired scheduling knobs are gone and their environment variables change nothing, and
PackedConv's padded width.
"""
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from unetseg_hip import lib as libmod
from unetseg_hip import ops
from unetseg_hip.lib import DT_BF16, DT_F32

PKG = os.path.dirname(os.path.dirname(os.path.abspath(ops.__file__)))
RETIRED = {"WG_AFTER_DGRAD": "1", "WG_SERIAL_HW": "1024", "WG_DEFER_CAT": "0", "SIDE_PRIORITY": "-1"}

#: (Pq, Qq): 1023 and 1024 pixels, the two sides of the default WG_DEFER_HW at the smallest sizes that differ
HW = ((33, 31), (32, 32))
CASES = list(itertools.product((None, object()), (False, True), (False, True), HW, ((1, 1), (3, 3)), (False, True),
                               (None, "stem", "layer1", "decoder")))


def _ctx(side=None, has_marker=False, flushed=False):
    return SimpleNamespace(side=side, has_marker=has_marker, flushed=flushed)


def _expected(ctx, layer, hw, rs, concat, defer_hw=1024, serial_layers=("stem",)):
    if (defer_hw != 0 and ctx.side is not None and ctx.has_marker and not ctx.flushed and hw >= defer_hw and
            rs > 1 and concat):
        return ops.WG_DEFERRED
    return ops.WG_SERIAL if layer in serial_layers else ops.WG_SIDE


def test_defaults():
    assert ops.WG_DEFER_HW == 1024 and ops.WG_SERIAL_LAYERS == frozenset({"stem"})
    assert len({ops.WG_SIDE, ops.WG_SERIAL, ops.WG_DEFERRED}) == 3


@pytest.mark.parametrize("side,has_marker,flushed,pq,rs,concat,layer", CASES)
def test_placement_truth_table(side, has_marker, flushed, pq, rs, concat, layer):
    loaded = libmod._lib
    ctx = _ctx(side, has_marker, flushed)
    (Pq, Qq), (R, S) = pq, rs
    assert Pq * Qq in (1023, 1024)
    want = _expected(ctx, layer, Pq * Qq, R * S, concat)
    assert ops._wgrad_place(ctx, layer, Pq, Qq, R, S, concat) == want
    assert libmod._lib is loaded  # nothing here loads the library


def test_placement_follows_the_knobs(monkeypatch):
    held = _ctx(object(), True, False)
    assert ops._wgrad_place(held, "decoder", 32, 32, 3, 3, True) == ops.WG_DEFERRED
    assert ops._wgrad_place(held, "stem", 32, 32, 3, 3, True) == ops.WG_DEFERRED  # deferral is decided first
    monkeypatch.setattr(ops, "WG_DEFER_HW", 0)
    for side, has_marker, flushed, (Pq, Qq), (R, S), concat, layer in CASES:
        ctx = _ctx(side, has_marker, flushed)
        got = ops._wgrad_place(ctx, layer, Pq, Qq, R, S, concat)
        assert got != ops.WG_DEFERRED
        assert got == _expected(ctx, layer, Pq * Qq, R * S, concat, defer_hw=0)
    monkeypatch.setattr(ops, "WG_DEFER_HW", 1024)
    monkeypatch.setattr(ops, "WG_SERIAL_LAYERS", frozenset())
    for side, has_marker, flushed, (Pq, Qq), (R, S), concat, layer in CASES:
        ctx = _ctx(side, has_marker, flushed)
        got = ops._wgrad_place(ctx, layer, Pq, Qq, R, S, concat)
        assert got != ops.WG_SERIAL
        assert got == _expected(ctx, layer, Pq * Qq, R * S, concat, serial_layers=())
    monkeypatch.setattr(ops, "WG_SERIAL_LAYERS", frozenset({"stem", "layer1"}))
    for layer, want in ((None, ops.WG_SIDE), ("stem", ops.WG_SERIAL), ("layer1", ops.WG_SERIAL),
                        ("decoder", ops.WG_SIDE)):
        assert ops._wgrad_place(_ctx(object(), True, True), layer, 32, 32, 3, 3, True) == want
        assert ops._wgrad_place(_ctx(), layer, 33, 31, 1, 1, False) == want


def test_retired_knobs_are_gone():
    for name in RETIRED:
        assert not hasattr(ops, name)
    # their environment variables change nothing: a fresh interpreter that imports ops with all four set keeps
    # the defaults, has none of the names and has not loaded the library
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from unetseg_hip import lib, ops\n"
            "assert lib._lib is None\n"
            "assert not [n for n in %r if hasattr(ops, n)]\n"
            "s = lambda **k: __import__('types').SimpleNamespace(**k)\n"
            "held, free = s(side=1, has_marker=True, flushed=False), s(side=1, has_marker=False, flushed=False)\n"
            "print(ops.WG_DEFER_HW, sorted(ops.WG_SERIAL_LAYERS), ops.WG_FLUSH, ops.OVERLAP,\n"
            "      ops._wgrad_place(held, 'decoder', 32, 32, 3, 3, True), ops._wgrad_place(held, 'decoder', 32, 32, 3, 3, False),\n"
            "      ops._wgrad_place(free, 'layer1', 64, 64, 3, 3, False), ops._wgrad_place(free, 'stem', 64, 64, 7, 7, False))\n"
            % (PKG, sorted(RETIRED)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("UNETSEG_")}
    env.update({"UNETSEG_" + k: v for k, v in RETIRED.items()})
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # the defaults: only a virtual concat is held back, large 3x3 maps stay on the side stream, the stem is serial
    assert r.stdout.split() == ["1024", "['stem']", "layer3", "True", "deferred", "side", "side", "serial"]


def _packed(K, R=1, stride=1):
    conv = torch.nn.Conv2d(16, K, R, stride=stride, padding=R // 2, bias=False)
    conv.stride, conv.padding = stride, R // 2  # the op layer's containers hold plain ints
    return ops.PackedConv(conv)


@pytest.mark.parametrize("K,want", [(8, 64), (32, 64), (64, 0), (72, 128)])
def test_padded_width(monkeypatch, K, want):
    loaded = libmod._lib
    pc = _packed(K)
    assert pc.kpad(DT_BF16) == want
    assert bool(pc.kpad(DT_BF16)) == bool(pc.padk(DT_BF16))
    # never padded: fp32, a 3x3 filter, a strided 1x1, or with the switch off
    assert pc.kpad(DT_F32) == 0
    assert _packed(K, R=3).kpad(DT_BF16) == 0
    assert _packed(K, stride=2).kpad(DT_BF16) == 0
    monkeypatch.setattr(ops, "PAD_K", False)
    assert pc.kpad(DT_BF16) == 0
    assert libmod._lib is loaded
