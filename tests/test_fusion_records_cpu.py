"""The op layer's fusion handshake on plain Nodes over CPU tensors (no launch, no library): the
Producer / Partials records and the test "x is a ReLU output and this op is its only consumer", as the
three fused backwards apply it.  The sites differ on purpose-or-not in ways this table pins, so that a
change to any of them is deliberate:

* the conv data gradient (_dgrad_fused) takes the shared test alone: conv + ReLU and BN-ReLU
  producers, and it does not ask that the record still describes x.data (its kernel reads the record's
  tensors);
* the upsample and head backwards take a conv + ReLU producer only and do ask that (their kernels mask
  with x.data itself); the upsample adds its own switch FUSE_UP, the head adds x.need_grad.
"""
import itertools
from types import SimpleNamespace

import pytest
import torch

from unetseg_hip import lib as libmod
from unetseg_hip import ops
from unetseg_hip.lib import DT_BF16, DT_F32


def _node(kind, uses=1, grad=False, replaced=False, need_grad=True):
    data = torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16)
    x = ops.Node(data, need_grad=need_grad)
    st = ops.BNState()
    if kind == ops.POST_RELU:
        x.fuse = ops.Producer(ops.POST_RELU, data)
    elif kind == ops.POST_BN_RELU:
        x.fuse = ops.Producer(ops.POST_BN_RELU, torch.zeros_like(data), st)  # act: the BN input
    else:
        x.fuse = ops.Producer(ops.POST_RES_BN_RELU, torch.zeros_like(data), st, torch.zeros(4, dtype=torch.uint8))
    x.uses = uses
    if grad:
        x.grad = torch.zeros_like(data)
    if replaced:  # data replaced after the record was made
        x.data = data.clone()
    return x


def _sites(ctx, x):
    return (ops._sole_relu_consumer(ctx, x), ops._upsample_may_fuse(ctx, x, x.data),
            ops._head_may_fuse(ctx, x, x.data))


CASES = list(itertools.product((1, 2, 3), (1, 2), (False, True), (False, True), (DT_BF16, DT_F32)))


@pytest.mark.parametrize("kind,uses,grad,replaced,dt", CASES)
def test_sole_consumer_truth_table(kind, uses, grad, replaced, dt):
    loaded = libmod._lib
    ctx = SimpleNamespace(dt=dt)
    sole = uses == 1 and not grad and dt == DT_BF16
    dgrad = sole and kind in (1, 2)  # replaced or not
    rides = sole and kind == 1 and not replaced
    assert _sites(ctx, _node(kind, uses, grad, replaced)) == (dgrad, rides, rides)
    assert libmod._lib is loaded  # nothing here loads the library


def test_site_specific_conditions(monkeypatch):
    ctx = SimpleNamespace(dt=DT_BF16)
    assert _sites(ctx, _node(1)) == (True, True, True)
    # a node nobody wants a gradient for: only the head backward asks
    assert _sites(ctx, _node(1, need_grad=False)) == (True, True, False)
    # a node without a record
    x = _node(1)
    x.fuse = None
    assert _sites(ctx, x) == (False, False, False)
    monkeypatch.setattr(ops, "FUSE_UP", False)  # the upsample fusion's own switch
    assert _sites(ctx, _node(1)) == (True, False, True)
    monkeypatch.setattr(ops, "FUSE_UP", True)
    monkeypatch.setattr(ops, "FUSE", False)  # the common switch
    assert _sites(ctx, _node(1)) == (False, False, False)
    assert _sites(ctx, _node(2)) == (False, False, False)


def test_records():
    # the kinds are the C ABI's post codes (unetseg_conv2d_dgrad_post takes them verbatim)
    assert (ops.POST_RELU, ops.POST_BN_RELU, ops.POST_RES_BN_RELU, ops.POST_RELU_BITS) == (1, 2, 3, 4)
    assert isinstance(ops.RELU_BITS, bool)  # the switch keeps its name
    a, bits = torch.zeros(2), torch.zeros(2, dtype=torch.uint8)
    p = ops.Producer(ops.POST_RELU, a, mbits=bits)
    assert (p.kind, p.act, p.mbits, p.st, p.act2, p.st2) == (1, a, bits, None, None, None)
    st, st2 = ops.BNState(), ops.BNState()
    p = ops.Producer(ops.POST_RES_BN_RELU, a, st, bits, a, st2)
    assert (p.st, p.mbits, p.act2, p.st2) == (st, bits, a, st2)
    f = ops.Partials(a, 7)
    assert (f.part, f.rows, f.nq) == (a, 7, 2)
    assert ops.Partials(a, 7, 3).nq == 3
    # slotted: no per-instance dict, and nothing beyond the tensors listed (no back-reference to a consumer)
    for o in (p, f, ops.Node(a)):
        assert not hasattr(o, "__dict__")
    assert ops.Producer.__slots__ == ("kind", "act", "st", "mbits", "act2", "st2")
    assert ops.Partials.__slots__ == ("part", "rows", "nq")
    assert "mbits" not in ops.Node.__slots__  # the packed mask lives in the producer record
    n = ops.Node(a)
    assert n.fuse is None and n.fused is None
