"""CPU: the float64 references of tests/nhwc_ref.py against the PyTorch operation or its autograd result, in
float64 (agreement to 1e-12 relative; indices and mask bytes exactly), and the contract helpers against
themselves (a 2-ulp perturbation and a touched guard byte must fail).  No GPU, no library."""
import pytest
import torch
import torch.nn.functional as F

import nhwc_ref as R

F64 = torch.float64
RESIZE_CASES = [(1, 1, 4, 3, True), (3, 1, 5, 1, True), (4, 5, 1, 1, True), (2, 3, 37, 64, False),
                (37, 64, 2, 3, False), (11, 11, 31, 31, True), (8, 10, 8, 10, False), (9, 11, 4, 5, False),
                (7, 7, 13, 20, True)]


def _close(a, b, what, tol=1e-12):
    a, b = a.to(F64), b.to(F64)
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: max|diff| {err:.3e} against max|ref| {scale:.3e}"


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("two", [False, True])
def test_batchnorm_residual_relu_and_gradients(two):
    """out = relu(BN(y1) + r) (res_mode 1) or relu(BN(y1) + BN(y2)) (res_mode 2), training mode: statistics
    from the per-tile partials merged by Chan's formula, running statistics, value, mask bytes, and every
    gradient of sum(out * dA)"""
    g = _gen(3 + two)
    N, H, W, C, tile, eps, mom = 2, 5, 7, 8, 16, 1e-5, 0.1
    M = N * H * W
    y1 = (3 + 0.5 * torch.randn(N, H, W, C, generator=g, dtype=F64)).requires_grad_()
    y2 = torch.randn(N, H, W, C, generator=g, dtype=F64).requires_grad_()
    dA = torch.randn(N, H, W, C, generator=g, dtype=F64)
    gam = [(torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_() for _ in range(2)]
    bet = [torch.randn(C, generator=g, dtype=F64).requires_grad_() for _ in range(2)]
    rm = [torch.randn(C, generator=g, dtype=F64) for _ in range(2)]
    rv = [torch.rand(C, generator=g, dtype=F64) + 0.5 for _ in range(2)]
    # PyTorch
    trm, trv = [t.clone() for t in rm], [t.clone() for t in rv]
    b1 = F.batch_norm(_nchw(y1), trm[0], trv[0], gam[0], bet[0], True, mom, eps)
    b2 = F.batch_norm(_nchw(y2), trm[1], trv[1], gam[1], bet[1], True, mom, eps) if two else _nchw(y2)
    out = torch.relu(b1 + b2)
    (out * _nchw(dA)).sum().backward()
    # reference: statistics from tile partials
    fin = []
    for y, k in ((y1, 0), (y2, 1)):
        part, _, ks = R.channel_stats(y.detach().reshape(M, C), tile)
        assert ks == [16, 16, 16, 16, 6] and part.shape == (5, 2, C)
        cnt = torch.tensor(ks, dtype=F64).unsqueeze(1)
        mean = part[:, 0].sum(0) / M
        m2 = (part[:, 1] + cnt * (part[:, 0] / cnt - mean) ** 2).sum(0)
        bm, bv = R.batch_stats(y.detach().reshape(M, C))
        _close(mean, bm, "merged mean")
        _close(m2 / M, bv, "merged variance")
        fin.append(R.bn_finalize(bm, bv, M, gam[k], bet[k], rm[k], rv[k], mom, eps))
    for k in range(2 if two else 1):
        _close(fin[k]["rmean"], trm[k], "running mean")
        _close(fin[k]["rvar"], trv[k], "running var")
    f1, f2 = fin
    Y1, Y2 = y1.detach().reshape(M, C), y2.detach().reshape(M, C)
    if two:
        val, mag, bits, pre = R.bn_apply(Y1, f1["scale"], f1["shift"], Y2, f2["scale"], f2["shift"], 2, 1, torch.float32)
    else:
        val, mag, bits, pre = R.bn_apply(Y1, f1["scale"], f1["shift"], Y2, None, None, 1, 1, torch.float32)
    want = _nhwc(out.detach()).reshape(M, C)
    _close(val, want, "bn_apply value")
    assert bool((mag >= pre.abs() * (1 - 1e-12)).all())
    mask = want > 0
    assert torch.equal(bits, R.pack_mask(mask, 4)) and torch.equal(R.unpack_mask(bits, 4), mask)
    b = R.bn_bwd(dA.reshape(M, C), mask, Y1, f1["mean"], f1["invstd"], Y2 if two else None, f2["mean"] if two else None,
                 f2["invstd"] if two else None, gam[0], gam[1] if two else None, M)
    _close(b["dy1"], y1.grad.reshape(M, C), "dy1")
    _close(b["sums"][1], gam[0].grad, "dgamma1")
    _close(b["sums"][0], bet[0].grad, "dbeta1")
    assert bool((b["sums_mag"] >= b["sums"].abs() * (1 - 1e-12)).all())
    if two:
        _close(b["dy2"], y2.grad.reshape(M, C), "dy2")
        _close(b["sums"][2], gam[1].grad, "dgamma2")
        _close(b["sums"][0], bet[1].grad, "dbeta2")
        assert b["coef"].shape == (6, C)
    else:
        _close(b["dz"], y2.grad.reshape(M, C), "dz (the residual's gradient)")
        assert b["coef"].shape == (3, C)
    _close(b["coef"][1], bet[0].grad / M, "coef mean dz")


def test_bn_eval_relu_bwd_add_colsum():
    g = _gen(5)
    C, M = 7, 33
    gam, bet, rm = (torch.randn(C, generator=g, dtype=F64) for _ in range(3))
    rv, cb = torch.rand(C, generator=g, dtype=F64) + 0.1, torch.randn(C, generator=g, dtype=F64)
    x = torch.randn(1, C, M, 1, generator=g, dtype=F64)
    sc, sh, _ = R.bn_eval_coeffs(gam, bet, rm, rv, 1e-5)
    _close(x * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1), F.batch_norm(x, rm, rv, gam, bet, False, 0.1, 1e-5), "eval BN")
    sc2, sh2, mag2 = R.bn_eval_coeffs(gam, bet, rm, rv, 1e-5, cb)
    _close((x + cb.view(1, C, 1, 1)) * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1),
           x * sc2.view(1, C, 1, 1) + sh2.view(1, C, 1, 1), "folded conv bias")
    A = torch.randn(M, C, generator=g, dtype=F64).requires_grad_()
    dA = torch.randn(M, C, generator=g, dtype=F64)
    bias = torch.zeros(C, dtype=F64, requires_grad=True)
    (torch.relu(A) * dA).sum().backward()
    dY, s, smag = R.relu_bwd_bias(dA, A.detach())
    _close(dY, A.grad, "relu backward")
    _close(s, A.grad.sum(0), "bias gradient")
    v, m = R.add(dA, dY)
    _close(v, dA + dY, "add")
    part = torch.randn(5, C, generator=g, dtype=F64)
    _close(R.colsum(part, 0)[0], part.sum(0), "colsum")
    _close(R.colsum(part, 1, s)[0], part.sum(0) + s, "colsum accumulate")
    assert bias.grad is None


@pytest.mark.parametrize("k,s,ceil", [(2, 2, False), (3, 2, True), (3, 1, False), (2, 2, True)])
@pytest.mark.parametrize("N,H,W,C", [(2, 6, 10, 4), (1, 7, 9, 3), (3, 3, 4, 5)])
def test_maxpool(k, s, ceil, N, H, W, C):
    g = _gen(H * 10 + W + k)
    x = torch.randint(0, 4, (N, H, W, C), generator=g).to(F64)  # small integers: many ties
    xt = _nchw(x).requires_grad_()
    want, ind = F.max_pool2d(xt, k, s, 0, 1, ceil, return_indices=True)
    y, idx, backward = R.maxpool(x, k, s, ceil)
    assert y.shape == _nhwc(want).shape
    assert torch.equal(y, _nhwc(want.detach()))
    P, Q = y.shape[1], y.shape[2]
    r, u = (idx // k).to(torch.int64), (idx % k).to(torch.int64)
    flat = (torch.arange(P).view(1, P, 1, 1) * s + r) * W + torch.arange(Q).view(1, 1, Q, 1) * s + u
    assert torch.equal(flat, _nhwc(ind)), "argmax positions (ties go to the first in raster order)"
    dy = torch.randn(N, P, Q, C, generator=g, dtype=F64)
    (want * _nchw(dy)).sum().backward()
    dx, mag, kk = backward(dy)
    _close(dx, _nhwc(xt.grad), "maxpool backward")
    dx0 = torch.randn(N, H, W, C, generator=g, dtype=F64)
    dxa, maga, kka = backward(dy, dx0)
    _close(dxa, _nhwc(xt.grad) + dx0, "maxpool backward, accumulated")
    assert kka == kk + 1 and bool((maga >= dxa.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (5, 7), (7, 2), (16, 16)])
def test_upsample2x(align, h, w):
    g = _gen(h * 20 + w)
    x = torch.randn(2, h, w, 3, generator=g, dtype=F64)
    xt = _nchw(x).requires_grad_()
    want = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=align)
    y, mag, backward = R.upsample2x(x, align, index_dtype=F64)
    _close(y, _nhwc(want.detach()), "upsample2x")
    dy = torch.randn(2, 2 * h, 2 * w, 3, generator=g, dtype=F64)
    (want * _nchw(dy)).sum().backward()
    _close(backward(dy)[0], _nhwc(xt.grad), "upsample2x backward")
    # the fp32 index rule moves a weight by no more than an fp32 rounding of the source coordinate
    y32 = R.upsample2x(x, align)[0]
    assert float((y32 - y).abs().max()) <= 2.0 ** -20 * float(x.abs().max()) * max(h, w)


@pytest.mark.parametrize("h,w,oh,ow,align", RESIZE_CASES)
def test_resize_values_float64(h, w, oh, ow, align):
    """with the source coordinates in float64 (the precision ATen uses for float64 tensors) the matrix form equals
    F.interpolate(size=...) and its autograd to 1e-12, for both align_corners settings"""
    for al in (align, not align):
        g = _gen(h * 100 + ow)
        x = torch.randn(2, h, w, 5, generator=g, dtype=F64)
        xt = _nchw(x).requires_grad_()
        want = F.interpolate(xt, size=(oh, ow), mode="bilinear", align_corners=al)
        y, mag, backward = R.resize(x, oh, ow, al, index_dtype=F64)
        _close(y, _nhwc(want.detach()), f"resize align={al}")
        assert bool((mag >= y.abs() * (1 - 1e-12)).all())
        dy = torch.randn(2, oh, ow, 5, generator=g, dtype=F64)
        (want * _nchw(dy)).sum().backward()
        dx, m, kk = backward(dy)
        _close(dx, _nhwc(xt.grad), f"resize backward align={al}")
        dx0 = torch.randn(2, h, w, 5, generator=g, dtype=F64)
        _close(backward(dy, dx0)[0], _nhwc(xt.grad) + dx0, "resize backward, accumulated")


@pytest.mark.parametrize("n_in,n_out", sorted({(a, b) for h, w, oh, ow, _ in RESIZE_CASES for a, b in ((h, oh), (w, ow))}
                                               | {(5, 10), (7, 14), (16, 32), (3, 6)}))
@pytest.mark.parametrize("align", [False, True])
def test_resize_index_rule_float32(n_in, n_out, align):
    """the float32 rule: F.interpolate of float32 one-hot rows shows the taps ATen selects and their weights.
    The half-pixel source coordinate has two fp32 evaluations: one fused multiply-add (the library's rule, and
    ATen's wherever its build contracts the expression: GPU, AVX2 and later) or the product rounded first
    (ATen's baseline CPU kernels); they differ by at most one rounding of a value below n_in + 0.5.  Whichever
    ATen used on this host, the reference's matrix of that form has exactly its non-zero pattern and its
    weights to one fp32 rounding (ATen rounds 1 - l1, the reference keeps it exact).  With align_corners there
    is one product and one form."""
    eye = torch.eye(n_in, dtype=torch.float32).view(n_in, 1, n_in, 1)  # image i = one-hot row i
    got = F.interpolate(eye, size=(n_out, 1), mode="bilinear", align_corners=align)[:, 0, :, 0].t().to(F64)
    Wm = R.axis_matrix(n_in, n_out, align)
    Wu = R.axis_matrix(n_in, n_out, align, fused=False)
    assert Wm.shape == got.shape == (n_out, n_in)
    if align:
        assert torch.equal(Wm, Wu)
    assert float((Wm - Wu).abs().max()) <= 2.0 ** -24 * (n_in + 0.5)
    fits = [torch.equal(Wf != 0, got != 0) and float((Wf - got).abs().max()) <= 2.0 ** -24 for Wf in (Wm, Wu)]
    assert any(fits), ("ATen's taps or weights match neither evaluation of the rule",
                       float((Wm - got).abs().max()), float((Wu - got).abs().max()))
    _close(Wm.sum(1), torch.ones(n_out, dtype=F64), "weights sum to one")
    i0, i1, l1 = R.axis_taps(n_in, n_out, align)
    assert bool(((i1 == i0) | (i1 == i0 + 1)).all()) and int(i1.max()) <= n_in - 1 and bool((l1 >= 0).all())


@pytest.mark.parametrize("h,w,oh,ow", [(5, 6, 8, 9), (5, 6, 5, 9), (1, 1, 1, 1)])
def test_pad2d(h, w, oh, ow):
    g = _gen(oh)
    for top, left in {(0, 0), (min(1, oh - h), min(2, ow - w)), (oh - h, ow - w)}:
        x = torch.randn(2, h, w, 3, generator=g, dtype=F64)
        xt = _nchw(x).requires_grad_()
        want = F.pad(xt, (left, ow - w - left, top, oh - h - top))
        y, backward = R.pad2d(x, top, left, oh, ow)
        assert torch.equal(y, _nhwc(want.detach()))
        dy = torch.randn(2, oh, ow, 3, generator=g, dtype=F64)
        (want * _nchw(dy)).sum().backward()
        dx, mag, kk = backward(dy)
        assert kk == 0 and torch.equal(dx, _nhwc(xt.grad))
        dx0 = torch.randn(2, h, w, 3, generator=g, dtype=F64)
        dxa, _, kka = backward(dy, dx0)
        assert kka == 1
        _close(dxa, _nhwc(xt.grad) + dx0, "pad backward, accumulated")


# ---- the helpers themselves --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ulp_store(dtype):
    p = 7 if dtype == torch.bfloat16 else 23
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, 3.0e-3, 1000.0, -1.0, 1.0 - 2.0 ** -30, 0.0], dtype=F64)
    want = torch.tensor([2.0 ** -p, 2.0 ** -p, 2.0 ** (1 - p), 2.0 ** (-1 - p), 2.0 ** (-9 - p), 2.0 ** (9 - p),
                         2.0 ** -p, 2.0 ** (-1 - p), 2.0 ** (-126 - p)], dtype=F64)
    assert torch.equal(R.ulp_store(v, dtype), want)
    # the spacing of the type itself
    one = torch.ones((), dtype=dtype)
    assert float(torch.nextafter(one, one * 2) - one) == 2.0 ** -p if dtype == torch.float32 else True


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_assert_elementwise(dtype):
    g = _gen(1)
    ref = torch.randn(6, 8, generator=g, dtype=F64)
    mag = ref.abs()
    good = R.round_store(ref, dtype)
    worst = R.assert_elementwise(good, ref, mag, dtype, 0)
    assert 0.0 <= worst <= 0.5 + 1e-9  # rounding to nearest: half a spacing
    bad = good.to(F64).clone()
    bad[3, 5] += 2 * float(R.ulp_store(ref[3, 5], dtype)) * (1 if bad[3, 5] >= ref[3, 5] else -1)
    with pytest.raises(AssertionError, match=r"worst at \[3, 5\]"):
        R.assert_elementwise(bad, ref, mag, dtype, 0)
    # k widens the bound by k fp32 roundings of the magnitude, no more
    off = ref + 3.0 * R.EPS32 * mag + R.ulp_store(ref, dtype) * 0.5
    assert R.assert_elementwise(off, ref, mag, dtype, 4) < 1.0
    with pytest.raises(AssertionError):
        R.assert_elementwise(ref + 6.0 * R.EPS32 * mag + R.ulp_store(ref, dtype), ref, mag, dtype, 4)
    nan = good.to(F64).clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"worst at \[0, 0\]"):
        R.assert_elementwise(nan, ref, mag, dtype, 4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fill", [R.SENTINEL, R.NAN])
def test_sliced_and_guard(dtype, fill):
    buf, view = R.sliced((3, 5), 8, 8 + 24, 8, dtype, fill)
    assert buf.shape == (3, 5, 32) and view.shape == (3, 5, 8)
    assert view.data_ptr() == buf.data_ptr() + 8 * buf.element_size() and view.stride(-2) == 32
    view.copy_(torch.randn(3, 5, 8).to(dtype))
    R.assert_guard(buf, 8, 8, fill)
    for c in (7, 16, 31, 0):  # the channel on either side of the slice, the ends of the row
        t = buf.clone()
        t[2, 4, c] = 1.0
        with pytest.raises(AssertionError, match="guard"):
            R.assert_guard(t, 8, 8, fill)
    # one touched byte: the sentinel's low byte flipped
    t = buf.clone()
    t.view(torch.uint8).view(3, 5, -1)[1, 2, 0] ^= 1
    with pytest.raises(AssertionError, match="guard"):
        R.assert_guard(t, 8, 8, fill)
    flat = torch.full((40,), 0xEE, dtype=torch.uint8)
    R.assert_tail(flat, 32, 0xEE)
    flat[32] = 0
    with pytest.raises(AssertionError):
        R.assert_tail(flat, 32, 0xEE)


# ---- narrow 1x1 heads, attention gate, global average pooling, input packing --------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_pw_heads(K):
    """pw_fwd / pw_bwd / pw_bwd_relu against F.conv2d (1x1) and its autograd: the value, dx (plain, accumulated and
    through the producer's ReLU) and the per-tile partials, which sum to the parameter gradients and of which
    the ragged last tile (one pixel) is that pixel's own outer product"""
    g = _gen(40 + K)
    N, HW, C, tile = 3, 43, 8, 128
    M = N * HW
    a = torch.randn(N, C, HW, 1, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(K, C, generator=g, dtype=F64).requires_grad_()
    b = torch.randn(K, generator=g, dtype=F64).requires_grad_()
    dy = torch.randn(N, K, HW, generator=g, dtype=F64)
    xin = torch.relu(a)
    xin.retain_grad()
    want = F.conv2d(xin, w.view(K, C, 1, 1), b)
    (want[..., 0] * dy).sum().backward()
    x = xin.detach()[..., 0].permute(0, 2, 1).reshape(M, C)
    y, mag = R.pw_fwd(x, w, b, N)
    assert y.shape == (N, K, HW)
    _close(y, want.detach()[..., 0], "pw_fwd")
    assert bool((mag >= y.abs() * (1 - 1e-12)).all())
    _close(R.pw_fwd(x, w, None, N)[0], want.detach()[..., 0] - b.detach().view(1, K, 1), "pw_fwd without bias")
    o = R.pw_bwd(dy, x, w, None, tile)
    nhwc = lambda t: t[..., 0].permute(0, 2, 1).reshape(M, C)
    _close(o["dx"], nhwc(xin.grad), "pw_bwd dx")
    assert o["n"] == [128, 1] and o["part_w"].shape == (K, C, 2) and o["part_b"].shape == (K, 2)
    _close(o["part_w"].sum(-1), w.grad, "part_w summed over the tiles")
    _close(o["part_b"].sum(-1), b.grad, "part_b summed over the tiles")
    last = dy.permute(0, 2, 1).reshape(M, K)[M - 1]
    _close(o["part_w"][:, :, 1], last.view(K, 1) * x[M - 1].view(1, C), "part_w of the one-pixel tile")
    _close(o["part_b"][:, 1], last, "part_b of the one-pixel tile")
    dx0 = torch.randn(M, C, generator=g, dtype=F64)
    oa = R.pw_bwd(dy, x, w, dx0, tile)
    _close(oa["dx"], nhwc(xin.grad) + dx0, "pw_bwd dx accumulated")
    assert bool((oa["dx_mag"] >= oa["dx"].abs() * (1 - 1e-12)).all())
    r = R.pw_bwd_relu(dy, x, w, tile, torch.bfloat16)
    _close(r["dx_pre"], nhwc(a.grad), "pw_bwd_relu dx before the store")
    assert torch.equal(r["dx"], R.round_store(r["dx_pre"], torch.bfloat16).to(F64))
    assert bool((r["dx"][x <= 0] == 0).all()) and int((x <= 0).sum()) > 0
    assert r["part_d"].shape == (2, 2, C) and bool((r["part_d"][:, 1] == 0).all())
    _close(r["part_d"][:, 0].sum(0), r["dx"].sum(0), "part_d slot 0 summed over the tiles")
    _close(r["part_d"][1, 0], r["dx"][M - 1], "part_d of the one-pixel tile")
    _close(r["part_w"], o["part_w"], "pw_bwd_relu part_w")


def test_attention_gate():
    """the gate's references chained as the op layer chains the kernels, against an autograd restatement of
    model/unet_attention.py:30-35 from the ReLU on: f = relu(pre), psi = BN(conv1x1(f)) with batch statistics,
    alpha = sigmoid(psi), out = skip * alpha"""
    g = _gen(77)
    M, Ci, Cs, tile, eps = 301, 8, 12, 128, 1e-5
    pre = torch.randn(M, Ci, generator=g, dtype=F64).requires_grad_()
    skip = torch.randn(M, Cs, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(1, Ci, generator=g, dtype=F64).requires_grad_()
    b = torch.randn(1, generator=g, dtype=F64).requires_grad_()
    gam = torch.tensor([1.3], dtype=F64, requires_grad=True)
    bet = torch.tensor([0.2], dtype=F64, requires_grad=True)
    dg = torch.randn(M, Cs, generator=g, dtype=F64)
    ds0 = torch.randn(M, Cs, generator=g, dtype=F64)
    f = torch.relu(pre)
    lin = f @ w.t() + b
    bn = F.batch_norm(lin.t().reshape(1, 1, M), None, None, gam, bet, True, 0.1, eps).reshape(M)
    al = torch.sigmoid(bn)
    out = skip * al.unsqueeze(1)
    (out * dg).sum().backward()
    # forward chain
    fd = f.detach()
    psi = R.pw_fwd(fd, w, b, 1)[0].reshape(M)
    _close(psi, lin.detach().reshape(M), "psi")
    part, pmag, ns = R.tile_stats(psi, tile)
    assert ns == [128, 128, 45] and part.shape == (3, 2)
    cnt = torch.tensor(ns, dtype=F64)
    mean = part[:, 0].sum() / M
    var = (part[:, 1] + cnt * (part[:, 0] / cnt - mean) ** 2).sum() / M
    _close(mean, psi.mean(), "merged mean of psi")
    _close(var, psi.var(unbiased=False), "merged variance of psi")
    fin = R.bn_finalize(mean.reshape(1), var.reshape(1), M, gam, bet, torch.zeros(1), torch.ones(1), 0.1, eps)
    alpha, z, zmag = R.attn_alpha(psi, fin["scale"], fin["shift"])
    _close(alpha, al.detach(), "alpha")
    assert bool((zmag >= z.abs() * (1 - 1e-12)).all())
    gated, gmag = R.attn_apply(skip.detach(), alpha)
    _close(gated, out.detach(), "gated")
    # backward chain
    b1 = R.attn_bwd1(dg, skip.detach(), alpha)
    _close(b1["dskip"], skip.grad, "dskip")
    _close(R.attn_bwd1(dg, skip.detach(), alpha, ds0)["dskip"], skip.grad + ds0, "dskip accumulated")
    p1, p1mag, n1 = R.attn_bwd1_part(b1["dpsibn"], psi, fin["mean"], fin["invstd"])
    assert p1.shape == (2, 3) and n1 == ns
    _close(p1[0].sum(), bet.grad[0], "sum dpsibn = dbeta")
    _close(p1[1].sum(), gam.grad[0], "sum dpsibn xhat = dgamma")
    coef = torch.stack([gam.detach()[0] * fin["invstd"][0], p1[0].sum() / M, p1[1].sum() / M])
    b2 = R.attn_bwd2(b1["dpsibn"], psi, fin["mean"], fin["invstd"], coef, fd, w, tile)
    _close(b2["dzf"], pre.grad, "dzf (through the ReLU)")
    assert bool((b2["dzf"][fd <= 0] == 0).all())
    assert b2["part_w"].shape == (Ci, 3) and b2["part_b"].shape == (3,) and b2["n"] == ns
    _close(b2["part_w"].sum(1), w.grad[0], "part_w summed over the tiles")
    # the bias in front of a batch-statistics BN has a zero gradient: hold the sum to its terms' magnitude
    assert abs(float(b2["part_b"].sum()) - float(b.grad[0])) <= 1e-12 * float(b2["dpsi"].abs().sum())
    _close(b2["part_w"][:, 2], b2["dpsi"][256:] @ fd[256:], "part_w of the ragged tile")
    for k in ("dpsi", "dzf", "part_w", "part_b"):
        assert bool((b2[k + "_mag"] >= b2[k].abs() * (1 - 1e-12)).all()), k


@pytest.mark.parametrize("B,HW,C", [(1, 1, 1), (3, 7, 8), (2, 300, 5)])
def test_gap(B, HW, C):
    g = _gen(B * 1000 + HW)
    x = torch.randn(B, HW, C, generator=g, dtype=F64).requires_grad_()
    dgp = torch.randn(B, C, generator=g, dtype=F64)
    (x.mean(1) * dgp).sum().backward()
    v, m = R.gap_fwd(x)
    _close(v, x.detach().mean(1), "gap_fwd")
    assert bool((m >= v.abs() * (1 - 1e-12)).all())
    _close(R.gap_bwd(dgp, HW)[0], x.grad, "gap_bwd")
    dx0 = torch.randn(B, HW, C, generator=g, dtype=F64)
    va, ma = R.gap_bwd(dgp, HW, dx0)
    _close(va, x.grad + dx0, "gap_bwd accumulated")
    assert bool((ma >= va.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("c,cpad", [(1, 1), (3, 8), (4, 16)])
def test_pack_input(c, cpad):
    g = _gen(c + cpad)
    x = torch.randn(2, c, 3, 5, generator=g)
    for dt in (torch.float32, torch.bfloat16):
        y = R.pack_input(x, cpad, dt)
        assert y.shape == (2, 3, 5, cpad) and y.dtype == dt
        assert torch.equal(y[..., :c], _nhwc(x).to(dt)) and bool((y[..., c:] == 0).all())
    if c <= 8:
        s = R.pack_input_stem(x)
        assert s.shape == (2, 3, 13, 8) and s.dtype == torch.bfloat16
        assert torch.equal(s[:, :, 3:8, :c], _nhwc(x).to(torch.bfloat16))
        assert bool((s[:, :, :3] == 0).all()) and bool((s[:, :, 8:] == 0).all()) and bool((s[..., c:] == 0).all())
