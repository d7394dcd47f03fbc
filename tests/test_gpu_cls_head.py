"""GPU: the multitask classification head and loss glue at op level (csrc/cls_head.hip gap_*, linear_*, ce_fwd;
csrc/loss.hip scale_grad; losses._MultiTaskFn), which the suite otherwise sees only inside whole-model runs
at I = 2048, O = 512 / 3.

ops.cls_head (model/unet_multitask.py:73-80: GAP -> FC -> ReLU -> Dropout -> FC) against float64 torch
at widths that reach linear_fwd_kernel's 8 x 64 unrolled body and its per-lane tail separately
(I = 200: tail only; I = 520: lanes 0..7 take one unrolled round, the others only the tail),
linear_bwd_x_kernel's 32-wide body and tail (O = 40, 31, 3, 2, 10), and ce_kernel's stride over
B > 256.  Tolerances as test_pw_head: 1e-5 relative to the maximum for fp32 tensors, 2e-2 for a bf16
tensor (the feature gradient), 1e-4 for parameter gradients.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _hw(HW):
    h = int(HW ** 0.5)
    while HW % h:
        h -= 1
    return h, HW // h


def _cls_head_case(dtname, N, HW, I, O1, O2, training, preload=False):
    from unetseg_hip import ops
    from unetseg_hip.lib import DT_BF16, DT_F32
    from unetseg_hip.nn import AdaptiveAvgPool2d, Dropout, Flatten, Linear, ReLU, Seq
    dt = DT_BF16 if dtname == "bf16" else DT_F32
    tdt = torch.bfloat16 if dtname == "bf16" else torch.float32
    g = torch.Generator().manual_seed(N * 1000 + I)
    torch.manual_seed(I + O1)
    head = Seq(AdaptiveAvgPool2d(1), Flatten(), Linear(I, O1), ReLU(), Dropout(0.5), Linear(O1, O2)).to(DEV)
    fc1, fc2, p = head[2], head[5], head[4].p
    H, W = _hw(HW)
    x = (torch.randn(N, H, W, I, generator=g) + 0.5).to(tdt).float()  # NHWC, representable in the mode's type
    keep = (torch.rand(N, O1, generator=g) >= p).float()
    dy = torch.randn(N, O2, generator=g)
    g0x = torch.randn(x.shape, generator=g).to(tdt).float()

    # float64 reference
    xr = x.double().requires_grad_(True)
    prm = [t.detach().cpu().double().requires_grad_(True) for t in (fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    h = F.relu(F.linear(xr.mean(dim=(1, 2)), prm[0], prm[1]))
    if training:
        h = h * keep.double() / (1.0 - p)
    ref = F.linear(h, prm[2], prm[3])
    ref.backward(dy.double())

    # the kernels accumulate into the parameter gradients: pre-fill them at the gradients' own scale
    pre = []
    for t, r in zip((fc1.weight, fc1.bias, fc2.weight, fc2.bias), prm):
        g0 = torch.randn(t.shape, generator=g) * r.grad.abs().max().float()
        t.grad = g0.to(DEV)
        pre.append(g0.double())

    ctx = ops.Ctx(dt, training, True, torch.device(DEV))
    feat = ops.Node(x.to(DEV).to(tdt))
    y, holder, mask = ops.cls_head(ctx, feat, head, dropout_mask=keep if training else None)
    assert _rel(y, ref.detach()) < 1e-5
    if training:
        assert torch.equal(mask.cpu(), keep)
    holder["grad"] = dy.to(DEV)
    if preload:
        feat.grad = g0x.to(DEV).to(tdt)
    ctx.backward()
    torch.cuda.synchronize()
    want = xr.grad + (g0x.double() if preload else 0.0)
    errs = [_rel(feat.grad.float(), want)] + [_rel(t.grad, g0 + r.grad) for t, g0, r in
                                              zip((fc1.weight, fc1.bias, fc2.weight, fc2.bias), pre, prm)]
    print(f"HEADERR cls_head {dtname} N{N} HW{HW} I{I} O{O1}/{O2} train={training} preload={preload}: "
          f"y {_rel(y, ref.detach()):.2e} dx {errs[0]:.2e} dW1 {errs[1]:.2e} db1 {errs[2]:.2e} dW2 {errs[3]:.2e} "
          f"db2 {errs[4]:.2e}")
    assert errs[0] < (2e-2 if dtname == "bf16" else 1e-5)
    assert max(errs[1:]) < 1e-4, errs


@pytest.mark.parametrize("dtname", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("N,HW,I,O1,O2", [(5, 24, 2048, 512, 3), (1, 1, 200, 40, 3), (3, 256, 520, 31, 2),
                                          (16, 4, 64, 64, 10)])
def test_cls_head(dtname, training, N, HW, I, O1, O2):
    """logits, feature gradient, both weight and bias gradients; train mode with a supplied keep-mask
    (scaled by 1 / (1 - p)) and eval mode"""
    _cls_head_case(dtname, N, HW, I, O1, O2, training)


@pytest.mark.parametrize("dtname", ["fp32", "bf16"])
def test_cls_head_second_consumer(dtname):
    """the feature node already holds a gradient (the decoder consumed feat5 too): gap_bwd accumulates"""
    _cls_head_case(dtname, 3, 256, 520, 31, 2, True, preload=True)


# ------------------------------------------------------------------------------------------------
# ce_fwd, scale_grad
# ------------------------------------------------------------------------------------------------
def _ce(c, t):
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P
    cd, td = c.to(DEV).contiguous(), t.to(DEV).contiguous()
    loss = torch.full((), -7.0, dtype=torch.float32, device=DEV)
    dlog = torch.full_like(cd, float("nan"))
    lib.ce_fwd(P(cd), P(td), c.shape[0], c.shape[1], P(loss), P(dlog), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return loss.cpu(), dlog.cpu()


@pytest.mark.parametrize("B,K", [(1, 3), (4, 3), (300, 10)])
def test_ce_fwd(B, K):
    """nn.CrossEntropyLoss() (mean, ignore_index -100) in float64; B = 300: the one block strides over
    the rows.  Bounds of test_ce_ignore_index."""
    g = torch.Generator().manual_seed(B)
    c = torch.randn(B, K, generator=g) * 2
    t = torch.randint(0, K, (B,), generator=g)
    if B > 1:
        t[torch.rand(B, generator=g) < 0.2] = -100
        t[1] = -100
        t[0] = K - 1
    c64 = c.double().requires_grad_(True)
    ref = F.cross_entropy(c64, t)
    ref.backward()
    loss, dlog = _ce(c, t)
    print(f"HEADERR ce_fwd B{B} K{K}: loss {abs(loss.item() - ref.item()):.2e} grad "
          f"{(dlog.double() - c64.grad).abs().max().item():.2e}")
    torch.testing.assert_close(loss.double(), ref.detach(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dlog.double(), c64.grad, rtol=1e-5, atol=1e-7)
    assert (dlog[t == -100] == 0).all()


def test_ce_fwd_all_ignored():
    """every row -100: a mean over nothing, NaN as torch; no row takes a gradient"""
    c = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))
    t = torch.full((5,), -100, dtype=torch.long)
    assert torch.isnan(F.cross_entropy(c.double(), t)).item()
    loss, dlog = _ce(c, t)
    assert torch.isnan(loss).item() and (dlog == 0).all()


@pytest.mark.parametrize("n", [1, 255, 70000])
@pytest.mark.parametrize("which", ["both", "s1_only", "s2_only"])
def test_scale_grad(n, which):
    """out = g * (s1[0] * a1 + s2[0] * a2), a NULL scalar counting as 0, against float64 at 1e-6"""
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    s1, a1, s2, a2 = 0.75, 1.5, 1.25, -0.3
    t1 = torch.tensor([s1], device=DEV) if which != "s2_only" else None
    t2 = torch.tensor([s2], device=DEV) if which != "s1_only" else None
    gd = g.to(DEV)
    out = torch.full_like(gd, float("nan"))
    lib.scale_grad(P(gd), n, P(t1), a1, P(t2), a2, P(out), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sc = (s1 * a1 if t1 is not None else 0.0) + (s2 * a2 if t2 is not None else 0.0)
    ref = g.double() * sc
    assert ((out.cpu().double() - ref).abs() <= 1e-6 * ref.abs()).all()


# ------------------------------------------------------------------------------------------------
# multitask_loss end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", ["total", "parts", "all"])
@pytest.mark.parametrize("kind", ["lovasz_hinge", "bce"])
def test_multitask_loss(kind, upstream):
    """total / seg / cls values and both logit gradients against oracle/ref_cpu.py multitask_loss
    (model/unet_multitask.py:119-139) at 4 x 1 x 97 x 131 (4 Lovasz tiles per image), with upstream
    gradients on `total`, on (seg_loss, cls_loss), and on all three: the g_total / g_seg / g_cls
    branches of _MultiTaskFn.backward.
    Lovasz: tie-free logits and the oracle in float32, loss 2e-6 / gradient 1e-5 of max
    (tests/test_gpu_losses_full.py); BCE: the oracle in float64, 1e-5 / 1e-5 of max
    (test_bce_and_confusion_bench_size); the CE term 1e-6 / 1e-5 of max (test_ce_ignore_index)."""
    from oracle import ref_cpu
    from test_gpu_losses_full import _tie_free
    from unetseg_hip import losses
    B, H, W, K, w = 4, 97, 131, 3, 0.7
    g = torch.Generator().manual_seed(41)
    if kind == "lovasz_hinge":
        # shifted so that both labels have positive hinge errors (tests/test_gpu_ignore_full.py SHIFT)
        seg, rdt, ltol = (_tie_free(B, H, W, g) + 3.375).unsqueeze(1), torch.float32, 2e-6
    else:
        seg, rdt, ltol = torch.randn(B, 1, H, W, generator=g) * 2, torch.float64, 1e-5
    cls = torch.randn(B, K, generator=g)
    seg_t = (torch.rand(B, H, W, generator=g) < 0.3).long()
    cls_t = torch.tensor([2, 0, 1, 1])
    coef = {"total": (1.7, 0.0, 0.0), "parts": (0.0, 0.6, 1.9), "all": (1.7, 0.6, 1.9)}[upstream]

    def run(fn, s, c, st, ct, **kw):
        s, c = s.detach().clone().requires_grad_(True), c.detach().clone().requires_grad_(True)
        tot, sl, cl = fn(s, c, st, ct, w, **kw)
        (coef[0] * tot + coef[1] * sl + coef[2] * cl).backward()
        return [v.item() for v in (tot.detach(), sl.detach(), cl.detach())], s.grad.detach().cpu().double(), c.grad.detach().cpu().double()

    rv, rs, rc = run(ref_cpu.multitask_loss, seg.to(rdt), cls.double() if rdt == torch.float64 else cls.clone(),
                     seg_t, cls_t, seg_loss=kind)
    hv, hs, hc = run(losses.multitask_loss, seg.to(DEV), cls.to(DEV), seg_t.to(DEV), cls_t.to(DEV), kind=kind)
    print(f"HEADERR multitask {kind} {upstream}: total/seg/cls rel "
          f"{[abs(a - b) / abs(b) for a, b in zip(hv, rv)]}  dseg {(hs - rs).abs().max().item() / rs.abs().max().item():.2e} "
          f"dcls {(hc - rc).abs().max().item() / rc.abs().max().item():.2e}")
    assert abs(hv[1] - rv[1]) <= ltol * abs(rv[1])
    assert abs(hv[2] - rv[2]) <= 1e-6 * abs(rv[2]) + 1e-6
    assert abs(hv[0] - rv[0]) <= 1e-5 * abs(rv[0])
    assert (hs - rs).abs().max().item() <= 1e-5 * rs.abs().max().item()
    assert (hc - rc).abs().max().item() <= 1e-5 * rc.abs().max().item()
