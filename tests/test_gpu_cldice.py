"""GPU: the soft skeleton and the soft-clDice loss (csrc/cldice.hip: unetseg_soft_skel_fwd / _bwd,
unetseg_cldice_fwd; losses.soft_skeleton, cldice_loss and cldice_weight= of the region losses) against the float64
reference of tests/cldice_ref.py (held to PyTorch autograd of the published code in tests/test_cldice_cpu.py,
which also asserts, for the inputs of tests/cldice_cases.py used here, that no selection and no relu is within
rounding of a tie).

Bounds (derivation: the head of tests/cldice_ref.py and DESIGN.md, "Soft clDice"), u = 2^-24:
  x_j       exact (read back from the workspace); at iters 0 the skeleton is fl32(relu(x - O(x))) bit for bit,
            which holds O(x_0) exact too
  S_k       |got - ref| <= 1.01 * 4 (k + 1) u
  gx        |got - ref| <= 1.01 * 24 (k + 1) u A, A the reference's sum of absolute terms; 0 where A is 0
  L, gz     cldice_ref.cldice's L_bound and gz_bound (the sums' and the fp32 sigmoid's errors carried through)
Every run passes interior pointers of larger buffers; the elements around every output and the bytes around the
workspace must keep their fill.
"""
import math

import numpy as np
import pytest
import torch

import cldice_cases as C
import cldice_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
WEIGHT = 0.75
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


def _guarded(n, dtype, fill, init=None, shift=0):
    """(buffer, view of n elements starting GUARD + shift elements in): the buffer is `fill` outside the view"""
    buf = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + n]
    if init is not None:
        view.copy_((init if isinstance(init, torch.Tensor) else torch.tensor(init)).reshape(-1))
    return buf, view


def _intact(buf, n, fill, shift=0):
    head, tail = buf[:GUARD + shift], buf[GUARD + shift + n:]
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_skel(case):
    """forward and backward through the C ABI on guarded buffers -> (skel, gx, [x_1 .. x_k] from the workspace)"""
    from unetseg_hip.lib import lib
    N, H, W = case["shape"]
    k, n = case["iters"], N * H * W
    xbuf, x = _guarded(n, torch.float32, 7.5, case["x"])
    gbuf, g = _guarded(n, torch.float32, 7.5, case["g"])
    sbuf, skel = _guarded(n, torch.float32, NAN)
    obuf, gx = _guarded(n, torch.float32, NAN)
    nb = lib.soft_skel_workspace(N, H, W, k)
    wbuf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wbuf.data_ptr() + 256
    lib.soft_skel_fwd(x.data_ptr(), N, H, W, k, ws, nb, skel.data_ptr(), _stream())
    lib.soft_skel_bwd(x.data_ptr(), N, H, W, k, ws, nb, g.data_ptr(), gx.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _intact(sbuf, n, NAN) and _intact(obuf, n, NAN), "write outside skel / gx"
    assert _intact(xbuf, n, 7.5) and _intact(gbuf, n, 7.5)
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + nb:] == 0xA5).all()), "write outside the workspace"
    assert torch.equal(x.cpu(), torch.tensor(case["x"]).reshape(-1)), "input changed"
    m = (4 * n + 255) // 256 * 256
    xs = [wbuf[256 + (j - 1) * m:256 + (j - 1) * m + 4 * n].cpu().view(torch.float32).numpy().reshape(N, H, W)
          for j in range(1, k + 1)]
    return skel.cpu().numpy().reshape(N, H, W), gx.cpu().numpy().reshape(N, H, W), xs


@pytest.mark.parametrize("shape,iters", C.SKEL_CASES)
def test_skeleton_forward_backward(shape, iters):
    case = C.skel_case(shape, iters)
    skel, gx, xs = _run_skel(case)
    lv = case["levels"]
    for j, xj in enumerate(xs, 1):
        assert np.array_equal(xj.astype(np.float64), lv[j]["x"]), f"x_{j} is not the exact selection"
    if iters == 0:
        want = np.maximum(case["x"] - lv[0]["o"].astype(np.float32), np.float32(0))
        assert skel.tobytes() == want.tobytes(), "O(x_0) is not the exact selection"
    ferr = np.abs(skel.astype(np.float64) - case["skel"])
    gb = R.grad_bound(case["A"], iters)
    gerr = np.abs(gx.astype(np.float64) - case["gx"])
    nz = case["A"] > 0
    worst_g = float((gerr[nz] / gb[nz]).max()) if nz.any() else 0.0
    print(f"\nCLERR skel {shape} k {iters}: fwd {ferr.max() / R.fwd_bound(iters):.3f} of bound  "
          f"grad {worst_g:.3f} of bound")
    assert (ferr <= R.fwd_bound(iters)).all()
    assert (skel[case["skel"] == 0] == 0).all()
    assert (gerr[nz] <= gb[nz]).all(), worst_g
    assert (gx[~nz] == 0).all()
    # the same calls again: bitwise
    skel2, gx2, _ = _run_skel(case)
    assert skel.tobytes() == skel2.tobytes() and gx.tobytes() == gx2.tobytes()


@pytest.mark.parametrize("form", ["NHW", "N1HW"])
def test_soft_skeleton_function(form):
    from unetseg_hip import losses
    case = C.skel_case((3, 13, 66), 3)
    x = torch.tensor(case["x"]).to(DEV)
    g = torch.tensor(case["g"]).to(DEV)
    if form == "N1HW":
        x, g = x.unsqueeze(1), g.unsqueeze(1)
    x.requires_grad_(True)
    s = losses.soft_skeleton(x)
    assert s.shape == x.shape and s.dtype == torch.float32
    (s * g).sum().backward()
    skel, gx, _ = _run_skel(case)
    assert s.detach().cpu().numpy().reshape(skel.shape).tobytes() == skel.tobytes()
    assert x.grad.cpu().numpy().reshape(gx.shape).tobytes() == gx.tobytes()
    with pytest.raises(ValueError):
        losses.soft_skeleton(x.detach().double())
    with pytest.raises(ValueError):
        losses.soft_skeleton(x.detach(), iters=65)


def _run_loss(case, weight=WEIGHT, accumulate=0, gz_init=None, want_gz=True, shift=0):
    """shift: elements by which out, tgt and gz are moved off their 16-byte alignment"""
    from unetseg_hip.lib import lib
    B, H, W = case["shape"]
    n, nch, k = B * H * W, case["nch"], case["iters"]
    obuf, out = _guarded(n * nch, torch.float32, 7.5, case["out"], shift)
    tbuf, tgt = _guarded(n, torch.int64, 1, case["t"], shift)
    gbuf, gz = _guarded(n, torch.float32, NAN, gz_init if gz_init is not None else torch.full((n,), NAN), shift)
    nb = lib.cldice_workspace(B, H, W, k)
    wbuf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    lbuf = torch.full((3,), NAN, dtype=torch.float32, device=DEV)
    lib.cldice_fwd(out.data_ptr(), nch, tgt.data_ptr(), B, H, W, -1 if case["ign"] is None else case["ign"], k, 1.0,
                   float(weight), wbuf.data_ptr() + 256, nb, gz.data_ptr() if want_gz else None, accumulate,
                   lbuf.data_ptr() + 4, _stream())
    torch.cuda.synchronize()
    assert _intact(gbuf, n, NAN, shift), "write outside gz"
    assert _intact(obuf, n * nch, 7.5, shift) and _intact(tbuf, n, 1, shift)
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + nb:] == 0xA5).all()), "write outside the workspace"
    assert math.isnan(lbuf[0].item()) and math.isnan(lbuf[2].item())
    assert torch.equal(out.cpu(), torch.tensor(case["out"]).reshape(-1)), "logits changed"
    if not want_gz:
        assert bool(torch.isnan(gz).all())
    return lbuf[1].item(), gz.cpu().numpy().reshape(B, H, W)


@pytest.mark.parametrize("case", C.LOSS_CASES)
def test_loss_and_gz(case):
    c = C.loss_case(*case)
    loss, gz = _run_loss(c)
    lerr = abs(loss - c["L"])
    gref, gb = WEIGHT * c["gz"], WEIGHT * c["gz_bound"]
    gerr = np.abs(gz.astype(np.float64) - gref)
    nz = gb > 0
    worst = float((gerr[nz] / gb[nz]).max()) if nz.any() else 0.0
    print(f"\nCLERR loss {case}: L {loss:.6f} err {lerr:.3e} / bound {c['L_bound']:.3e}  gz {worst:.3f} of bound")
    assert math.isfinite(loss) and np.isfinite(gz).all()
    assert lerr <= c["L_bound"], (loss, c["L"])
    assert (gerr[nz] <= gb[nz]).all(), worst
    assert (gz[~nz] == 0).all()  # ignored pixels: exactly 0
    if c["kind"] == "ignored":
        assert loss == 0.0 and not gz.any()
    # the loss needs neither gz nor the weight
    l2, _ = _run_loss(c, weight=0.0, want_gz=False)
    assert np.float32(l2).tobytes() == np.float32(loss).tobytes()


@pytest.mark.parametrize("case", [c for c in C.LOSS_CASES if c[0] in ((3, 13, 66), (2, 13, 21))])
def test_accumulate_and_repeat(case):
    c = C.loss_case(*case)
    n = int(np.prod(c["shape"]))
    loss, gz = _run_loss(c)
    loss2, gz2 = _run_loss(c)
    assert np.float32(loss).tobytes() == np.float32(loss2).tobytes() and gz.tobytes() == gz2.tobytes()
    lz, gzz = _run_loss(c, accumulate=1, gz_init=torch.zeros(n))
    assert np.array_equal(gz, gzz) and np.float32(lz).tobytes() == np.float32(loss).tobytes()
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1e-3
    _, gza = _run_loss(c, accumulate=1, gz_init=g0)
    want = (g0 + torch.from_numpy(gz).reshape(-1)).numpy().reshape(gz.shape)  # the product, then the sum
    assert gza.tobytes() == want.tobytes()


@pytest.mark.parametrize("nch", [1, 2])
def test_unaligned_pointers(nch):
    """out, tgt and gz one element off their 16-byte alignment take the element loads and stores: same bits.
    2574 pixels leave a tail group, and 858 per image put groups across two images"""
    c = C.loss_case((3, 13, 66), nch, True, 3, "mixed")
    a = _run_loss(c)
    b = _run_loss(c, shift=1)
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
    assert a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("form", ["B2HW", "B1HW", "BHW"])
def test_cldice_loss_function(form):
    from unetseg_hip import losses
    nch = 2 if form == "B2HW" else 1
    c = C.loss_case((3, 13, 66), nch, True, 3, "mixed")
    B, H, W = c["shape"]
    o = torch.tensor(c["out"]).to(DEV)
    if form == "BHW":
        o = o[:, 0].contiguous()
    o.requires_grad_(True)
    loss = losses.cldice_loss(o, torch.tensor(c["t"]).to(DEV), ignore_index=C.IGN)
    (2.0 * loss).backward()
    assert abs(loss.item() - c["L"]) <= c["L_bound"]
    g = o.grad.cpu().numpy().astype(np.float64)
    if nch == 2:
        assert np.array_equal(g[:, 0], -g[:, 1])
        g = g[:, 1]
    g = g.reshape(B, H, W)
    # weight 1 and the upstream 2 are exact factors; dz_to_dout multiplies twice more
    assert (np.abs(g - 2.0 * c["gz"]) <= 2.0 * c["gz_bound"] + 2 * R.U * np.abs(2.0 * c["gz"])).all()
    with pytest.raises(ValueError):
        losses.cldice_loss(o, torch.tensor(c["t"]).to(DEV), smooth=0.0)


def _strokes(B, H, W, seed):
    return C._targets(np.random.default_rng(seed), (B, H, W), False, "mixed")


#: (nch, ignore) -> seed of the BCE comparisons' logits, picked on the CPU so that C.conditions_hold
_BCE_SEED = {(2, False): 902, (2, True): 901, (1, False): 902}


def _composition_logits(kind, nch, B, H, W, ignore=False):
    """Lovasz: the tie-free grid of the region tests (the sort order, hence the reference gradient, is unique);
    its z step of 3 / 32768 keeps every p apart by 9e-5 of itself.  BCE: the loss cases' logits on a seed for
    which the clDice conditions hold (4 randn, as the region tests draw them, has a near-tie on most seeds)"""
    from test_gpu_boundary_loss import _region_inputs
    if kind == "lovasz_hinge":
        return _region_inputs(kind, nch, B, H, W)
    return torch.from_numpy(C._loss_inputs((B, H, W), nch, False, "mixed", _BCE_SEED[(nch, ignore)])[0])


def _conditions(kind, ref):
    if kind == "bce":
        return C.conditions_hold(ref["levels"], ref["p"], C.LOSS_MARGIN)
    return R.selection_margin(ref["levels"]) > C.LOSS_MARGIN


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
@pytest.mark.parametrize("ignore", [False, True])
def test_binary_loss_with_cldice_weight(kind, ignore):
    """weight 0: torch.equal to the call without the argument; weight 0.3: region + w L within the region tests'
    own bounds plus the term's; with the boundary term as well: the sum of all three"""
    from oracle import ref_cpu
    from unetseg_hip import losses
    import boundary_loss_ref as BR
    B, H, W, w = 2, 40, 67, 0.3
    t_np = _strokes(B, H, W, 3)
    if ignore:
        t_np[np.random.default_rng(4).random(t_np.shape) < 0.1] = C.IGN
    tgt = torch.from_numpy(t_np)
    ign = C.IGN if ignore else None
    out = _composition_logits(kind, 2, B, H, W, ignore)

    def hip(**kw):
        o = out.to(DEV).requires_grad_(True)
        loss = losses.binary_segmentation_loss(o, tgt.to(DEV), kind, ignore_index=ign, **kw)
        loss.backward()
        return loss.detach().cpu(), o.grad.cpu()

    l0, g0 = hip()
    l1, g1 = hip(cldice_weight=0.0)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    l1, g1 = hip(cldice_weight=0.0, cldice_iters=5)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    rdt, ltol = (torch.float32, 2e-6) if kind == "lovasz_hinge" and not ignore else (torch.float64, 1e-5)
    o = out.clone().to(rdt).requires_grad_(True)
    region = ref_cpu.binary_segmentation_loss(o, tgt, kind, ignore_index=ign)
    region.backward()
    rg = o.grad.double().numpy()
    ref = R.cldice(out.numpy(), t_np, iters=3, smooth=1.0, ignore=ign)
    assert _conditions(kind, ref)
    lw, gw = hip(cldice_weight=w)
    total = region.item() + w * ref["L"]
    ltol_abs = ltol * abs(region.item()) + w * ref["L_bound"] + 3 * R.U * abs(total)
    gref = rg.copy()
    gref[:, 1] += w * ref["gz"]
    gref[:, 0] -= w * ref["gz"]
    gtol = 1e-5 * np.abs(rg).max() + w * ref["gz_bound"][:, None] + 3 * R.U * np.abs(gref)
    gerr = np.abs(gw.double().numpy() - gref)
    print(f"\nCLERR binary {kind} ign {ignore}: loss err {abs(lw.item() - total):.3e} / {ltol_abs:.3e}  grad worst "
          f"{float((gerr / gtol).max()):.3f} of bound; clDice share of the gradient "
          f"{w * np.abs(ref['gz']).max() / np.abs(rg).max():.3f}")
    assert abs(lw.item() - total) <= ltol_abs
    assert (gerr <= gtol).all()
    assert not torch.equal(gw, g0)
    # both added terms
    wb = 0.05
    inv = float(np.float32(1.0 / math.sqrt(H * H + W * W)))
    Lb, gzb, _ = BR.boundary_loss(out.numpy(), t_np, ignore=ign, inv_norm=inv)
    l2, g2 = hip(cldice_weight=w, boundary_weight=wb)
    total2 = total + wb * Lb
    assert abs(l2.item() - total2) <= ltol_abs + wb * BR.loss_bound(out.numpy(), t_np, 2, ignore=ign, inv_norm=inv) \
        + 3 * R.U * abs(total2)
    gref2 = gref.copy()
    gref2[:, 1] += wb * gzb
    gref2[:, 0] -= wb * gzb
    gtol2 = gtol + wb * BR.gz_bound(out.numpy(), t_np, gzb, 2)[:, None] + 3 * R.U * np.abs(gref2)
    assert (np.abs(g2.double().numpy() - gref2) <= gtol2).all()


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
def test_multitask_loss_with_cldice_weight(kind):
    from oracle import ref_cpu
    from unetseg_hip import losses
    B, H, W, w, wc = 2, 40, 67, 0.3, 0.7
    t_np = _strokes(B, H, W, 5)
    seg_t = torch.from_numpy(t_np)
    seg = _composition_logits(kind, 1, B, H, W)
    cls = torch.randn(B, 3, generator=torch.Generator().manual_seed(2))
    cls_t = torch.tensor([2, 0])

    def hip(**kw):
        s, c = seg.to(DEV).requires_grad_(True), cls.to(DEV).requires_grad_(True)
        tot, sl, cl = losses.multitask_loss(s, c, seg_t.to(DEV), cls_t.to(DEV), wc, kind, **kw)
        tot.backward()
        return [v.detach().cpu() for v in (tot, sl, cl)], s.grad.cpu(), c.grad.cpu()

    v0, s0, c0 = hip()
    v1, s1, c1 = hip(cldice_weight=0.0)
    assert all(torch.equal(a, b) for a, b in zip(v0, v1)) and torch.equal(s0, s1) and torch.equal(c0, c1)
    rdt, ltol = (torch.float32, 2e-6) if kind == "lovasz_hinge" else (torch.float64, 1e-5)
    s = seg.clone().to(rdt).requires_grad_(True)
    _, region, cl_ref = ref_cpu.multitask_loss(s, cls.to(rdt), seg_t, cls_t, wc, seg_loss=kind)
    region.backward()
    ref = R.cldice(seg.numpy(), t_np, iters=3, smooth=1.0)
    assert _conditions(kind, ref)
    vw, sw, cw = hip(cldice_weight=w)
    seg_total = region.item() + w * ref["L"]
    tol = ltol * abs(region.item()) + w * ref["L_bound"] + 3 * R.U * abs(seg_total)
    assert abs(vw[1].item() - seg_total) <= tol
    total = seg_total + wc * cl_ref.item()
    assert abs(vw[0].item() - total) <= 1e-5 * abs(total) + tol
    assert torch.equal(vw[2], v0[2]) and torch.equal(cw, c0)
    rg = s.grad.double().numpy()[:, 0]
    gref = rg + w * ref["gz"]
    gtol = 1e-5 * np.abs(rg).max() + w * ref["gz_bound"] + 3 * R.U * np.abs(gref)
    gerr = np.abs(sw.double().numpy()[:, 0] - gref)
    print(f"\nCLERR multitask {kind}: seg err {abs(vw[1].item() - seg_total):.3e} / {tol:.3e}  grad worst "
          f"{float((gerr / gtol).max()):.3f} of bound")
    assert (gerr <= gtol).all()
    assert not torch.equal(sw, s0)
