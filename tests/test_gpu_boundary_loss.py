"""GPU: the boundary loss (csrc/boundary_loss.hip, unetseg_boundary_loss_fwd; losses.boundary_loss,
signed_distance and boundary_weight= of the region losses) against the float64 reference of
tests/boundary_loss_ref.py (held to scipy, hand-written maps and autograd in tests/test_boundary_loss_cpu.py).

Shapes (B, H, W): 1x1x1, 2x5x7, 3x64x64, 2x65x129, 1x130x67 -- the transform's 64-pixel seams on both axes, every
tail of the 4-pixel vector (B H W mod 4 = 1, 2, 0, 2, 2; H W mod 4 = 1, 3, 0, 1, 2, so the second distance plane
and the second logit plane start unaligned) -- and 5x66x35, one batch of a normal image, one without foreground,
one that is all foreground, one that is all ignored (with ignore_index) and a normal one again: the 2 B batching
of the transform must keep the images and the fg / bg halves apart.  The listed shapes carry the same kinds in
that order as far as their B goes.  nch 1 and 2, with and without ignore_index.  Logits are 4 randn.

Bounds (derivation: DESIGN.md, "Boundary loss"; constants in tests/boundary_loss_ref.py):
  phi   sign and zero pattern exact; |phi| within 1 fp32 ulp of float32(sqrt(float64(d2))) (- 1 on fg)
  gz    |got - ref| <= 1.01 (15 + |z| [nch 2]) 2^-24 |ref| per element
  loss  |got - ref| <= 1.01 2^-24 (inv_norm / Nvalid sum (6 + |z| [nch 2]) |p phi| + |ref|)
Every run passes interior pointers of larger buffers: the 64 elements before and after gz and phi and the 256
bytes around the workspace must keep their fill.
"""
import functools
import math

import numpy as np
import pytest
import torch

import boundary_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = 255
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 64, 64), (2, 65, 129), (1, 130, 67), (5, 66, 35)]
GUARD = 64  # elements
WEIGHT = 0.75


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


def _make_targets(rng, B, H, W, ignore):
    """image b: normal, no foreground, all foreground, all ignored (normal without ignore), normal, ..."""
    t = (rng.random((B, H, W)) < 0.35).astype(np.int64)
    if H * W > 64:  # a solid region too, so that distances grow past a chunk of the row pass
        t[:, H // 4:H // 4 + H // 3, W // 5:W // 5 + W // 2] = 1
    if ignore:
        t[rng.random((B, H, W)) < 0.1] = IGN
    for b in range(B):
        kind = b % 5
        if kind == 1:
            t[b][t[b] == 1] = 0
        elif kind == 2:
            t[b] = 1
        elif kind == 3 and ignore:
            t[b] = IGN
    return t


@functools.lru_cache(maxsize=None)
def _case(shape, nch, ignore):
    """inputs and the float64 reference of one case, computed once and shared (read-only) by the tests"""
    B, H, W = shape
    rng = np.random.default_rng(1000 * B + 10 * H + W + nch + (7 if ignore else 0))
    out = (4 * rng.standard_normal((B, nch, H, W))).astype(np.float32)
    t = _make_targets(rng, B, H, W, ignore)
    inv = float(np.float32(1.0 / math.sqrt(H * H + W * W)))
    ign = IGN if ignore else None
    L, gz, phi = R.boundary_loss(out, t, ignore=ign, inv_norm=inv)
    d2fg, d2bg = R.sq_distances(t, ignore=ign)
    for a in (out, t, gz, phi, d2fg, d2bg):
        a.setflags(write=False)
    return dict(shape=shape, nch=nch, ign=ign, out=out, t=t, inv=inv, L=L, gz=gz, phi=phi, d2fg=d2fg, d2bg=d2bg,
                gz_bound=R.gz_bound(out, t, gz, nch), L_bound=R.loss_bound(out, t, nch, ignore=ign, inv_norm=inv))


def _guarded(n, dtype, fill, init=None, shift=0):
    """(buffer, view of n elements starting GUARD + shift elements in): the buffer is `fill` outside the view"""
    buf = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + n]
    if init is not None:
        view.copy_(init.reshape(-1))
    return buf, view


def _intact(buf, n, fill, shift=0):
    head, tail = buf[:GUARD + shift], buf[GUARD + shift + n:]
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def _run(case, weight=WEIGHT, accumulate=0, gz_init=None, want_gz=True, want_phi=True, shift=0):
    """one call of the entry point on guarded buffers -> (loss, gz, phi) on the host; asserts every guard.
    shift: elements by which out, tgt, gz and phi are moved off their 16-byte alignment"""
    from unetseg_hip.lib import lib
    B, H, W = case["shape"]
    n = B * H * W
    nan = float("nan")
    obuf, out = _guarded(n * case["nch"], torch.float32, 7.5, torch.tensor(case["out"]).to(DEV), shift)
    tbuf, tgt = _guarded(n, torch.int64, 1, torch.tensor(case["t"]).to(DEV), shift)
    gbuf, gz = _guarded(n, torch.float32, nan, gz_init if gz_init is not None else torch.full((n,), nan), shift)
    pbuf, phi = _guarded(n, torch.float32, nan, None, shift)
    phi.fill_(nan)
    nb = lib.boundary_loss_workspace(B, H, W)
    wbuf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    lbuf = torch.full((3,), nan, dtype=torch.float32, device=DEV)
    lib.boundary_loss_fwd(out.data_ptr(), case["nch"], tgt.data_ptr(), B, H, W, 1, -1 if case["ign"] is None else IGN,
                          case["inv"], float(weight), wbuf.data_ptr() + 256, nb, gz.data_ptr() if want_gz else None,
                          accumulate, phi.data_ptr() if want_phi else None, lbuf.data_ptr() + 4,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _intact(gbuf, n, nan, shift) and _intact(pbuf, n, nan, shift), "write outside gz / phi"
    assert _intact(obuf, n * case["nch"], 7.5, shift) and _intact(tbuf, n, 1, shift)
    assert bool((wbuf[:256] == 0xA5).all()) and bool((wbuf[256 + nb:] == 0xA5).all()), "write outside the workspace"
    assert math.isnan(lbuf[0].item()) and math.isnan(lbuf[2].item())
    assert torch.equal(out.cpu(), torch.tensor(case["out"]).reshape(-1)), "logits changed"
    assert torch.equal(tgt.cpu(), torch.tensor(case["t"]).reshape(-1)), "target changed"
    if not want_gz:
        assert bool(torch.isnan(gz).all())
    if not want_phi:
        assert bool(torch.isnan(phi).all())
    return lbuf[1].item(), gz.cpu().numpy().reshape(B, H, W), phi.cpu().numpy().reshape(B, H, W)


CASES = [(s, nch, ign) for s in SHAPES for nch in (1, 2) for ign in (False, True)]


@pytest.mark.parametrize("shape,nch,ignore", CASES)
def test_phi_gz_loss(shape, nch, ignore):
    case = _case(shape, nch, ignore)
    loss, gz, phi = _run(case)
    # phi: pattern exact, magnitude within one fp32 ulp of the rounded float64 root
    ref = case["phi"]
    assert np.array_equal(np.sign(phi), np.sign(ref)), "sign / zero pattern of phi"
    fg = case["t"] == 1
    d2 = np.where(fg, case["d2bg"], case["d2fg"])
    root = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    mag = np.where(fg, root - np.float32(1), root)
    nz = ref != 0
    err_phi = np.abs(np.abs(phi[nz]).astype(np.float64) - mag[nz].astype(np.float64))
    ulp = np.spacing(root[nz]).astype(np.float64)
    worst_phi = float((err_phi / ulp).max()) if nz.any() else 0.0
    # gz and the loss against the float64 reference
    gref, gb = WEIGHT * case["gz"], WEIGHT * case["gz_bound"]
    err = np.abs(gz.astype(np.float64) - gref)
    worst_gz = float((err[gb > 0] / gb[gb > 0]).max()) if (gb > 0).any() else 0.0
    lerr = abs(loss - case["L"])
    print(f"\nBLERR {shape} nch {nch} ign {ignore}: phi {worst_phi:.2f} ulp  gz {worst_gz:.3f} of bound  "
          f"loss {lerr:.3e} / bound {case['L_bound']:.3e}")
    assert worst_phi <= 1.0
    assert (err <= gb).all(), worst_gz
    assert (gz[gref == 0] == 0).all()  # ignored pixels and empty images: exactly 0
    assert lerr <= case["L_bound"], (loss, case["L"])


@pytest.mark.parametrize("shape,nch,ignore", [c for c in CASES if c[1] == 2 or c[0] == (2, 65, 129)])
def test_accumulate_repeat_and_optional_outputs(shape, nch, ignore):
    case = _case(shape, nch, ignore)
    n = int(np.prod(shape))
    loss, gz, phi = _run(case)
    # the same call again: bitwise
    loss2, gz2, phi2 = _run(case)
    assert np.float32(loss).tobytes() == np.float32(loss2).tobytes()
    assert gz.tobytes() == gz2.tobytes() and phi.tobytes() == phi2.tobytes()
    # accumulated onto zeros: the written bits
    lz, gzz, _ = _run(case, accumulate=1, gz_init=torch.zeros(n))
    assert gz.tobytes() == gzz.tobytes() and np.float32(lz).tobytes() == np.float32(loss).tobytes()
    # accumulated onto random values: the float sum
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1e-4
    _, gza, _ = _run(case, accumulate=1, gz_init=g0)
    want = (g0 + torch.from_numpy(gz).reshape(-1)).numpy().reshape(gz.shape)
    assert gza.tobytes() == want.tobytes()
    # gz and phi are optional; the loss does not depend on them or on the weight
    l3, _, _ = _run(case, weight=0.0, want_gz=False, want_phi=False)
    assert np.float32(l3).tobytes() == np.float32(loss).tobytes()


@pytest.mark.parametrize("nch", [1, 2])
def test_unaligned_pointers(nch):
    """out, tgt, gz and phi one element off their 16-byte alignment take the element loads and stores: same bits"""
    case = _case((2, 65, 129), nch, True)
    a = _run(case)
    b = _run(case, shift=1)
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- the Python layer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["B2HW", "B1HW", "BHW"])
@pytest.mark.parametrize("normalize", [True, False])
def test_boundary_loss_function(form, normalize):
    """losses.boundary_loss through autograd and losses.signed_distance, for the three logit layouts"""
    from unetseg_hip import losses
    nch = 2 if form == "B2HW" else 1
    case = _case((2, 65, 129), nch, True)
    B, H, W = case["shape"]
    inv = case["inv"] if normalize else 1.0
    L, gz, _ = R.boundary_loss(case["out"], case["t"], ignore=IGN, inv_norm=inv)
    o = torch.tensor(case["out"]).to(DEV)
    if form == "BHW":
        o = o[:, 0].contiguous()
    o.requires_grad_(True)
    t = torch.tensor(case["t"]).to(DEV)
    loss = losses.boundary_loss(o, t, ignore_index=IGN, normalize=normalize)
    (2.0 * loss).backward()
    scale = inv / case["inv"]
    assert abs(loss.item() - L) <= scale * case["L_bound"] + R.U * abs(L)
    g = o.grad.cpu().numpy().astype(np.float64)
    if nch == 2:
        assert np.array_equal(g[:, 0], -g[:, 1])
        g = g[:, 1]
    g = g.reshape(B, H, W)
    # weight 1 and the upstream 2 are exact factors; dz_to_dout multiplies twice more
    assert (np.abs(g - 2.0 * gz) <= 2.0 * scale * case["gz_bound"] + 2 * R.U * np.abs(2.0 * gz)).all()
    phi = losses.signed_distance(t, ignore_index=IGN).cpu().numpy()
    assert phi.dtype == np.float32 and phi.shape == (B, H, W)
    assert np.array_equal(np.sign(phi), np.sign(case["phi"]))
    assert (np.abs(phi - case["phi"]) <= R.K_PHI * R.U * np.abs(case["phi"])).all()


def _region_inputs(kind, nch, B, H, W):
    """logits for a region + boundary comparison: 4 randn; for the Lovasz hinge the tie-free grid of
    tests/test_gpu_losses_full.py (the sort order, hence the reference gradient, is then unique), with the
    multitask test's shift so that both labels have positive hinge errors"""
    from test_gpu_losses_full import _tie_free
    g = torch.Generator().manual_seed(17 + nch)
    if kind == "lovasz_hinge":
        z = _tie_free(B, H, W, g) + (3.375 if nch == 1 else 0.0)
    else:
        z = 4 * torch.randn(B, H, W, generator=g)
    if nch == 1:
        return z.unsqueeze(1)
    o0 = 4 * torch.randn(B, H, W, generator=g) if kind == "bce" else torch.zeros(B, H, W)
    return torch.stack([o0, (o0 + z) if kind == "bce" else z], 1)


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
@pytest.mark.parametrize("ignore", [False, True])
def test_binary_loss_with_boundary_weight(kind, ignore):
    """weight 0: torch.equal to the call without the argument; weight 0.3: region + w L against the references"""
    from oracle import ref_cpu
    from unetseg_hip import losses
    B, H, W, w = 2, 40, 67, 0.3  # small: the masked Lovasz oracle loops over single pixels
    t_np = _make_targets(np.random.default_rng(3), B, H, W, ignore)
    t_np[1] = _make_targets(np.random.default_rng(4), 1, H, W, ignore)[0]  # two normal images
    tgt = torch.from_numpy(t_np)
    ign = IGN if ignore else None
    out = _region_inputs(kind, 2, B, H, W)

    def hip(**kw):
        o = out.to(DEV).requires_grad_(True)
        loss = losses.binary_segmentation_loss(o, tgt.to(DEV), kind, ignore_index=ign, **kw)
        loss.backward()
        return loss.detach().cpu(), o.grad.cpu()

    l0, g0 = hip()
    l1, g1 = hip(boundary_weight=0.0)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    # region reference and tolerance of the existing tests: Lovasz without ignore_index in the oracle's fp32, 2e-6 /
    # 1e-5 of max (test_gpu_losses_full.py); the others in float64, 1e-5 / 1e-5 of max (test_gpu_ignore_full.py)
    rdt, ltol = (torch.float32, 2e-6) if kind == "lovasz_hinge" and not ignore else (torch.float64, 1e-5)
    o = out.clone().to(rdt).requires_grad_(True)
    region = ref_cpu.binary_segmentation_loss(o, tgt, kind, ignore_index=ign)
    region.backward()
    inv = float(np.float32(1.0 / math.sqrt(H * H + W * W)))
    o_np = out.numpy()
    L, gz, _ = R.boundary_loss(o_np, t_np, ignore=ign, inv_norm=inv)
    lw, gw = hip(boundary_weight=w)
    total = region.item() + w * L
    ltol_abs = ltol * abs(region.item()) + w * R.loss_bound(o_np, t_np, 2, ignore=ign, inv_norm=inv) + 3 * R.U * abs(total)
    rg = o.grad.double().numpy()
    gref = rg.copy()
    gref[:, 1] += w * gz
    gref[:, 0] -= w * gz
    gtol = 1e-5 * np.abs(rg).max() + w * R.gz_bound(o_np, t_np, gz, 2)[:, None] + 3 * R.U * np.abs(gref)
    gerr = np.abs(gw.double().numpy() - gref)
    print(f"\nBLERR binary {kind} ign {ignore}: loss err {abs(lw.item() - total):.3e} / {ltol_abs:.3e}  "
          f"grad worst {float((gerr / gtol).max()):.3f} of bound; boundary share of the gradient "
          f"{w * np.abs(gz).max() / np.abs(rg).max():.3f}")
    assert abs(lw.item() - total) <= ltol_abs
    assert (gerr <= gtol).all()
    assert not torch.equal(gw, g0)


@pytest.mark.parametrize("kind", ["bce", "lovasz_hinge"])
def test_multitask_loss_with_boundary_weight(kind):
    from oracle import ref_cpu
    from unetseg_hip import losses
    B, H, W, w, wc = 2, 40, 67, 0.3, 0.7
    t_np = _make_targets(np.random.default_rng(5), B, H, W, False)
    t_np[1] = _make_targets(np.random.default_rng(6), 1, H, W, False)[0]
    seg_t = torch.from_numpy(t_np)
    seg = _region_inputs(kind, 1, B, H, W)
    cls = torch.randn(B, 3, generator=torch.Generator().manual_seed(2))
    cls_t = torch.tensor([2, 0])

    def hip(**kw):
        s, c = seg.to(DEV).requires_grad_(True), cls.to(DEV).requires_grad_(True)
        tot, sl, cl = losses.multitask_loss(s, c, seg_t.to(DEV), cls_t.to(DEV), wc, kind, **kw)
        tot.backward()
        return [v.detach().cpu() for v in (tot, sl, cl)], s.grad.cpu(), c.grad.cpu()

    v0, s0, c0 = hip()
    v1, s1, c1 = hip(boundary_weight=0.0)
    assert all(torch.equal(a, b) for a, b in zip(v0, v1)) and torch.equal(s0, s1) and torch.equal(c0, c1)
    rdt, ltol = (torch.float32, 2e-6) if kind == "lovasz_hinge" else (torch.float64, 1e-5)
    s = seg.clone().to(rdt).requires_grad_(True)
    _, region, cl_ref = ref_cpu.multitask_loss(s, cls.to(rdt), seg_t, cls_t, wc, seg_loss=kind)
    region.backward()
    inv = float(np.float32(1.0 / math.sqrt(H * H + W * W)))
    L, gz, _ = R.boundary_loss(seg.numpy(), t_np, inv_norm=inv)
    vw, sw, cw = hip(boundary_weight=w)
    seg_total = region.item() + w * L
    tol = ltol * abs(region.item()) + w * R.loss_bound(seg.numpy(), t_np, 1, inv_norm=inv) + 3 * R.U * abs(seg_total)
    assert abs(vw[1].item() - seg_total) <= tol
    # the total is seg + wc * cls: test_gpu_cls_head.py's 1e-5, plus the boundary term's own bound
    total = seg_total + wc * cl_ref.item()
    assert abs(vw[0].item() - total) <= 1e-5 * abs(total) + tol
    assert torch.equal(vw[2], v0[2]) and torch.equal(cw, c0)
    rg = s.grad.double().numpy()[:, 0]
    gref = rg + w * gz
    gtol = 1e-5 * np.abs(rg).max() + w * R.gz_bound(seg.numpy(), t_np, gz, 1) + 3 * R.U * np.abs(gref)
    gerr = np.abs(sw.double().numpy()[:, 0] - gref)
    print(f"\nBLERR multitask {kind}: seg err {abs(vw[1].item() - seg_total):.3e} / {tol:.3e}  grad worst "
          f"{float((gerr / gtol).max()):.3f} of bound")
    assert (gerr <= gtol).all()
    assert not torch.equal(sw, s0)
