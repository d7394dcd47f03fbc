"""GPU: exact and per-element contract of the generic conv kernels (csrc/conv_generic.hip igemm_tn_kernel<T, BN>
and wgrad_kernel<T>, with the split-K reduce of csrc/conv_wgrad_reduce.hip) -- the whole fp32 parity mode and the
bf16 fallback of the dispatch -- through the C ABI, against the float64 references of tests/conv_generic_cases.py
(checked against PyTorch on the CPU in tests/test_conv_generic_cpu.py, which also proves that every case selects
the generic kernels in both dtypes).

Every (case, dtype, mode) makes the same call twice:

  packed   ld == channels, pointer at channel 0;
  strided  every activation operand is the slice [..., c0:c0+C] of its own wider buffer (ld and c0 multiples of
           8, different per tensor; one tail layout per direction), GUARD sentinel pixels before and after.
           Inputs and accumulated outputs carry SENTINEL outside the slice, written outputs NaN.
           F_dense_inplace instead reads channels [0, 96) and writes channels [96, 128) of one buffer with ld 160,
           as the dense block of dualdense_unet does.

and asserts
  * the mode's value contract on the packed result (conv_generic_cases: `exact` and `onehot` bit for bit against
    the float64 reference rounded once to the storage type, `randn` element by element at the derived k);
  * strided == packed bit for bit inside the slice;
  * every foreign channel and guard pixel of every buffer, inputs included, and the sentinel tails of the BN
    partials, dw and the exact-size weight-gradient workspace survive; inputs are unchanged;
  * elements no tap reaches are exactly zero when dx is initialised and keep dx0 bit for bit when accumulated;
  * BN partials of the stored output: the sums bit-exact in `exact` mode, sums and M2 (about the tile mean)
    against nhwc_ref.tile_stats at k = n and n + 3 (n rows of the tile), the rule of channel_stats in
    tests/test_gpu_elem_contract.py;
  * weight gradients: the slab count of the dispatch, and the accumulated second pass == exactly twice the first.

Each test prints one `generic-case` line: id, dtype, mode, worst |err| / bound, seconds; the module prints the
worst randn ratio per (direction, dtype) at the end (DESIGN.md section 4e records them).
"""
import time

import pytest
import torch

import conv_generic_cases as cg
import nhwc_ref as R
from nhwc_ref import NAN, SENTINEL

pytestmark = pytest.mark.gpu

DEV = "cuda"
#: sentinel pixels before and after every strided operand: two row tiles of the generic kernel, and more than
#: the W + 1 pixels a tap of the first / last row reaches past the tensor at the widths used here
GUARD = 256
TAIL = 64
F32 = torch.float32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()
    yield
    for (direction, dtname), r in sorted(WORST.items()):
        print(f"\nworst randn ratio  {direction:<10s} {dtname:<5s} {r:.4g}", end="")
    print()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtname):
    from unetseg_hip.lib import DT_BF16, DT_F32
    return DT_BF16 if dtname == "bf16" else DT_F32


def _rows(t):
    """[N][C][H][W] -> [N*H*W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _dev(t, dtype):
    return t.contiguous().to(dtype).to(DEV)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ne = R._bits(a.cpu()) != R._bits(b.cpu())
    n = int(ne.sum())
    if n:
        i = [int(v[0]) for v in torch.nonzero(ne, as_tuple=True)]
        raise AssertionError(f"{what}: {n} of {a.numel()} elements differ bit for bit; first at {i}: "
                             f"{a[tuple(i)].item()!r} != {b[tuple(i)].item()!r}")


def _contract(mode, got, ref, mag, store, k, what):
    """the mode's value contract; returns |err| / bound of the worst element (0 for the bit-exact modes)"""
    if mode == "randn":
        return R.assert_elementwise(got, ref, mag, store, k, what)
    _same(got, R.round_store(ref + 0.0, store), f"{what} ({mode}: the reference rounded once)")
    return 0.0


class _Buf:
    """one activation operand: `values` [M][C] float64 (None: an output that is written) as the channel slice
    [c0, c0 + C) of a [guard + M + guard][ld] buffer filled with `fill`; ld == C, c0 == 0 is the packed form"""

    def __init__(self, M, C, lay, dtype, fill, values=None):
        self.M, self.C, (self.ld, self.c0), self.fill = M, C, lay, fill
        self.g = 0 if (self.ld == C and self.c0 == 0) else GUARD
        self.buf, view = R.sliced((self.g + M + self.g,), C, self.ld, self.c0, dtype, fill, DEV)
        self.view = view[self.g:self.g + M]
        self.values = None
        if values is not None:
            self.values = _dev(values.reshape(M, C), dtype)
            self.view.copy_(self.values)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        return self.view.contiguous().cpu()

    def check(self, what, is_input):
        R.assert_guard(self.buf, self.c0, self.C, self.fill, f"{what} (foreign channels)")
        if self.g:
            R.assert_guard(self.buf[:self.g], 0, 0, self.fill, f"{what} (guard pixels before)")
            R.assert_guard(self.buf[self.g + self.M:], 0, 0, self.fill, f"{what} (guard pixels after)")
        if is_input:
            _same(self.view.contiguous(), self.values, f"{what}: an input was written")


def _report(cid, dtname, mode, direction, ratio, t0):
    if mode == "randn":
        WORST[(direction, dtname)] = max(WORST.get((direction, dtname), 0.0), ratio)
    print(f"generic-case {cid} {dtname} {mode}: worst ratio {ratio:.4g} {time.perf_counter() - t0:.2f}s")


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def _check_stats(stats, y_rows, mode, what):
    """stats [G][2][K] against the tile statistics of the stored output y_rows [M][K]"""
    y = R.f64(y_rows)
    G, _, K = stats.shape
    ref, mag = torch.zeros(G, 2, K, dtype=R.F64), torch.zeros(G, 2, K, dtype=R.F64)
    for c in range(K):
        ref[:, :, c], mag[:, :, c], ns = R.tile_stats(y[:, c], cg.TILE_M)
    assert len(ns) == G
    worst = 0.0
    for g, n in enumerate(ns):
        if mode == "exact":
            _same(stats[g, 0], ref[g, 0].to(F32), f"{what}: BN partial sums of tile {g}")
        worst = max(worst, R.assert_elementwise(stats[g, 0], ref[g, 0], mag[g, 0], F32, n, f"{what}: sums of tile {g}"),
                    R.assert_elementwise(stats[g, 1], ref[g, 1], mag[g, 1], F32, n + 3, f"{what}: M2 of tile {g}"))
    return worst


def _fwd_call(cid, dtname, d, shape, ep, lay):
    """one forward call; lay None: the in-place layout of F_dense_inplace.  -> {"y": [M][K], "stats": [G][2][K]}"""
    from unetseg_hip.lib import lib
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    store, dt = cg.STORE[dtname], _dt(dtname)
    P, Q = cg.out_hw(H, W, Rr, S, stride, pad)
    Mi, Mo = N * H * W, N * P * Q
    xr = _rows(d["x"])
    shared = None
    if lay is None:  # x1 = buf[..., 0:96], y = buf[..., 96:128], ld 160
        assert Mi == Mo and C2 == 0 and C1 + K == 128
        shared = torch.full((GUARD + Mi + GUARD, 160), SENTINEL, dtype=store, device=DEV)
        body = shared[GUARD:GUARD + Mi]
        xin = _dev(xr, store)
        body[:, :C1] = xin
        body[:, C1:C1 + K] = NAN
        x1p, ld1, yp, ldy, yview = body.data_ptr(), 160, body[:, C1:].data_ptr(), 160, body[:, C1:C1 + K]
        x2p = ld2 = 0
        bufs = []
    else:
        x1 = _Buf(Mi, C1, lay[0], store, SENTINEL, xr[:, :C1])
        x2 = _Buf(Mi, C2, lay[1], store, SENTINEL, xr[:, C1:]) if C2 else None
        y = _Buf(Mo, K, lay[-1], store, NAN)
        x1p, ld1, yp, ldy, yview = x1.ptr, x1.ld, y.ptr, y.ld, y.view
        x2p, ld2 = (x2.ptr, x2.ld) if C2 else (0, 0)
        bufs = [("x1", x1, True), ("y", y, False)] + ([("x2", x2, True)] if C2 else [])
    wk = _dev(d["w"].permute(0, 2, 3, 1), store)  # [K][R][S][C]
    bias = _dev(d["bias"], F32) if d["bias"] is not None else None
    esc = _dev(d["escale"], F32) if d["escale"] is not None else None
    relu = int(bool(ep.get("relu")))
    G = -(-Mo // cg.TILE_M)
    stt = torch.full((G * 2 * K + TAIL,), SENTINEL, dtype=F32, device=DEV) if ep.get("stats") else None
    if esc is not None:
        lib.conv2d_fwd_affine(dt, x1p, C1, ld1, x2p, C2, ld2, N, H, W, wk.data_ptr(), K, Rr, S, stride, pad,
                              esc.data_ptr(), bias.data_ptr(), relu, yp, ldy, _st())
    else:
        lib.conv2d_fwd(dt, x1p, C1, ld1, x2p, C2, ld2, N, H, W, wk.data_ptr(), K, Rr, S, stride, pad,
                       bias.data_ptr() if bias is not None else 0, relu, yp, ldy,
                       stt.data_ptr() if stt is not None else 0, _st())
    torch.cuda.synchronize()
    out = {"y": yview.contiguous().cpu()}
    if stt is not None:
        R.assert_tail(stt, G * 2 * K, SENTINEL, f"{cid} BN partials")
        out["stats"] = stt[:G * 2 * K].reshape(G, 2, K).cpu()
    for name, b, is_input in bufs:
        b.check(f"{cid} {name}", is_input)
    if shared is not None:
        R.assert_guard(shared, 0, C1 + K, SENTINEL, f"{cid} shared buffer (foreign channels)")
        R.assert_guard(shared[:GUARD], 0, 0, SENTINEL, f"{cid} shared buffer (guard pixels before)")
        R.assert_guard(shared[GUARD + Mi:], 0, 0, SENTINEL, f"{cid} shared buffer (guard pixels after)")
        _same(shared[GUARD:GUARD + Mi, :C1].contiguous(), xin, f"{cid}: the input channels of the shared buffer changed")
    return out


FWD_PARAMS = [(c, t, m) for c in cg.FWD_CASES for t in cg.STORE for m in cg.MODES] + \
             [(c, t, m) for c in cg.AFFINE_CASES for t in cg.STORE for m in cg.AFFINE_MODES]


@pytest.mark.parametrize("cid,dtname,mode", FWD_PARAMS, ids=["-".join(p) for p in FWD_PARAMS])
def test_forward(cid, dtname, mode):
    t0 = time.perf_counter()
    affine = cid in cg.AFFINE_CASES
    ep = dict(relu=cg.AFFINE_CASES[cid][1]) if affine else cg.FWD_CASES[cid][1]
    shape = cg.case_shape(cid, dtname)
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    store = cg.STORE[dtname]
    d = cg.make_data(cid, "fwd", shape, dtname, mode, bias=ep.get("bias", False), affine=affine)
    ref, mag = cg.ref_fwd(d["x"], d["w"], stride, pad, d["bias"], d["escale"], ep.get("relu", False))
    ref, mag = _rows(ref), _rows(mag)
    e = 1 if d["bias"] is not None else 0  # the bias add, or the affine fma that takes the bias along
    k = cg.k_rule(dtname, cg.max_products("fwd", shape), e)
    chs = cg.operand_channels("fwd", shape)
    packed = _fwd_call(cid, dtname, d, shape, ep, cg.packed_layout(chs))
    ratio = _contract(mode, packed["y"], ref, mag, store, k, f"{cid} {dtname} y")
    if "stats" in packed:
        if mode == "exact":  # the stored output is the rounded reference: so are its sums
            want = R.round_store(ref + 0.0, store)
            _same(packed["stats"][:, 0], torch.stack([t.to(R.F64).sum(0) for t in want.split(cg.TILE_M)]).to(F32),
                  f"{cid} {dtname}: BN partial sums")
        ratio = max(ratio, _check_stats(packed["stats"], packed["y"], mode, f"{cid} {dtname}"))
    lay = None if cid == "F_dense_inplace" else cg.layout(chs, cid in cg.TAIL_CASES)
    strided = _fwd_call(cid, dtname, d, shape, ep, lay)
    for name in packed:
        _same(strided[name], packed[name], f"{cid} {dtname} {name}: strided vs packed")
    _report(cid, dtname, mode, "fwd_affine" if affine else "fwd", ratio, t0)


# ------------------------------------------------------------------------------------------------
# data gradient
# ------------------------------------------------------------------------------------------------
def _dgrad_call(cid, dtname, d, shape, lay):
    from unetseg_hip.lib import lib
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    store, dt = cg.STORE[dtname], _dt(dtname)
    P, Q = cg.out_hw(H, W, Rr, S, stride, pad)
    Mi, Mo = N * H * W, N * P * Q
    dy = _Buf(Mo, K, lay[0], store, SENTINEL, _rows(d["dy"]))
    wt = _dev(d["w"].permute(1, 2, 3, 0), store)  # [C][R][S][K]
    out = {}
    for acc in (0, 1):
        dx = _Buf(Mi, C1, lay[1], store, SENTINEL if acc else NAN, _rows(d["dx0"]) if acc else None)
        lib.conv2d_dgrad(dt, dy.ptr, dy.ld, N, P, Q, wt.data_ptr(), K, C1, Rr, S, stride, pad, dx.ptr, dx.ld, H, W, acc,
                         _st())
        torch.cuda.synchronize()
        out[f"dx{acc}"] = dx.get()
        dx.check(f"{cid} dx (accumulate {acc})", False)
    dy.check(f"{cid} dy", True)
    return out


DGRAD_PARAMS = [(c, t, m) for c in cg.DGRAD_CASES for t in cg.STORE for m in cg.MODES]


@pytest.mark.parametrize("cid,dtname,mode", DGRAD_PARAMS, ids=["-".join(p) for p in DGRAD_PARAMS])
def test_dgrad(cid, dtname, mode):
    t0 = time.perf_counter()
    shape = cg.case_shape(cid, dtname)
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    store = cg.STORE[dtname]
    d = cg.make_data(cid, "dgrad", shape, dtname, mode)
    L = cg.max_products("dgrad", shape)
    chs = cg.operand_channels("dgrad", shape)
    packed = _dgrad_call(cid, dtname, d, shape, cg.packed_layout(chs))
    ratio = 0.0
    untouched = _rows(cg.products("dgrad", shape)) == 0
    for acc in (0, 1):
        ref, mag = cg.ref_dgrad(d["dy"], d["w"], H, W, stride, pad, d["dx0"] if acc else None)
        got = packed[f"dx{acc}"]
        ratio = max(ratio, _contract(mode, got, _rows(ref), _rows(mag), store, cg.k_rule(dtname, L, acc),
                                     f"{cid} {dtname} dx (accumulate {acc})"))
        # elements no tap reaches: exactly +0 when initialised, dx0 kept bit for bit when accumulated
        keep = R.round_store(_rows(d["dx0"]) if acc else torch.zeros(N * H * W, C1, dtype=R.F64), store)
        _same(got[untouched], keep[untouched], f"{cid} {dtname} elements no tap reaches (accumulate {acc})")
    strided = _dgrad_call(cid, dtname, d, shape, cg.layout(chs, cid in cg.TAIL_CASES))
    for name in packed:
        _same(strided[name], packed[name], f"{cid} {dtname} {name}: strided vs packed")
    _report(cid, dtname, mode, "dgrad", ratio, t0)


# ------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------
def _wgrad_call(cid, dtname, d, shape, opt, lay):
    from unetseg_hip.lib import lib, wgrad_config
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    C = C1 + C2
    store, dt = cg.STORE[dtname], _dt(dtname)
    P, Q = cg.out_hw(H, W, Rr, S, stride, pad)
    Mi, Mo = N * H * W, N * P * Q
    xr = _rows(d["x"])
    x1 = _Buf(Mi, C1, lay[0], store, SENTINEL, xr[:, :C1])
    x2 = _Buf(Mi, C2, lay[1], store, SENTINEL, xr[:, C1:]) if C2 else None
    dy = _Buf(Mo, K, lay[-1], store, SENTINEL, _rows(d["dy"]))
    x2p, ld2 = (x2.ptr, x2.ld) if C2 else (0, 0)
    kern, splits, _ = wgrad_config(dt, C1, x1.ld, C2, ld2, N, H, W, dy.ld, K, Rr, S, stride, pad)
    assert kern == "wgrad_generic", (cid, dtname, kern)
    assert splits == cg.generic_splits(dtname, K, Rr * S * C, Mo) == opt.get("splits", {}).get(dtname, splits), splits
    ws_bytes = lib.conv2d_wgrad_workspace(dt, N, P, Q, K, C, Rr, S)
    assert ws_bytes % 4 == 0 and ws_bytes >= splits * K * Rr * S * C * 4
    # the workspace starts as the (finite) sentinel: a slab the kernel leaves unwritten shows in dw
    ws = torch.full((ws_bytes // 4 + TAIL,), SENTINEL, dtype=F32, device=DEV)
    rows, dw_c = opt.get("dw_rows", K), opt.get("dw_c", C)
    nw = rows * dw_c * Rr * S
    dw = torch.full((nw + TAIL,), SENTINEL, dtype=F32, device=DEV)
    dw[:nw] = NAN
    out = {}
    for acc in (0, 1):
        if "dw_rows" in opt:
            lib.conv2d_wgrad_rows(dt, x1.ptr, C1, x1.ld, N, H, W, dy.ptr, dy.ld, K, Rr, S, stride, pad, ws.data_ptr(),
                                  ws_bytes, dw.data_ptr(), dw_c, acc, rows, _st())
        else:
            lib.conv2d_wgrad(dt, x1.ptr, C1, x1.ld, x2p, C2, ld2, N, H, W, dy.ptr, dy.ld, K, Rr, S, stride, pad,
                             ws.data_ptr(), ws_bytes, dw.data_ptr(), dw_c, acc, _st())
        torch.cuda.synchronize()
        out[f"dw{acc}"] = dw[:nw].reshape(rows, dw_c, Rr, S).cpu().clone()
    R.assert_tail(dw, nw, SENTINEL, f"{cid} dw")
    R.assert_tail(ws, ws_bytes // 4, SENTINEL, f"{cid} workspace")
    for name, b in [("x1", x1), ("dy", dy)] + ([("x2", x2)] if C2 else []):
        b.check(f"{cid} {name}", True)
    return out


WGRAD_PARAMS = [(c, t, m) for c in cg.WGRAD_CASES for t in cg.STORE for m in cg.MODES]


@pytest.mark.parametrize("cid,dtname,mode", WGRAD_PARAMS, ids=["-".join(p) for p in WGRAD_PARAMS])
def test_wgrad(cid, dtname, mode, monkeypatch):
    t0 = time.perf_counter()
    opt = cg.WGRAD_CASES[cid][1]
    for name, val in opt.get("env", {}).get(dtname, {}).items():
        monkeypatch.setenv(name, val)
    shape = cg.case_shape(cid, dtname)
    N, H, W, C1, C2, K, Rr, S, stride, pad = shape
    d = cg.make_data(cid, "wgrad", shape, dtname, mode)
    ref, mag = cg.ref_wgrad(d["x"], d["dy"], Rr, S, stride, pad)
    rows, dw_c = opt.get("dw_rows", K), opt.get("dw_c", C1 + C2)
    ref, mag = ref[:rows, :dw_c], mag[:rows, :dw_c]
    k = cg.k_rule(dtname, cg.max_products("wgrad", shape), 0)
    chs = cg.operand_channels("wgrad", shape)
    packed = _wgrad_call(cid, dtname, d, shape, opt, cg.packed_layout(chs))
    ratio = _contract(mode, packed["dw0"], ref, mag, F32, k, f"{cid} {dtname} dw")
    _same(packed["dw1"], packed["dw0"] + packed["dw0"], f"{cid} {dtname}: the accumulated second pass vs twice the first")
    strided = _wgrad_call(cid, dtname, d, shape, opt, cg.layout(chs, cid in cg.TAIL_CASES))
    for name in packed:
        _same(strided[name], packed[name], f"{cid} {dtname} {name}: strided vs packed")
    _report(cid, dtname, mode, "wgrad", ratio, t0)
