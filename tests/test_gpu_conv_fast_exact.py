"""GPU: bit-exact contract of every fast bf16 conv configuration (csrc/conv_fast.hip, conv_halo.hip,
conv_tn_persist.hip, conv_first.hip, conv_wgrad_fast.hip, conv_wgrad_ring.hip, conv_wgrad_reduce.hip).

tests/test_gpu_configs.py and tests/test_gpu_conv_strided.py hold these kernels to float64 with random normal
data at norm-scaled tolerances, which a dropped pixel of a split-K slab, one misplaced 8-channel chunk of a long K
loop, a BN partial taken from the unrounded accumulator or the other rounding order of an accumulated gradient all
fit inside.  Here every case of STRIDED_CASES (its environment, its configuration keys, its shape), FIRST3X3_CASES,
the padded-K shapes, the head and the mask entry points is called packed (the strided test ties strided to packed
bit for bit) through the caller of that file, with the data of tests/conv_fast_exact_cases.py:

  exact   small integers and halves; tests/test_conv_fast_exact_cpu.py proves from the data that every asserted
          sum stays below 2^24, so fp32 accumulation is exact in any order and
            y, plain dx, masked d  == bf16_rn(reference) (bias and ReLU before the one rounding; masked: +0)
            accumulated dx         == ACC_RULE of the configuration (conv_fast_exact_cases)
            dw == reference as fp32, its accumulated second pass == twice it
            stats[g][0]            == the sum over tile g's rows of the stored y, per tile
            part[:, q] summed over the row tiles in float64 == the reference of the stored d (integers, halves)
            head logits == head_b + head_w . stored y;  mask bits == the sign of the stored y
          stats[g][1] (M2 about the tile mean) is not exact: nhwc_ref.channel_stats' rule of DESIGN.md 4a,
          k = n + 3 (n rows of the tile) -- the only bound of this file.
  onehot  one exact 15/16-bit product per output: y, dx == bf16_rn(product), dw == the product; pins every
          gather address.  Forward, plain data gradient (the accumulated pass by ACC_RULE), plain weight gradient.

The stem is out of scope: its input goes through the image packing path.
Each test prints one `exact-case` line: id, mode, configuration, seconds.
"""
import time

import pytest
import torch

import conv_fast_exact_cases as fx
import nhwc_ref as R
import test_gpu_conv_strided as tcs
from nhwc_ref import NAN
from test_gpu_configs import _P, _st

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = R._bits(got) != R._bits(want)
    n = int(ne.sum())
    if n:
        i = tuple(int(v[0]) for v in torch.nonzero(ne, as_tuple=True))
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ bit for bit; first at {list(i)}: got "
                             f"{got[i].item()!r}, expected {want[i].item()!r}")


def _equal64(got, want, what):
    """float64 sums of fp32 partials against the integer / half reference: equal"""
    ne = got != want
    n = int(ne.sum())
    if n:
        i = tuple(int(v[0]) for v in torch.nonzero(ne, as_tuple=True))
        raise AssertionError(f"{what}: {n} of {got.numel()} sums differ; first at {list(i)}: got {got[i].item()!r}, "
                             f"expected {want[i].item()!r}")


class _Op:
    """the attributes of test_gpu_configs._Op the caller reads, filled from a data dict"""

    def __init__(self, shape, d):
        N, H, W, C1, C2, K, R_, s = shape
        self.shape, self.pad = shape, R_ // 2
        self.P, self.Q = tcs._out_hw(H, W, R_, s)
        self.x, self.dy = d["x"].to(BF), d["dy"].to(BF)
        self.bias = d["bias"].to(F32)

    def x_parts(self):
        C1, C2 = self.shape[3], self.shape[4]
        return tcs._nhwc(self.x[:, :C1]), (tcs._nhwc(self.x[:, C1:]) if C2 else None)


class _Values:
    """the attributes of test_gpu_conv_strided._Values, filled from a data dict (float64, on the device)"""

    def __init__(self, direction, shape, d):
        self.op = _Op(shape, d)
        self.wk = d["w"].permute(0, 2, 3, 1).contiguous().to(BF)  # [K][R][S][C]
        self.wt = d["w"].permute(1, 2, 3, 0).contiguous().to(BF)  # [C][R][S][K]
        self.sc, self.sh = d["sc"].to(F32), d["sh"].to(F32)
        if "g0" in d:
            self.g0, self.z, self.y2 = d["g0"].to(BF), d["z"].to(BF), d["y2"].to(BF)
            self.aux = torch.relu(self.z) if direction == "post1" else self.z
            self.mu, self.inv, self.mu2, self.inv2 = (d[k].to(F32) for k in ("mu", "inv", "mu2", "inv2"))
            self.mbits = d["mbits"]


def _device(d):
    return {k: v.to(DEV) for k, v in d.items()}


def _check_stats(stats, tile, y_rows, key, nhw, what):
    """stats [G][2][K] against the stored rows of each tile (conv_fast_exact_cases.stats_rows): the sums bit for
    bit, M2 at k = n + 3"""
    y_rows = y_rows[fx.stats_rows(key, *nhw, tile).to(y_rows.device)]
    G = stats.shape[0]
    assert G == -(-y_rows.shape[0] // tile), (what, G, tile)
    _same(stats[:, 0].contiguous(), fx.tile_sums(y_rows, tile).to(F32), f"{what}: BN partial sums per tile")
    ref, mag, ns = R.channel_stats(y_rows, tile)
    st = stats.cpu()
    for g, n in enumerate(ns):
        R.assert_elementwise(st[g, 1], ref[g, 1], mag[g, 1], F32, n + 3, f"{what}: M2 of tile {g}")


def _check(cid, direction, shape, mode, d, out, keys):
    q = fx.query_class(direction)
    two = fx.acc_two_roundings(keys[0]) if q == "dgrad" else True
    ex = fx.expect(direction, shape, d, two)
    for name in ("y", "dx0", "dx1", "dx", "dw0", "dw1"):
        if name in ex:
            got = out[name].reshape(ex[name].shape)
            _same(got, ex[name], f"{cid} {mode} {name} ({', '.join(sorted(set(keys)))})")
    if "stats" in out and mode == "exact":
        N, H, W, _, _, _, R_, s_ = shape
        _check_stats(out["stats"], out["tile"], out["y"], keys[0], (N,) + tcs._out_hw(H, W, R_, s_), f"{cid} {mode}")
    if "part" in out:
        assert out["part"].shape[1] >= ex["part"].shape[0]
        got = out["part"].to(F64).sum(0)
        for i in range(ex["part"].shape[0]):
            _equal64(got[i], ex["part"][i], f"{cid} partial quantity {i}")


PARAMS = [(cid, mode) for cid, c in tcs.STRIDED_CASES.items() for mode in fx.MODES
          if mode == "exact" or c[0] in fx.ONEHOT_DIRECTIONS]


@pytest.mark.parametrize("cid,mode", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_fast_case(cid, mode, monkeypatch):
    t0 = time.perf_counter()
    direction, shape, expect, env, _ = tcs.STRIDED_CASES[cid]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    lay = tcs.packed_layout(tcs.operand_channels(direction, shape))
    keys = tcs.case_keys(direction, shape, lay)
    assert keys == expect, f"{cid}: selects {keys}, the case lists {expect}"
    d = _device(fx.make_data(direction, shape, mode, fx.NARROW.get(cid) if mode == "exact" else None))
    out, _ = tcs._call(direction, shape, _Values(direction, shape, d), lay)
    _check(cid, direction, shape, mode, d, out, keys)
    torch.cuda.synchronize()
    print(f"exact-case {cid} {mode}: config {','.join(sorted(set(keys)))} {time.perf_counter() - t0:.2f}s")


@pytest.mark.parametrize("mode", fx.MODES)
@pytest.mark.parametrize("direction,shape", tcs.FIRST3X3_CASES)
def test_first3x3(direction, shape, mode):
    """the first-3x3 kernel on the 8-channel packed image (ldc1 == 8)"""
    from unetseg_hip.lib import DT_BF16, fwd_config, lib
    N, H, W, C1, C2, K, R_, s = shape
    assert fwd_config(DT_BF16, 8, 8, 0, 0, N, H, W, K, 3, 3, 1, 1) == "first3x3"
    d = _device(fx.make_data(direction, shape, mode))
    v = _Values(direction, shape, d)
    M = N * H * W
    relu, stats = direction == "fwd_relu", direction == "fwd_stats"
    tile = lib.conv2d_fwd_tile_m(DT_BF16, 8, 8, 0, 0, N, H, W, K, 3, 3, 1, 1)
    G = -(-M // tile)
    y = torch.full((M, K), NAN, dtype=BF, device=DEV)
    stt = tcs._flat(G * 2 * K) if stats else None
    lib.conv2d_fwd(DT_BF16, _P(v.op.x_parts()[0]), 8, 8, 0, 0, 0, N, H, W, _P(v.wk), K, 3, 3, 1, 1,
                   _P(v.op.bias) if relu else 0, int(relu), _P(y), K, _P(stt), _st())
    torch.cuda.synchronize()
    _same(y, fx.expect(direction, shape, d)["y"], f"first3x3 {direction} {mode} y")
    if stats:
        R.assert_tail(stt, G * 2 * K, NAN, "first3x3 BN partials")
        if mode == "exact":
            _check_stats(stt[:G * 2 * K].reshape(G, 2, K), tile, y, "fwd:first3x3", (N, H, W), f"first3x3 {direction}")


@pytest.mark.parametrize("K,C1,H,W", fx.PADK_CASES)
def test_padk(K, C1, H, W):
    """the narrow 1x1 gradients on a 64-padded dY: unetseg_conv2d_wgrad_rows into rows 0..K-1 of dw, the padded-K
    unetseg_conv2d_dgrad (wt [C1][64], pad columns zero), plain and accumulated onto x"""
    from unetseg_hip.lib import DT_BF16, dgrad_config, lib, wgrad_config
    N, KP = fx.PADK_N, fx.PADK_KP
    M = N * H * W
    d = _device(fx.padk_data(K, C1, H, W))
    ex = fx.padk_expect(d, K)
    kd = dgrad_config(DT_BF16, KP, N, H, W, KP, C1, 1, 1, 1, 0, C1, H, W)
    assert all(fx.acc_two_roundings("dgrad:" + c) for c in kd), kd
    assert wgrad_config(DT_BF16, C1, C1, 0, 0, N, H, W, KP, KP, 1, 1, 1, 0)[0] != "wgrad_generic"
    x, dy = d["x"].to(BF), d["dy"].to(BF)
    wt = torch.zeros(C1, KP, dtype=BF, device=DEV)
    wt[:, :K] = d["w"].t().to(BF)
    ws_bytes = lib.conv2d_wgrad_workspace(DT_BF16, N, H, W, KP, C1, 1, 1)
    ws = torch.full((max(ws_bytes, 1) // 4 + 1,), NAN, dtype=F32, device=DEV)
    dw = torch.full((KP, C1), R.SENTINEL, dtype=F32, device=DEV)
    for acc in (0, 1):
        lib.conv2d_wgrad_rows(DT_BF16, _P(x), C1, C1, N, H, W, _P(dy), KP, KP, 1, 1, 1, 0, _P(ws), ws_bytes, _P(dw), C1,
                              acc, K, _st())
        torch.cuda.synchronize()
        _same(dw[:K].contiguous(), ex[f"dw{acc}"], f"padk dw rows (accumulate {acc})")
        R.assert_guard(dw[K:], 0, 0, R.SENTINEL, "dw rows past dw_rows")
    for acc in (0, 1):
        dx = x.clone() if acc else torch.full((M, C1), NAN, dtype=BF, device=DEV)
        lib.conv2d_dgrad(DT_BF16, _P(dy), KP, N, H, W, _P(wt), KP, C1, 1, 1, 1, 0, _P(dx), C1, H, W, acc, _st())
        torch.cuda.synchronize()
        _same(dx, ex[f"dx{acc}"], f"padk dx (accumulate {acc}, {kd})")


def _head_operands(hs, monkeypatch):
    monkeypatch.setenv("UNETSEG_HALO_HS", hs)
    shape = fx.HEAD_SHAPE
    d = _device(fx.make_data("fwd_relu", shape, "exact"))
    return shape, d, _Values("fwd_relu", shape, d), fx.expect("fwd_relu", shape, d)["y"]


@pytest.mark.parametrize("head_k,hs", fx.HEAD_CASES)
def test_fwd_head(head_k, hs, monkeypatch):
    """unetseg_conv2d_fwd_head: y, and the fp32 logits [n][head_k][h][w] = head_b + head_w . stored y, exactly"""
    from unetseg_hip.lib import DT_BF16, lib
    shape, d, v, want = _head_operands(hs, monkeypatch)
    N, H, W = shape[:3]
    M = N * H * W
    hd = _device(fx.head_data(head_k))
    hw, hb = hd["hw"].to(F32), hd["hb"].to(F32)
    assert lib.conv2d_fwd_head_ok(DT_BF16, 64, N, H, W, 64, head_k) == 1
    y = torch.full((M, 64), NAN, dtype=BF, device=DEV)
    logits = tcs._flat(N * head_k * H * W)
    lib.conv2d_fwd_head(DT_BF16, _P(v.op.x_parts()[0]), 64, N, H, W, _P(v.wk), _P(v.op.bias), _P(y), 64, head_k,
                        _P(hw), _P(hb), _P(logits), _st())
    torch.cuda.synchronize()
    R.assert_tail(logits, N * head_k * H * W, NAN, "logits")
    _same(y, want, f"head_k {head_k} y")
    _same(logits[:N * head_k * H * W].reshape(N, head_k, H, W), fx.head_expect(y, hd, N, H, W).contiguous(),
          f"head_k {head_k} logits")


@pytest.mark.parametrize("hs", fx.MASK_CASES)
def test_fwd_mask(hs, monkeypatch):
    """unetseg_conv2d_fwd_mask: y, and mask bits [M][8] naming the sign of the stored y"""
    from unetseg_hip.lib import DT_BF16, lib
    shape, d, v, want = _head_operands(hs, monkeypatch)
    N, H, W = shape[:3]
    M = N * H * W
    assert lib.conv2d_fwd_mask(DT_BF16, 0, 64, N, H, W, 0, 0, 0, 64, 0, 0) == 1
    y = torch.full((M, 64), NAN, dtype=BF, device=DEV)
    mb = torch.full((M * 8 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    lib.conv2d_fwd_mask(DT_BF16, _P(v.op.x_parts()[0]), 64, N, H, W, _P(v.wk), _P(v.op.bias), _P(y), 64, _P(mb), _st())
    torch.cuda.synchronize()
    R.assert_tail(mb, M * 8, 0xA5, "mask bits")
    _same(y, want, "mask y")
    bits = ((y.float() > 0).reshape(M, 8, 8).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1)
    assert torch.equal(mb[:M * 8].reshape(M, 8).to(torch.int32), bits), "mask bits are not the sign of the stored y"
    assert 0.2 < float((y == 0).float().mean()) < 0.8, "the ReLU zero is not exercised"
