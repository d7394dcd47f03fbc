"""Cases, data makers, expected results and the exactness budget of the bit-exact tests of the fast bf16 conv
kernels (csrc/conv_fast.hip, conv_halo.hip, conv_tn_persist.hip, conv_first.hip, conv_wgrad_fast.hip,
conv_wgrad_ring.hip, conv_wgrad_reduce.hip): tests/test_gpu_conv_fast_exact.py runs them on the GPU,
tests/test_conv_fast_exact_cpu.py checks this file on the CPU.  Nothing here imports the library or touches a GPU;
every function works on the device its operands live on.

The cases are those of tests/test_gpu_conv_strided.py -- every entry of STRIDED_CASES with its environment, its
configuration keys and its shape, FIRST3X3_CASES, the padded-K shapes of test_padk_strided, the head and the mask
entry points -- called packed.  The data makers and im2col references are those of tests/conv_generic_cases.py.

Two data modes:

  exact   x, w, dy, bias, the head weights: integers in [-3, 3] (NARROW lists the cases whose range is smaller);
          the accumulated-onto g0: integers in [-8, 8]; BN-on-load and post-op coefficients sc, sh integers in
          [-3, 3], mu in {-1, 0, 1}, inv in {0.5, 1, 2}; z, y2 integers in [-3, 3]; mbits random.  Every
          intermediate is an integer or a half, and budget() proves from the data that the absolute values of
          the terms of every asserted sum stay below 2^24 (2^23 for halves): fp32 accumulation is exact in any
          order, so every output is the float64 reference rounded where the kernel rounds, bit for bit.
  onehot  conv_generic_cases.onehot_weight / onehot_dy / _odd with the 8-bit field: every output is one exact
          15/16-bit product.  Forward, plain data gradient, plain weight gradient; BN-on-load with sc = 1, sh = 0.
          Two-source forward cases move the weights of output channels 1 and 2 to input channels C1 - 1 and C1.

The rounding of an accumulated data gradient (ACC_RULE, asserted per configuration):

  halo3                       dx = bf16_rn(dgrad + old)            the sum is formed in fp32, one rounding
  every TN configuration      dx = bf16_rn(bf16_rn(dgrad) + old)   (tiles, gather rings, halo-A rings, their
  (tn*, ring*, multi*)                                              persistent forms, the merged stride-2 classes:
                                                                    the epilogue rounds the gradient for its
                                                                    transpose / statistics, then adds)
  post 3 (TN only)            d = mask * bf16_rn(bf16_rn(dgrad) + old)
"""
import torch
import torch.nn.functional as F

import conv_generic_cases as cg

F64 = torch.float64
BF = torch.bfloat16
LIMIT = 2.0 ** 24
MODES = ("exact", "onehot")
#: directions the one-hot mode covers (post-ops are left to `exact`)
ONEHOT_DIRECTIONS = ("fwd_relu", "fwd_stats", "fwd_all", "fwd_bnrelu_in", "dgrad", "wgrad", "wgrad_bnrelu_in")

#: id -> {operand: largest |integer|} of the exact-mode cases whose default range [-3, 3] exceeds the budget
#: (post 2 on 2 x 128 x 128 x 192 from 1152 products: sum |d xhat| over the 32768 rows reaches 2^24.7 in halves)
NARROW = {"post2_ring256x128_halo": dict(dy=1), "post2_ring256x128_hp": dict(dy=1)}

#: the padded-K shapes of test_padk_strided: (K, C1, H, W), N = 2, dY padded to 64 columns
PADK_N, PADK_KP = 2, 64
PADK_CASES = [(K, C1, H, W) for (H, W) in ((15, 17), (16, 32)) for C1 in (64, 128) for K in (32, 40)]
#: unetseg_conv2d_fwd_head / _fwd_mask at the shapes of their strided tests: (N, H, W), 64 -> 64 channels, 3x3
HEAD_SHAPE = (3, 16, 64, 64, 0, 64, 3, 1)
HEAD_CASES = [(1, "0"), (2, "1")]  # (head_k, UNETSEG_HALO_HS)
MASK_CASES = ["1", "0"]  # UNETSEG_HALO_HS


def strided():
    """tests/test_gpu_conv_strided.py (imports no library at module level)"""
    import test_gpu_conv_strided as tcs
    return tcs


def query_class(direction):
    """fwd / bnin / dgrad / wgrad"""
    return strided()._QUERY[direction][1]


def acc_two_roundings(key):
    """ACC_RULE: does the configuration `key` ("dgrad:halo3", "dgrad_post3:tn128x128_1st", ...) round the data
    gradient to bf16 before it adds the old value?"""
    name = key.split(":")[1]
    assert name == "halo3" or name.startswith(("tn", "ring", "multi")), key
    return name != "halo3"


def bf16_rn(t):
    """float64 (an integer or half below 2^24: exact in fp32) -> bf16, round to nearest even; -0 -> +0"""
    return (t + 0.0).to(torch.float32).to(BF)


def rows(t):
    """[N][C][H][W] -> [N*H*W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unpack_bits(mbits, M, C):
    """uint8 [M * C/8] -> bool [M][C]: bit e of byte (p, c/8) is channel 8 (c/8) + e"""
    b = mbits.reshape(M, C // 8).to(torch.int32)
    return ((b.unsqueeze(-1) >> torch.arange(8, dtype=torch.int32, device=b.device)) & 1).bool().reshape(M, C)


# ------------------------------------------------------------------------------------------------
# float64 contractions: F.conv2d / F.conv_transpose2d on the CPU (im2col there is too large at 130 x 130 x 1024),
# the im2col references of conv_generic_cases on a device
# ------------------------------------------------------------------------------------------------
def conv(x, w, stride, pad):
    if x.device.type == "cpu":
        return F.conv2d(x, w, None, stride, pad)
    return cg._fwd(x, w, stride, pad)


def conv_t(dy, w, H, W, stride, pad):
    if dy.device.type == "cpu":
        R_ = w.shape[2]
        P, Q = dy.shape[2:]
        oph, opw = H - ((P - 1) * stride - 2 * pad + R_), W - ((Q - 1) * stride - 2 * pad + R_)
        return F.conv_transpose2d(dy, w, None, stride, pad, (oph, opw))
    return cg._dgrad(dy, w, H, W, stride, pad)


def conv_w(x, dy, R_, stride, pad):
    return cg._wgrad(x, dy, R_, R_, stride, pad)


# ------------------------------------------------------------------------------------------------
# data (CPU float64; the same shape draws the same operand for every direction)
# ------------------------------------------------------------------------------------------------
def _g(field, shape):
    return cg._gen("conv_fast_exact", field, tuple(shape))


def _choice(g, n, values):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), (n,), generator=g)]


def make_data(direction, shape, mode, narrow=None):
    """dict of float64 CPU tensors: x [N][cin][H][W], w [K][cin][R][R], dy [N][K][P][Q], bias [K], g0 / z / y2
    [N][H][W][cin], sc / sh / mu / inv / mu2 / inv2 [max(cin, C1)], mbits uint8 [N H W cin / 8]"""
    N, H, W, C1, C2, K, R_, s = shape
    cin, pad = C1 + C2, R_ // 2
    P, Q = cg.out_hw(H, W, R_, R_, s, pad)
    q = query_class(direction)
    m = dict(x=cg.OPER_MAX, w=cg.OPER_MAX, dy=cg.OPER_MAX)
    m.update(narrow or {})
    n = max(cin, C1)
    d = {}
    if mode == "exact":
        d["x"] = cg._ints(_g(("x", m["x"]), shape), (N, cin, H, W), m["x"])
        d["w"] = cg._ints(_g(("w", m["w"]), shape), (K, cin, R_, R_), m["w"])
        d["dy"] = cg._ints(_g(("dy", m["dy"]), shape), (N, K, P, Q), m["dy"])
        d["bias"] = cg._ints(_g("bias", shape), (K,), cg.OPER_MAX)
        d["sc"], d["sh"] = cg._ints(_g("sc", shape), (n,), cg.OPER_MAX), cg._ints(_g("sh", shape), (n,), cg.OPER_MAX)
    else:
        assert direction in ONEHOT_DIRECTIONS, direction
        g = _g(("onehot", q), shape)
        d["x"], d["dy"] = cg._odd(g, (N, cin, H, W), 8), cg._odd(g, (N, K, P, Q), 8)
        d["bias"] = torch.zeros(K, dtype=F64)
        d["sc"], d["sh"] = torch.ones(n, dtype=F64), torch.zeros(n, dtype=F64)
        if q == "wgrad":
            d["dy"] = cg.onehot_dy(g, N, K, P, Q, 8)
            d["w"] = torch.zeros(K, cin, R_, R_, dtype=F64)
        else:
            d["w"] = cg.onehot_weight(g, K, cin, R_, R_, "c" if q == "dgrad" else "k", 8)
            if q == "fwd" and C2:
                # the source boundary: output channel 1 reads the last channel of x1, channel 2 the first of x2
                for k, c in ((1, C1 - 1), (2, C1)):
                    val = d["w"][k][d["w"][k] != 0]
                    d["w"][k] = 0
                    d["w"][k, c, (R_ - 1) * (k - 1), R_ // 2] = val
    if q == "dgrad":
        d["g0"] = cg._ints(_g("g0", shape), (N, H, W, cin), cg.ACC_MAX)
        d["z"] = cg._ints(_g("z", shape), (N, H, W, cin), cg.OPER_MAX)
        d["y2"] = cg._ints(_g("y2", shape), (N, H, W, cin), cg.OPER_MAX)
        d["mu"], d["inv"] = _choice(_g("mu", shape), n, [-1.0, 0.0, 1.0]), _choice(_g("inv", shape), n, [0.5, 1.0, 2.0])
        d["mu2"], d["inv2"] = _choice(_g("mu2", shape), n, [-1.0, 0.0, 1.0]), _choice(_g("inv2", shape), n, [0.5, 1.0, 2.0])
        d["mbits"] = torch.randint(0, 256, (N * H * W * (cin // 8),), generator=_g("mbits", shape), dtype=torch.uint8)
    return d


def padk_data(K, C1, H, W):
    """x [M][C1], dy [M][64] (columns >= K zero), w [K][C1]: integers in [-3, 3]; x doubles as the old dx"""
    M = PADK_N * H * W
    key = (K, C1, H, W)
    x = cg._ints(_g("padk_x", key), (M, C1), cg.OPER_MAX)
    dy = torch.zeros(M, PADK_KP, dtype=F64)
    dy[:, :K] = cg._ints(_g("padk_dy", key), (M, K), cg.OPER_MAX)
    return dict(x=x, dy=dy, w=cg._ints(_g("padk_w", key), (K, C1), cg.OPER_MAX))


def head_data(head_k):
    return dict(hw=cg._ints(_g("head_w", (head_k,)), (head_k, 64), cg.OPER_MAX),
                hb=cg._ints(_g("head_b", (head_k,)), (head_k,), cg.OPER_MAX))


# ------------------------------------------------------------------------------------------------
# expected results
# ------------------------------------------------------------------------------------------------
def bnrelu_in(x, sc, sh):
    """the BN-ReLU-on-load operand bf16(relu(fma(x, sc, sh))): an exact integer here.  x [N][C][H][W]"""
    C = x.shape[1]
    return bf16_rn(torch.relu(x * sc[:C].view(1, -1, 1, 1) + sh[:C].view(1, -1, 1, 1))).to(F64)


def stats_rows(key, N, P, Q, tile):
    """the output rows in the order the BN partial tiles of configuration `key` take them: tile g holds rows
    [g * tile, (g + 1) * tile) of the result.  The TN tiles and gather rings take consecutive rows (the last tile
    ragged); halo3, first3x3 and the halo-A rings (*_halo, their persistent *_hp) take tile / 32 x 32 spatial
    blocks, dealt row-major over (image, block row, block column)."""
    name = key.split(":")[1]
    rows_ = torch.arange(N * P * Q)
    if name in ("halo3", "first3x3") or name.endswith(("_halo", "_hp")):
        tr = tile // 32
        assert tile % 32 == 0 and P % tr == 0 and Q % 32 == 0, (key, tile, P, Q)
        rows_ = rows_.reshape(N * P // tr, tr, Q // 32, 32).permute(0, 2, 1, 3).reshape(-1)
    return rows_


def tile_sums(y_rows, tile):
    """per-tile column sums [G][K] (float64) of the stored rows [M][K]"""
    return torch.stack([t.to(F64).sum(0) for t in y_rows.split(tile)])


def expect(direction, shape, d, two_round=True):
    """what the call returns, by the names of test_gpu_conv_strided._call: bf16 tensors [M][C] for y / dx, fp32
    [K][cin][R][R] for dw, float64 [nq][cin] for the partials summed over the row tiles (`part`), and `terms`:
    float64 [M][cin] per partial quantity, whose absolute column sums are the budget of that quantity.
    two_round: ACC_RULE of the configuration (acc_two_roundings)."""
    N, H, W, C1, C2, K, R_, s = shape
    cin, pad, M = C1 + C2, R_ // 2, N * H * W
    q = query_class(direction)
    out = {}
    if q in ("fwd", "bnin"):
        x = bnrelu_in(d["x"], d["sc"], d["sh"]) if q == "bnin" else d["x"]
        ref = conv(x, d["w"], s, pad)
        if direction in ("fwd_relu", "fwd_all"):
            ref = torch.relu(ref + d["bias"].view(1, -1, 1, 1))
        out["y"] = bf16_rn(rows(ref))
        return out
    if q == "wgrad":
        x = bnrelu_in(d["x"], d["sc"], d["sh"]) if direction == "wgrad_bnrelu_in" else d["x"]
        ref = conv_w(x, d["dy"], R_, s, pad) + 0.0
        out["dw0"], out["dw1"] = ref.to(torch.float32), (ref + ref).to(torch.float32)
        return out
    ref = rows(conv_t(d["dy"], d["w"], H, W, s, pad))
    r1 = bf16_rn(ref)
    g0 = d["g0"].reshape(M, cin)
    acc = bf16_rn((r1.to(F64) if two_round else ref) + g0)
    if direction == "dgrad":
        out["dx0"], out["dx1"] = r1, acc
        return out
    zero = torch.zeros((), dtype=BF, device=ref.device)
    z = d["z"].reshape(M, cin)
    if direction in ("post1", "post2", "post4"):
        if direction == "post1":
            mask = torch.relu(z) > 0
        elif direction == "post2":
            mask = (z * d["sc"][:cin] + d["sh"][:cin]) > 0
        else:
            mask = unpack_bits(d["mbits"], M, cin)
        dd = torch.where(mask, r1, zero)
        terms = [dd.to(F64)]
        if direction == "post2":
            terms.append(dd.to(F64) * ((z - d["mu"][:cin]) * d["inv"][:cin]))
    else:
        assert two_round, "post 3 has TN kernels only"
        dd = torch.where(unpack_bits(d["mbits"], M, cin), acc, zero)
        terms = [dd.to(F64), dd.to(F64) * ((z - d["mu"][:cin]) * d["inv"][:cin])]
        if direction == "post3_y2":
            terms.append(dd.to(F64) * ((d["y2"].reshape(M, cin) - d["mu2"][:cin]) * d["inv2"][:cin]))
    out["dx"], out["terms"] = dd, terms
    out["part"] = torch.stack([t.sum(0) for t in terms])
    return out


def padk_expect(d, K):
    """-> dw rows [K][C1] fp32 (and twice it), dx0 / dx1 bf16 [M][C1] (1x1 TN kernels: two roundings)"""
    ref = d["dy"][:, :K].t() @ d["x"] + 0.0
    dref = d["dy"][:, :K] @ d["w"]
    r1 = bf16_rn(dref)
    return dict(dw0=ref.to(torch.float32), dw1=(ref + ref).to(torch.float32), dx0=r1, dx1=bf16_rn(r1.to(F64) + d["x"]))


def head_expect(y_rows, hd, N, H, W):
    """logits fp32 [N][head_k][H][W] = head_b + head_w . (stored y)"""
    lg = y_rows.to(F64) @ hd["hw"].t() + hd["hb"]
    return lg.reshape(N, H, W, -1).permute(0, 3, 1, 2).to(torch.float32)


# ------------------------------------------------------------------------------------------------
# the exactness budget, from the data
# ------------------------------------------------------------------------------------------------
def budget(direction, shape, d, ex, tile_rows=None):
    """{quantity: the largest sum of the absolute values of its terms, in units of its quantum (1, or 1/2 where
    the terms are halves)}: per output element the products + |bias| + |g0|; per weight-gradient element over all
    pixels, doubled for the accumulated pass; per channel over all M rows the BN partial sum of the stored y and
    every partial slot of the stored d.  Every figure must be below 2^24."""
    N, H, W, C1, C2, K, R_, s = shape
    cin, pad = C1 + C2, R_ // 2
    q = query_class(direction)
    out = {}
    if q in ("fwd", "bnin"):
        x = bnrelu_in(d["x"], d["sc"], d["sh"]) if q == "bnin" else d["x"]
        mag = conv(x.abs(), d["w"].abs(), s, pad)
        if direction in ("fwd_relu", "fwd_all"):
            mag = mag + d["bias"].abs().view(1, -1, 1, 1)
        out["y"] = float(mag.max())
        if direction != "fwd_relu":
            out["stats"] = float(ex["y"].to(F64).abs().sum(0).max())
    elif q == "wgrad":
        x = bnrelu_in(d["x"], d["sc"], d["sh"]) if direction == "wgrad_bnrelu_in" else d["x"]
        out["dw"] = 2.0 * float(conv_w(x.abs(), d["dy"].abs(), R_, s, pad).max())
    else:
        mag = rows(conv_t(d["dy"].abs(), d["w"].abs(), H, W, s, pad)) + d["g0"].reshape(-1, cin).abs()
        out["dx"] = float(mag.max())
        for i, t in enumerate(ex.get("terms", [])):
            out[f"part{i}"] = (2.0 if i else 1.0) * float(t.abs().sum(0).max())
    return out
