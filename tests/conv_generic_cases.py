"""Cases, data makers and float64 references of the contract tests of the generic conv kernels
(csrc/conv_generic.hip: igemm_tn_kernel<T, BN>, wgrad_kernel<T>, with the split-K reduce of
csrc/conv_wgrad_reduce.hip): tests/test_gpu_conv_generic.py runs them on the GPU, tests/test_conv_generic_cpu.py
checks this file against PyTorch on the CPU.  Nothing here imports the library or touches a GPU.

A case is (N, H, W, C1, C2, K, R, S, stride, pad): x = cat(x1 [C1], x2 [C2]) NHWC, w [K][C1+C2][R][S], one pad
for both axes (the ABI has one), stride 1 or 2, R != S allowed.  References are im2col on F.unfold / F.fold in
float64 and return, next to the value, `mag`: the same contraction over the absolute values of the operands
(+ |bias|, + |dx0| where they enter), the magnitude nhwc_ref.assert_elementwise scales its bound with.

Three data modes, each with its own contract:

  exact   x, w, dy, bias (and the affine scale) are integers in [-3, 3], accumulated-onto tensors integers in
          [-8, 8].  exact_budget() proves every partial sum, in any order, stays below 2^24, so fp32 accumulation
          is exact: an fp32 output equals the integer reference bit for bit, a bf16 output equals bf16_rn(reference)
          (the epilogue adds bias and the old value in fp32 and rounds once), and so do the weight gradients, their
          accumulated second pass and the BN partial sums of the stored output.
  onehot  every output channel's weight has exactly one non-zero (r, s, c) (data gradient: every input channel's
          weight one non-zero (r, s, k); weight gradient: dy non-zero at one pixel per output channel) and the
          operands are odd integers with the top bit of a 12-bit (fp32) / 8-bit (bf16) field set, so every output is
          one exact product whose lowest mantissa bit is set: the gather address of every tap and channel chunk
          is pinned, and an fp32 path that multiplies or accumulates below fp32 precision shows.
  randn   normal operands rounded to the storage type, held element by element with
              k = 2 L + e (fp32: one rounding per product and one per addition at most)
              k = L + e     (bf16: products of bf16 are exact in fp32)
          L = the most products any element of the output sums, e = the bias add / the affine fma / the
          accumulate, whichever the call has (k_rule).
"""
import math
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
STORE = {"fp32": torch.float32, "bf16": torch.bfloat16}
MODES = ("exact", "onehot", "randn")
#: row tile of the generic kernel: its BN partials are per 128 output rows
TILE_M = 128
#: integer ranges of the exact mode
OPER_MAX, ACC_MAX = 3, 8

# ------------------------------------------------------------------------------------------------
# case tables: id -> ((N, H, W, C1, C2, K, R, S, stride, pad), ...)
# ------------------------------------------------------------------------------------------------
#: forward (unetseg_conv2d_fwd): epilogue flags
FWD_CASES = {
    # x1 = buf[..., 0:96], y = buf[..., 96:128] of one buffer with ld 160 (the dense block's layout); M = 400:
    # three row tiles and a 16-row remainder; BN = 64 with a half-empty column tile; bf16 K tail (864 = 13.5 x 64)
    "F_dense_inplace": ((2, 10, 20, 96, 0, 32, 3, 3, 1, 1), dict(stats=True)),
    "F_dense_cat": ((2, 10, 20, 64, 32, 32, 3, 3, 1, 1), dict(stats=True)),  # two sources, different ld
    "F_cin8": ((2, 9, 11, 8, 0, 64, 3, 3, 1, 1), dict(bias=True, relu=True, stats=True)),  # several taps per K step
    "F_ng200": ((1, 9, 8, 40, 0, 200, 3, 3, 1, 1), dict(bias=True, relu=True)),  # BN = 128, second tile 72 columns
    "F_s2": ((2, 16, 14, 32, 0, 40, 3, 3, 2, 1), dict(stats=True)),
    "F_1x1s2_cat": ((2, 9, 9, 24, 8, 16, 1, 1, 2, 0), dict()),
    "F_7x7": ((1, 19, 23, 8, 0, 64, 7, 7, 2, 3), dict()),  # 49 taps
    "F_1x3": ((1, 6, 7, 16, 0, 24, 1, 3, 1, 1), dict()),  # R != S; the output is taller than the input
    "F_valid": ((1, 7, 9, 16, 0, 8, 3, 3, 1, 0), dict(bias=True)),  # pad 0, Ng = 8
}
#: unetseg_conv2d_fwd_affine: id -> (forward case whose shape it takes, relu); exact and randn only
AFFINE_CASES = {"A_dense_cat": ("F_dense_cat", False), "A_s2": ("F_s2", True)}
AFFINE_MODES = ("exact", "randn")

#: data gradient (unetseg_conv2d_dgrad), accumulate 0 then 1 onto dx0; cin = C1, cout = K
DGRAD_CASES = {
    "D_dense": (2, 10, 20, 96, 0, 32, 3, 3, 1, 1),
    "D_s2_odd": (2, 17, 23, 40, 0, 32, 3, 3, 2, 1),  # parity classes with 4 / 2 / 2 / 1 taps; Ng = 40
    "D_1x1s2": (2, 9, 9, 32, 0, 16, 1, 1, 2, 0),  # three classes without taps: zeros / dx0 kept
    "D_uncovered": (1, 8, 10, 16, 0, 32, 3, 3, 2, 0),  # row 7 is reached by no output
    "D_7x7": (1, 19, 23, 8, 0, 32, 7, 7, 2, 3),
    "D_1x3_c20": (1, 6, 7, 20, 0, 24, 1, 3, 1, 1),  # cin = 20: not a multiple of 8, accepted by the ABI
}

#: weight gradient: id -> (shape with N = (fp32 N, bf16 N) where they differ, options)
WGRAD_CASES = {
    "W_dense": ((2, 10, 20, 64, 32, 32, 3, 3, 1, 1), dict(splits={"fp32": 3, "bf16": 1})),
    # 513 K steps -> 64 slabs of 9 steps: slabs 57..63 are empty and must be zeros
    "W_empty_slabs": (((1, 2), 76, 108, 8, 0, 8, 1, 1, 1, 0), dict(splits={"fp32": 64, "bf16": 64})),
    "W_s2_k200": ((2, 17, 23, 40, 0, 200, 3, 3, 2, 1), dict()),  # two Cout tiles, the second with 72 rows
    "W_first_dwc3": ((1, 19, 23, 8, 0, 32, 7, 7, 2, 3), dict(dw_c=3)),  # the padded first conv
    # unetseg_conv2d_wgrad_rows; cout = 64 is fast-eligible in bf16, which runs under UNETSEG_NO_FAST=1
    "W_rows": ((2, 9, 11, 16, 0, 64, 3, 3, 1, 1), dict(dw_rows=21, env={"bf16": {"UNETSEG_NO_FAST": "1"}})),
    "W_1x3": ((1, 6, 7, 16, 0, 24, 1, 3, 1, 1), dict()),
    "W_q3": ((3, 5, 3, 16, 0, 16, 3, 3, 1, 1), dict()),  # Q = 3 is shorter than a K step
}

#: the case of each direction whose strided layout ends every slice at its ld
TAIL_CASES = {"F_valid", "A_s2", "D_uncovered", "W_1x3"}


def case_shape(cid, dtname):
    """(N, H, W, C1, C2, K, R, S, stride, pad) of a case of any table, N resolved for the dtype"""
    if cid in AFFINE_CASES:
        cid = AFFINE_CASES[cid][0]
    shape = FWD_CASES[cid][0] if cid in FWD_CASES else DGRAD_CASES[cid] if cid in DGRAD_CASES else WGRAD_CASES[cid][0]
    if isinstance(shape[0], tuple):
        shape = (shape[0][0 if dtname == "fp32" else 1],) + tuple(shape[1:])
    return shape


def all_shapes():
    """{(id, dtname): shape} of every case of every table"""
    out = {}
    for cid in list(FWD_CASES) + list(DGRAD_CASES) + list(WGRAD_CASES):
        for dtname in STORE:
            out[(cid, dtname)] = case_shape(cid, dtname)
    return out


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


# ------------------------------------------------------------------------------------------------
# float64 references (NCHW / [K][C][R][S], as PyTorch)
# ------------------------------------------------------------------------------------------------
def _fwd(x, w, stride, pad):
    N, _, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = out_hw(H, W, R, S, stride, pad)
    cols = F.unfold(x, (R, S), padding=pad, stride=stride)  # [N][C*R*S][P*Q]
    return (w.reshape(K, -1) @ cols).reshape(N, K, P, Q)


def _dgrad(dy, w, H, W, stride, pad):
    N, K, P, Q = dy.shape
    _, _, R, S = w.shape
    cols = w.reshape(K, -1).t() @ dy.reshape(N, K, P * Q)  # [N][C*R*S][P*Q]
    return F.fold(cols, (H, W), (R, S), padding=pad, stride=stride)


def _wgrad(x, dy, R, S, stride, pad):
    N, K = dy.shape[:2]
    cols = F.unfold(x, (R, S), padding=pad, stride=stride)
    return torch.einsum("nkl,ncl->kc", dy.reshape(N, K, -1), cols).reshape(K, x.shape[1], R, S)


def ref_fwd(x, w, stride, pad, bias=None, escale=None, relu=False):
    """y = [relu](conv(x, w) [* escale] [+ bias]) -> (y, mag) [N][K][P][Q]"""
    x, w = x.to(F64), w.to(F64)
    y, mag = _fwd(x, w, stride, pad), _fwd(x.abs(), w.abs(), stride, pad)
    if escale is not None:
        e = escale.to(F64).view(1, -1, 1, 1)
        y, mag = y * e, mag * e.abs()
    if bias is not None:
        b = bias.to(F64).view(1, -1, 1, 1)
        y, mag = y + b, mag + b.abs()
    return (y.clamp_min(0.0) if relu else y), mag


def ref_dgrad(dy, w, H, W, stride, pad, dx0=None):
    """dx = conv_transpose(dy, w) (+ dx0) -> (dx, mag) [N][C][H][W]"""
    dy, w = dy.to(F64), w.to(F64)
    dx, mag = _dgrad(dy, w, H, W, stride, pad), _dgrad(dy.abs(), w.abs(), H, W, stride, pad)
    if dx0 is not None:
        dx, mag = dx + dx0.to(F64), mag + dx0.to(F64).abs()
    return dx, mag


def ref_wgrad(x, dy, R, S, stride, pad):
    """dw[k][c][r][s] = sum over the output pixels of dy * the tap's x -> (dw, mag) [K][C][R][S]"""
    x, dy = x.to(F64), dy.to(F64)
    return _wgrad(x, dy, R, S, stride, pad), _wgrad(x.abs(), dy.abs(), R, S, stride, pad)


def products(direction, shape):
    """float64 tensor shaped like the direction's output: the number of products each element sums (the
    contraction over operands of ones: taps outside the image and parity classes without taps do not count)"""
    N, H, W, C1, C2, K, R, S, stride, pad = shape
    C = C1 + C2
    P, Q = out_hw(H, W, R, S, stride, pad)
    x, w, dy = torch.ones(N, C, H, W, dtype=F64), torch.ones(K, C, R, S, dtype=F64), torch.ones(N, K, P, Q, dtype=F64)
    if direction == "fwd":
        return _fwd(x, w, stride, pad)
    if direction == "dgrad":
        return _dgrad(dy, w, H, W, stride, pad)
    return _wgrad(x, dy, R, S, stride, pad)


def max_products(direction, shape):
    """L of the k rule: the most products any element sums"""
    return int(products(direction, shape).max())


def k_rule(dtname, L, e):
    """roundings on the longest path of an element that sums L products and then makes e more fp32 operations
    (the bias add, the affine fma, the accumulate).  fp32: every product and every addition may round -> 2 L + e;
    bf16: the product of two bf16 values is exact in fp32, only the additions round -> L + e."""
    return (2 * L if dtname == "fp32" else L) + e


def exact_budget(direction, shape, bias=False, affine=False, accumulate=False):
    """Largest possible |partial sum| of the exact mode, from the integer ranges alone: L products of two
    operands in [-OPER_MAX, OPER_MAX] (times an affine scale in the same range), a bias in that range, an
    accumulated-onto value in [-ACC_MAX, ACC_MAX]; a weight gradient's second pass doubles it.  `stats` is the bound
    of a BN partial sum: TILE_M rows of the stored output.  Every figure must stay below 2^24 for fp32 addition
    to be exact in any order."""
    L = max_products(direction, shape)
    part = OPER_MAX * OPER_MAX * L
    if affine:
        part *= OPER_MAX
    if bias or affine:
        part += OPER_MAX
    if direction == "dgrad" and accumulate:
        part += ACC_MAX
    if direction == "wgrad" and accumulate:
        part *= 2
    return dict(L=L, partial=part, stats=TILE_M * part if direction == "fwd" else 0)


# ------------------------------------------------------------------------------------------------
# data makers (CPU, float64 values that the storage type holds exactly)
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, m):
    return torch.randint(-m, m + 1, shape, generator=g).to(F64)


def _odd(g, shape, bits):
    """odd integers of either sign with the top bit of a `bits`-bit field set: |v| in [2^(bits-1) + 1, 2^bits - 1]"""
    v = 2 ** (bits - 1) + 2 * torch.randint(0, 2 ** (bits - 2), shape, generator=g) + 1
    return (v * (2 * torch.randint(0, 2, shape, generator=g) - 1)).to(F64)


def _normal(g, shape, dtname, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(STORE[dtname]).to(F64)


def spread(n_out, n_pos):
    """one position in [0, n_pos) per output: an even spread with a varying offset inside each stratum; the
    first output takes position 0 and the last one n_pos - 1 (the K tail)"""
    step = max(1, n_pos // n_out)
    pos = [min(n_pos - 1, (k * n_pos) // n_out + (5 * k) % step) for k in range(n_out)]
    pos[0], pos[-1] = 0, n_pos - 1
    return pos


def onehot_weight(g, K, C, R, S, per, bits):
    """w [K][C][R][S] with one non-zero per output channel k at a flat (r, s, c) position (per == "k": the
    forward GEMM's K axis order) or one per input channel c at a flat (r, s, k) position (per == "c": the data
    gradient's)"""
    w = torch.zeros(K, C, R, S, dtype=F64)
    n_out, n_in = (K, C) if per == "k" else (C, K)
    vals = _odd(g, (n_out,), bits)
    for o, pos in enumerate(spread(n_out, R * S * n_in)):
        r, s, i = pos // (S * n_in), (pos // n_in) % S, pos % n_in
        if per == "k":
            w[o, i, r, s] = vals[o]
        else:
            w[i, o, r, s] = vals[o]
    return w


def onehot_dy(g, N, K, P, Q, bits):
    """dy [N][K][P][Q] non-zero at one output pixel per channel"""
    dy = torch.zeros(N, K, P, Q, dtype=F64)
    vals = _odd(g, (K,), bits)
    for k, pos in enumerate(spread(K, N * P * Q)):
        dy[pos // (P * Q), k, (pos // Q) % P, pos % Q] = vals[k]
    return dy


def make_data(cid, direction, shape, dtname, mode, bias=False, affine=False):
    """dict of float64 CPU tensors the storage type holds exactly: x [N][C][H][W], w [K][C][R][S], dy [N][K][P][Q],
    dx0 [N][C][H][W]; bias / escale [K] (fp32 values) or None.  The one-hot mode takes no bias."""
    N, H, W, C1, C2, K, R, S, stride, pad = shape
    C = C1 + C2
    P, Q = out_hw(H, W, R, S, stride, pad)
    g = _gen(cid, direction, dtname, mode)
    d = dict(bias=None, escale=None)
    if mode == "exact":
        d["x"], d["w"] = _ints(g, (N, C, H, W), OPER_MAX), _ints(g, (K, C, R, S), OPER_MAX)
        d["dy"], d["dx0"] = _ints(g, (N, K, P, Q), OPER_MAX), _ints(g, (N, C, H, W), ACC_MAX)
        if bias or affine:
            d["bias"] = _ints(g, (K,), OPER_MAX)
        if affine:
            d["escale"] = _ints(g, (K,), OPER_MAX)
    elif mode == "onehot":
        bits = 12 if dtname == "fp32" else 8
        d["x"], d["dy"] = _odd(g, (N, C, H, W), bits), _odd(g, (N, K, P, Q), bits)
        d["dx0"] = _ints(g, (N, C, H, W), ACC_MAX)
        if direction == "wgrad":
            d["dy"] = onehot_dy(g, N, K, P, Q, bits)
            d["w"] = torch.zeros(K, C, R, S, dtype=F64)
        else:
            d["w"] = onehot_weight(g, K, C, R, S, "k" if direction == "fwd" else "c", bits)
    else:
        d["x"], d["dy"] = _normal(g, (N, C, H, W), dtname), _normal(g, (N, K, P, Q), dtname)
        d["w"] = _normal(g, (K, C, R, S), dtname, 1.0 / math.sqrt(C * R * S))
        d["dx0"] = _normal(g, (N, C, H, W), dtname)
        if bias or affine:
            d["bias"] = _normal(g, (K,), "fp32", 0.1)
        if affine:
            d["escale"] = 1.0 + _normal(g, (K,), "fp32", 0.3)
    return d


# ------------------------------------------------------------------------------------------------
# layouts and the split rule
# ------------------------------------------------------------------------------------------------
def layout(chs, tail):
    """[(ld, c0)] per tensor of `chs` channels: ld and c0 multiples of 8, every ld and every c0 different,
    c0 > 0; tail: the slice ends at ld where the channel count allows (C % 8 == 0), else channels follow it"""
    out, lds, c0s = [], set(), set()
    for i, C in enumerate(chs):
        pre, post = 8 * (i + 1), 0 if tail and C % 8 == 0 else 8 * (i + 2)
        ld = -(-(C + pre + post) // 8) * 8
        while ld in lds or pre in c0s:
            pre, ld = pre + 8, ld + 8
        lds.add(ld)
        c0s.add(pre)
        out.append((ld, pre))
    return out


def packed_layout(chs):
    return [(C, 0) for C in chs]


def operand_channels(direction, shape):
    """channels of the activation operands in the order the layouts are dealt: forward and weight gradient
    x1 [, x2], y / dy; data gradient dy, dx"""
    N, H, W, C1, C2, K = shape[:6]
    if direction == "dgrad":
        return [K, C1 + C2]
    return [C1] + ([C2] if C2 else []) + [K]


def generic_splits(dtname, cout, Ng, kpix):
    """split-K slabs of the generic weight gradient (wgrad_generic_splits, csrc/conv_generic.hip): enough
    128 x 128 tiles x slabs for 768 blocks, at least 8 K steps (32 pixels in bf16, 16 in fp32) per slab, at
    most 64"""
    bk = 32 if dtname == "bf16" else 16
    tiles = -(-cout // 128) * -(-Ng // 128)
    nkt = -(-kpix // bk)
    return max(1, min(-(-768 // tiles), max(1, nkt // 8), 64))
