"""GPU: the channel-slice contract of the conv C ABI, per kernel configuration.

Every activation operand of a conv entry point has a pixel stride (ldc1 / ldc2, ldy, ldx, the stride of aux /
y1 / y2): the op layer hands the kernels channel slices of concat buffers.  Each case below makes the same call
twice with the same values:

  packed   ld == channels, pointer at channel 0 -- what tests/test_gpu_configs.py drives -- checked against the
           float64 im2col references of that file at its tolerances (bf16 outputs
           2^-8 |ref| + 1e-4 max|ref|, dw 1e-3 |ref| + 2e-5 max|ref|, partials 1e-4 after merging);
  strided  every activation operand is the slice [..., c0:c0+C] of its own wider buffer (a different ld and a
           different non-zero c0 per tensor, multiples of 8 elements; `tail` cases end the slice at ld), with
           GUARD sentinel pixels before the first and after the last pixel inside the same allocation.  Inputs
           and accumulated outputs carry the finite SENTINEL outside the slice, written outputs NaN.

and asserts that
  * the host-only configuration queries name the same configuration for both and the one the case lists;
  * inside the slice the strided result equals the packed one bit for bit (strides change addresses, not
    arithmetic; the split-K reduce order is deterministic);
  * every foreign channel and guard pixel of every buffer, inputs included, still holds its fill bit for bit.

tests/test_conv_strided_cover_cpu.py proves on the CPU that the cases reach every configuration key the cases
of tests/test_gpu_configs.py reach (PACKED_ONLY is the explicit list of exceptions: empty).  Every test prints
one `strided-case` line: configuration, row tiles, the largest packed-vs-float64 error over its bound, seconds.
"""
import math
import os
import re
import time

import pytest
import torch

import test_gpu_configs as tgc
from nhwc_ref import NAN, SENTINEL, assert_elementwise, assert_guard, assert_tail, sliced
from test_gpu_configs import _bf, _check_bf16, _nchw, _nhwc, _Op, _out_hw, _P, _ref_dgrad, _ref_fwd, _ref_wgrad, _st

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
#: sentinel pixels before and after every strided operand: two 256-row tiles (the largest row tile, and more
#: than the W + 1 pixels a 3x3 tap of the first / last row reaches past the tensor at the widths used here)
GUARD = 512


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unetseg_hip import load
    load()


# ------------------------------------------------------------------------------------------------
# layouts and host-only configuration queries (shared with the CPU coverage test)
# ------------------------------------------------------------------------------------------------
def layout(chs, tail):
    """[(ld, c0)] per tensor of `chs` channels: multiples of 8, every ld and every c0 different, c0 > 0;
    tail: the slice ends at ld (c0 + C == ld), else channels follow it too"""
    out, lds, c0s = [], set(), set()
    for i, C in enumerate(chs):
        pre, post = 8 * (i + 1), 0 if tail else 8 * (i + 2)
        while C + pre + post in lds or pre in c0s:
            pre += 8
        lds.add(C + pre + post)
        c0s.add(pre)
        out.append((C + pre + post, pre))
    return out


def packed_layout(chs):
    return [(C, 0) for C in chs]


#: direction -> (prefix of its configuration keys, the query it is asked through)
_QUERY = {"fwd_relu": ("fwd", "fwd"), "fwd_stats": ("fwd", "fwd"), "fwd_all": ("fwd", "fwd"),
          "dgrad": ("dgrad", "dgrad"), "post1": ("dgrad_post1", "dgrad"), "post2": ("dgrad_post2", "dgrad"),
          "post3": ("dgrad_post3", "dgrad"), "post3_y2": ("dgrad_post3", "dgrad"), "post4": ("dgrad_post4", "dgrad"),
          "wgrad": ("wgrad", "wgrad"), "fwd_bnrelu_in": ("fwd_bnrelu_in", "bnin"),
          "wgrad_bnrelu_in": ("wgrad_bnrelu_in", "wgrad")}


def operand_channels(direction, shape):
    """channels of the activation operands of a call, in the order the layouts are dealt"""
    N, H, W, C1, C2, K, R, s = shape
    cin = C1 + C2
    q = _QUERY[direction][1]
    if q == "dgrad":
        extra = {"post1": [cin], "post2": [cin], "post3": [cin], "post3_y2": [cin, cin]}.get(direction, [])
        return [K, cin] + extra  # dy, dx, aux / y1, y2
    return [C1] + ([C2] if C2 else []) + [K]  # x1, x2, y / dy


def case_keys(direction, shape, lay):
    """configuration keys of a call whose operands have the (ld, c0) of `lay` (host-only queries)"""
    from unetseg_hip import lib
    from unetseg_hip.lib import DT_BF16
    N, H, W, C1, C2, K, R, s = shape
    pad, cin = R // 2, C1 + C2
    P, Q = _out_hw(H, W, R, s)
    pfx, q = _QUERY[direction]
    if q == "fwd":
        return [f"{pfx}:" + lib.fwd_config(DT_BF16, C1, lay[0][0], C2, lay[1][0] if C2 else 0, N, H, W, K, R, R, s, pad)]
    if q == "dgrad":
        return [f"{pfx}:{c}" for c in lib.dgrad_config(DT_BF16, lay[0][0], N, P, Q, K, cin, R, R, s, pad, lay[1][0], H, W)]
    if q == "bnin":
        cfg = lib.load().unetseg_conv2d_fwd_bnrelu_in_config(DT_BF16, C1, lay[0][0], N, H, W, K)
        return [f"{pfx}:" + lib.CFG_NAMES.get(cfg, str(cfg))]
    kern = lib.wgrad_config(DT_BF16, C1, lay[0][0], C2, lay[1][0] if C2 else 0, N, H, W, lay[-1][0], K, R, R, s, pad)[0]
    return [f"{pfx}:{kern}"]


def row_tiles(key, direction, shape):
    """row tiles of the launch: output rows over the configuration's row tile (8 x 32 pixels on the halo
    kernels); for a weight gradient the 32-pixel K steps of its reduction"""
    N, H, W, C1, C2, K, R, s = shape
    P, Q = _out_hw(H, W, R, s)
    name = key.split(":")[1]
    if _QUERY[direction][1] == "wgrad":
        return -(-N * P * Q // 32)
    M = N * -(-H // s) * -(-W // s) if _QUERY[direction][1] == "dgrad" else N * P * Q
    m = re.search(r"(\d+)x\d+", name)
    bm = int(m.group(1)) if m else 256  # halo3, first3x3: 256-pixel tiles; generic: 128
    return -(-M // (128 if name == "generic" else bm))


PLAIN = {"UNETSEG_TN_PERSIST": "0"}
PERSIST3 = {"UNETSEG_TN_PERSIST_T": "3"}
HS0, HS1 = {"UNETSEG_HALO_HS": "0"}, {"UNETSEG_HALO_HS": "1"}

# id: (direction, (N, H, W, C1, C2, K, R, stride), configuration keys the queries must name, environment, tail)
# The shapes are the smallest of a grid over (N, H, W, C1, C2, K, R, stride) that select the configuration with
# the padded strides of `layout`, preferring two or more row tiles with a partial last one: 10 x 20 = 200 rows
# (128 + 72), 9 x 8 = 72 rows (64 + 8), 130 x 130 = 16900 rows where a configuration needs >= 256 tiles; the
# halo kernels only take whole 8 x 32 tiles (16 x 32: two of them; 128 x 128 where the tile count selects).
STRIDED_CASES = {
    # ---- forward: bias + ReLU / BN partials / both; one and two sources (ldc1 != ldc2) ----
    "fwd_halo3_relu": ("fwd_relu", (1, 16, 32, 64, 0, 64, 3, 1), ["fwd:halo3"], HS0, False),
    "fwd_halo3_stats_hs": ("fwd_stats", (1, 16, 32, 64, 0, 64, 3, 1), ["fwd:halo3"], HS1, True),
    "fwd_halo3_relu_hs": ("fwd_relu", (3, 16, 64, 64, 0, 64, 3, 1), ["fwd:halo3"], HS1, False),
    "fwd_halo3_k128": ("fwd_all", (3, 16, 64, 64, 0, 128, 3, 1), ["fwd:halo3"], HS0, False),
    "fwd_tn128x64_1st": ("fwd_all", (1, 10, 20, 64, 0, 64, 1, 1), ["fwd:tn128x64_1st"], {}, False),
    "fwd_tn128x128_1step": ("fwd_stats", (1, 10, 20, 64, 0, 128, 1, 1), ["fwd:tn128x128_1step"], {}, True),
    "fwd_tn128x128_1st": ("fwd_all", (1, 10, 20, 64, 64, 128, 1, 1), ["fwd:tn128x128_1st"], {}, False),
    "fwd_tn128x64": ("fwd_stats", (1, 10, 20, 256, 64, 64, 1, 1), ["fwd:tn128x64"], {}, False),
    "fwd_tn64x128": ("fwd_all", (1, 9, 8, 256, 64, 128, 1, 1), ["fwd:tn64x128"], {}, False),
    "fwd_tn128x128": ("fwd_all", (1, 130, 130, 256, 64, 192, 1, 1), ["fwd:tn128x128"], {}, False),
    "fwd_ring128x64_t9": ("fwd_relu", (1, 10, 20, 64, 64, 64, 3, 1), ["fwd:ring128x64_t9"], {}, False),
    "fwd_ring64x128_t9": ("fwd_stats", (1, 9, 8, 192, 64, 128, 3, 1), ["fwd:ring64x128_t9"], {}, False),
    "fwd_ring64x128_t1": ("fwd_stats", (1, 9, 8, 2048, 0, 128, 1, 1), ["fwd:ring64x128_t1"], {}, True),
    "fwd_ring64x128_5x5": ("fwd_all", (1, 9, 8, 64, 64, 128, 5, 1), ["fwd:ring64x128"], {}, False),
    "fwd_ring256x128_t1": ("fwd_stats", (1, 130, 130, 256, 64, 512, 1, 1), ["fwd:ring256x128_t1"], {}, False),
    "fwd_ring256x128_t9": ("fwd_all", (1, 130, 130, 64, 0, 512, 3, 1), ["fwd:ring256x128_t9"], {}, False),
    "fwd_ring128x128_5st_t1": ("fwd_stats", (1, 130, 130, 1024, 0, 192, 1, 1), ["fwd:ring128x128_5st_t1"], {}, False),
    "fwd_ring128x128_5st_t9": ("fwd_all", (1, 130, 130, 64, 64, 192, 3, 1), ["fwd:ring128x128_5st_t9"], {}, False),
    "fwd_ring128x128_halo": ("fwd_stats", (1, 128, 128, 64, 64, 192, 3, 1), ["fwd:ring128x128_halo"], PLAIN, False),
    "fwd_ring128x128_halo_p3": ("fwd_all", (1, 128, 128, 64, 64, 192, 3, 1), ["fwd:ring128x128_halo"], PERSIST3, True),
    "fwd_ring256x128_halo": ("fwd_all", (2, 128, 128, 64, 64, 192, 3, 1), ["fwd:ring256x128_halo"], PLAIN, False),
    "fwd_ring256x128_hp": ("fwd_all", (2, 128, 128, 64, 64, 192, 3, 1), ["fwd:ring256x128_hp"], PERSIST3, False),
    "fwd_ring256x64_halo": ("fwd_all", (1, 16, 64, 64, 64, 64, 3, 1), ["fwd:ring256x64_halo"], PLAIN, False),
    "fwd_ring256x64_hp": ("fwd_stats", (1, 40, 32, 64, 64, 64, 3, 1), ["fwd:ring256x64_hp"], PERSIST3, False),
    # the generic kernel: an 8-channel source whose stride is not the packed image's
    "fwd_generic_cin8": ("fwd_stats", (1, 9, 11, 8, 0, 64, 3, 1), ["fwd:generic"], {}, False),
    # ---- 1x1 conv reading BN-ReLU on load ----
    "bnin_tn128x128_1step": ("fwd_bnrelu_in", (1, 10, 20, 64, 0, 128, 1, 1), ["fwd_bnrelu_in:tn128x128_1step"], {}, False),
    "bnin_tn128x128_1st": ("fwd_bnrelu_in", (1, 10, 20, 128, 0, 128, 1, 1), ["fwd_bnrelu_in:tn128x128_1st"], {}, True),
    "bnin_tn64x128": ("fwd_bnrelu_in", (1, 9, 8, 320, 0, 128, 1, 1), ["fwd_bnrelu_in:tn64x128"], {}, False),
    "bnin_tn128x128": ("fwd_bnrelu_in", (1, 130, 130, 320, 0, 192, 1, 1), ["fwd_bnrelu_in:tn128x128"], {}, False),
    "bnin_tn256x128": ("fwd_bnrelu_in", (1, 130, 130, 320, 0, 512, 1, 1), ["fwd_bnrelu_in:tn256x128"], {}, False),
    # ---- data gradient: plain, then accumulated; stride 2 = the four parity classes; cin = C1 + C2 ----
    "dgrad_halo3": ("dgrad", (1, 16, 32, 64, 0, 64, 3, 1), ["dgrad:halo3"], HS0, False),
    "dgrad_halo3_hs": ("dgrad", (3, 16, 64, 64, 0, 64, 3, 1), ["dgrad:halo3"], HS1, True),
    "dgrad_tn128x64_1st": ("dgrad", (1, 10, 20, 64, 0, 64, 1, 1), ["dgrad:tn128x64_1st"], {}, False),
    "dgrad_tn128x128_1step": ("dgrad", (1, 10, 20, 128, 0, 64, 1, 1), ["dgrad:tn128x128_1step"], {}, True),
    "dgrad_tn128x128_1st_cat": ("dgrad", (1, 10, 20, 64, 64, 128, 1, 1), ["dgrad:tn128x128_1st"], {}, False),
    "dgrad_tn128x64": ("dgrad", (1, 10, 20, 64, 0, 320, 1, 1), ["dgrad:tn128x64"], {}, False),
    "dgrad_tn64x128": ("dgrad", (1, 9, 8, 128, 0, 320, 1, 1), ["dgrad:tn64x128"], {}, False),
    "dgrad_tn128x128": ("dgrad", (1, 130, 130, 192, 0, 320, 1, 1), ["dgrad:tn128x128"], {}, False),
    "dgrad_ring128x64_t9": ("dgrad", (1, 10, 20, 64, 0, 128, 3, 1), ["dgrad:ring128x64_t9"], {}, False),
    "dgrad_ring64x128_t9": ("dgrad", (1, 9, 8, 128, 0, 256, 3, 1), ["dgrad:ring64x128_t9"], {}, False),
    "dgrad_ring64x128_t1": ("dgrad", (1, 9, 8, 128, 0, 2048, 1, 1), ["dgrad:ring64x128_t1"], {}, False),
    "dgrad_ring64x128_5x5": ("dgrad", (1, 9, 8, 128, 0, 128, 5, 1), ["dgrad:ring64x128"], {}, False),
    "dgrad_ring256x128_t1": ("dgrad", (1, 130, 130, 512, 0, 320, 1, 1), ["dgrad:ring256x128_t1"], {}, False),
    "dgrad_ring256x128_t9": ("dgrad", (1, 130, 130, 512, 0, 64, 3, 1), ["dgrad:ring256x128_t9"], {}, False),
    "dgrad_ring128x128_5st_t1": ("dgrad", (1, 130, 130, 192, 0, 1024, 1, 1), ["dgrad:ring128x128_5st_t1"], {}, False),
    "dgrad_ring128x128_5st_t9": ("dgrad", (1, 130, 130, 192, 0, 128, 3, 1), ["dgrad:ring128x128_5st_t9"], {}, False),
    "dgrad_ring128x128_halo": ("dgrad", (1, 128, 128, 128, 64, 128, 3, 1), ["dgrad:ring128x128_halo"], PLAIN, False),
    "dgrad_ring256x128_halo": ("dgrad", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad:ring256x128_halo"], PLAIN, False),
    "dgrad_ring256x128_hp": ("dgrad", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad:ring256x128_hp"], PERSIST3, False),
    "dgrad_ring256x64_halo": ("dgrad", (1, 16, 64, 64, 0, 128, 3, 1), ["dgrad:ring256x64_halo"], PLAIN, False),
    "dgrad_ring256x64_hp": ("dgrad", (1, 40, 32, 64, 0, 128, 3, 1), ["dgrad:ring256x64_hp"], PERSIST3, False),
    "dgrad_multi128x128_s2": ("dgrad", (1, 24, 24, 64, 64, 64, 3, 2), ["dgrad:multi128x128"] * 4, {}, False),
    "dgrad_multi64x128_s2": ("dgrad", (1, 15, 17, 128, 0, 128, 3, 2), ["dgrad:multi64x128"] * 4, {}, True),
    # ---- data gradient with the producer's ReLU (post 1) / BN-ReLU (post 2) backward: ldy, ldx, ld_aux differ ----
    "post1_halo3": ("post1", (1, 16, 32, 64, 0, 64, 3, 1), ["dgrad_post1:halo3"], HS0, False),
    "post1_halo3_hs": ("post1", (3, 16, 64, 64, 0, 64, 3, 1), ["dgrad_post1:halo3"], HS1, False),
    "post2_halo3": ("post2", (3, 16, 64, 64, 0, 64, 3, 1), ["dgrad_post2:halo3"], HS0, True),
    "post2_halo3_hs": ("post2", (1, 16, 32, 64, 0, 64, 3, 1), ["dgrad_post2:halo3"], HS1, False),
    "post4_halo3": ("post4", (3, 16, 64, 64, 0, 64, 3, 1), ["dgrad_post4:halo3"], HS0, False),
    "post4_halo3_hs": ("post4", (1, 16, 32, 64, 0, 64, 3, 1), ["dgrad_post4:halo3"], HS1, True),
    "post1_ring256x128_t9": ("post1", (1, 130, 130, 512, 0, 64, 3, 1), ["dgrad_post1:ring256x128_t9"], {}, False),
    "post1_ring128x128_5st_t9": ("post1", (1, 130, 130, 192, 0, 128, 3, 1), ["dgrad_post1:ring128x128_5st_t9"], {}, True),
    "post1_ring128x128_halo": ("post1", (1, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post1:ring128x128_halo"], PLAIN, False),
    "post1_ring256x128_halo": ("post1", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post1:ring256x128_halo"], PLAIN, False),
    "post1_ring256x128_hp": ("post1", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post1:ring256x128_hp"], PERSIST3, False),
    "post1_ring256x64_halo": ("post1", (1, 16, 64, 64, 0, 128, 3, 1), ["dgrad_post1:ring256x64_halo"], PLAIN, False),
    "post1_ring256x64_hp": ("post1", (1, 40, 32, 64, 0, 128, 3, 1), ["dgrad_post1:ring256x64_hp"], PERSIST3, False),
    "post2_tn128x64_1st": ("post2", (1, 10, 20, 64, 0, 64, 1, 1), ["dgrad_post2:tn128x64_1st"], {}, False),
    "post2_tn128x128_1st": ("post2", (1, 10, 20, 128, 0, 128, 1, 1), ["dgrad_post2:tn128x128_1st"], {}, False),
    "post2_tn128x64": ("post2", (1, 10, 20, 64, 0, 320, 1, 1), ["dgrad_post2:tn128x64"], {}, False),
    "post2_tn64x128": ("post2", (1, 9, 8, 128, 0, 320, 1, 1), ["dgrad_post2:tn64x128"], {}, True),
    "post2_tn128x128": ("post2", (1, 130, 130, 192, 0, 320, 1, 1), ["dgrad_post2:tn128x128"], {}, False),
    "post2_ring64x128_t9": ("post2", (1, 9, 8, 128, 0, 256, 3, 1), ["dgrad_post2:ring64x128_t9"], {}, False),
    "post2_ring64x128_t1": ("post2", (1, 9, 8, 128, 0, 2048, 1, 1), ["dgrad_post2:ring64x128_t1"], {}, False),
    "post2_ring256x128_t1": ("post2", (1, 130, 130, 512, 0, 320, 1, 1), ["dgrad_post2:ring256x128_t1"], {}, False),
    "post2_ring256x128_t9": ("post2", (1, 130, 130, 512, 0, 64, 3, 1), ["dgrad_post2:ring256x128_t9"], {}, False),
    "post2_ring128x128_5st_t1": ("post2", (1, 130, 130, 192, 0, 1024, 1, 1), ["dgrad_post2:ring128x128_5st_t1"], {}, False),
    "post2_ring128x128_5st_t9": ("post2", (1, 130, 130, 192, 0, 128, 3, 1), ["dgrad_post2:ring128x128_5st_t9"], {}, False),
    "post2_ring128x128_halo": ("post2", (1, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post2:ring128x128_halo"], PLAIN, False),
    "post2_ring256x128_halo": ("post2", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post2:ring256x128_halo"], PLAIN, False),
    "post2_ring256x128_hp": ("post2", (2, 128, 128, 192, 0, 128, 3, 1), ["dgrad_post2:ring256x128_hp"], PERSIST3, False),
    "post2_multi128x128_s2": ("post2", (1, 24, 24, 64, 0, 64, 3, 2), ["dgrad_post2:multi128x128"] * 4, {}, False),
    "post2_multi64x128_s2": ("post2", (1, 15, 17, 128, 0, 128, 3, 2), ["dgrad_post2:multi64x128"] * 4, {}, False),
    # ---- residual post-op (post 3; shape = (N, H, W, C, 0, K, 1, 1) of test_gpu_post_res.py's (N, H, W, K, C)):
    #      ldy, ldx, ld(y1) and ld(y2) all differ ----
    "post3_ragged": ("post3", (1, 15, 17, 256, 0, 64, 1, 1), ["dgrad_post3:tn128x128_1step"], {}, False),
    # fewer than 65 rows in the only tile (its second row-wave is empty), with the downsample branch
    "post3_5x5_y2": ("post3_y2", (1, 5, 5, 256, 0, 64, 1, 1), ["dgrad_post3:tn128x128_1step"], {}, False),
    "post3_tn128x128_1st_y2": ("post3_y2", (1, 10, 20, 128, 0, 128, 1, 1), ["dgrad_post3:tn128x128_1st"], {}, True),
    "post3_ring256x128_t1": ("post3", (1, 130, 130, 512, 0, 320, 1, 1), ["dgrad_post3:ring256x128_t1"], {}, False),
    # ---- weight gradient (accumulate 0, then 1) ----
    "wgrad_halo3": ("wgrad", (1, 16, 32, 64, 0, 64, 3, 1), ["wgrad:halo3_wgrad"], {}, False),
    "wgrad_halo3_cat": ("wgrad", (3, 16, 64, 64, 64, 128, 3, 1), ["wgrad:halo3_wgrad"], {}, True),
    "wgrad128_ragged": ("wgrad", (1, 10, 20, 64, 0, 128, 1, 1), ["wgrad:wgrad128"], {}, False),
    "wgrad128_ragged_3x3": ("wgrad", (2, 15, 17, 64, 64, 128, 3, 1), ["wgrad:wgrad128"], {}, False),
    "wgrad64x256_ragged": ("wgrad", (1, 15, 17, 256, 0, 64, 1, 1), ["wgrad:wgrad64x256"], {}, False),
    "wgrad128_row_cat": ("wgrad", (1, 8, 32, 64, 64, 192, 1, 1), ["wgrad:wgrad128_row"], {}, False),
    "wgrad64x256_row_cat": ("wgrad", (1, 8, 32, 64, 64, 64, 1, 1), ["wgrad:wgrad64x256_row"], {}, False),
    "wgrad_ring128": ("wgrad", (3, 8, 32, 64, 0, 128, 1, 1), ["wgrad:wgrad_ring128"], {}, True),
    "wgrad_ring128_3x3s2": ("wgrad", (3, 8, 32, 64, 0, 128, 3, 2), ["wgrad:wgrad_ring128"], {}, False),
    "wgrad_ring64x256": ("wgrad", (1, 16, 32, 128, 0, 64, 1, 1), ["wgrad:wgrad_ring64x256"], {}, False),
    "bnin_wgrad128": ("wgrad_bnrelu_in", (1, 10, 20, 64, 0, 128, 1, 1), ["wgrad_bnrelu_in:wgrad128"], {}, False),
    "bnin_wgrad_ring128": ("wgrad_bnrelu_in", (3, 8, 32, 64, 0, 128, 1, 1), ["wgrad_bnrelu_in:wgrad_ring128"], {}, True),
    "bnin_wgrad_ring64x256": ("wgrad_bnrelu_in", (1, 16, 32, 128, 0, 64, 1, 1), ["wgrad_bnrelu_in:wgrad_ring64x256"], {}, False),
}

#: configurations no stride other than the packed one reaches, with the dispatch condition that excludes them.
#: Empty: no dispatch rule of csrc/conv.hip, conv_fast.hip, conv_wgrad_fast.hip tests a pixel stride except through
#: the 2^31-byte extents (and the gather rings' 32-bit offset range, tn_taps), which a few padding channels do not
#: move at these sizes.  fwd:first3x3 admits a wide ldy but requires ldc1 == 8 (conv_first.hip first3x3_ok): its
#: strided cases (test_first3x3_strided) keep the packed image and slice the output only.
PACKED_ONLY = set()

#: keys of the special-entry-point tests below (the stem through unetseg_stem_config, first3x3 through fwd_config)
STEM_CASES = [(2, 64, False, "stem_halo"), (2, 64, True, "tn128x64"), (1, 200, False, "tn128x64")]
FIRST3X3_CASES = [("fwd_stats", (1, 32, 64, 8, 0, 64, 3, 1)), ("fwd_relu", (2, 32, 32, 8, 0, 64, 3, 1))]


def strided_keys():
    """every configuration key the strided cases reach, by the host-only queries alone"""
    from unetseg_hip import introspect
    from unetseg_hip.lib import DT_BF16, fwd_config, stem_config
    keys = set()
    for direction, shape, _, env, tail in STRIDED_CASES.values():
        with _environ(env):
            keys.update(case_keys(direction, shape, layout(operand_channels(direction, shape), tail)))
    for N, H, tn, _ in STEM_CASES:
        with _environ({"UNETSEG_STEM_TN": "1"} if tn else {}):
            keys.add("stem_fwd:" + stem_config(N, H, H, 64)[0])
            keys.add(introspect.call_configs(("stem_wgrad", N, H, H, 3, 0, 64, 7, 7, 2, 3, 8, 0))[0])
    for _, (N, H, W, C1, C2, K, R, s) in FIRST3X3_CASES:
        keys.add("fwd:" + fwd_config(DT_BF16, C1, 8, 0, 0, N, H, W, K, R, R, s, 1))
    return keys


class _environ:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
class _Slice:
    """one activation operand: `values` [..., C] (None: an output that is written) as the channel slice
    [c0, c0 + C) of a [guard + M + guard][ld] buffer filled with `fill`; ld == C, c0 == 0 is the packed form
    (no guard pixels: the call test_gpu_configs.py makes)"""

    def __init__(self, M, C, ld, c0, dtype, fill, values=None):
        self.M, self.C, self.ld, self.c0, self.fill = M, C, ld, c0, fill
        self.g = 0 if (ld == C and c0 == 0) else GUARD
        self.buf, view = sliced((self.g + M + self.g,), C, ld, c0, dtype, fill, DEV)
        self.view = view[self.g:self.g + M]
        self.values = None
        if values is not None:
            self.values = values.reshape(M, C).clone()
            self.view.copy_(self.values)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        return self.view.contiguous()

    def check(self, what, is_input):
        assert_guard(self.buf, self.c0, self.C, self.fill, f"{what} (foreign channels)")
        if self.g:
            assert_guard(self.buf[:self.g], 0, 0, self.fill, f"{what} (guard pixels before)")
            assert_guard(self.buf[self.g + self.M:], 0, 0, self.fill, f"{what} (guard pixels after)")
        if is_input:
            assert torch.equal(_bits(self.view), _bits(self.values)), f"{what}: an input was written"


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    n = int((a != b).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ between the strided and the packed call"


def _flat(nf, n_extra=64):
    """(exact-size fp32 output of nf elements with a NaN tail of n_extra, checked by _tail)"""
    return torch.full((nf + n_extra,), NAN, dtype=torch.float32, device=DEV)


def _ratio_bf16(out, ref, extra=None):
    """largest |out - ref| over the bf16 output bound 2^-8 |ref| (+ extra) + 1e-4 max|ref|"""
    out, ref = out.double(), ref.double()
    bound = 2.0 ** -8 * (ref.abs() if extra is None else extra) + 1e-4 * ref.abs().max().item()
    return float(((out - ref).abs() / bound).max())


def _merge_stats(stt, tile, M, y_rows, what):
    """the BN partials [G][2][K] merged over the row tiles against the stored output's statistics (1e-4, as
    tests/test_gpu_configs.py); returns the largest error over its bound"""
    st_ = stt.double()
    G = st_.shape[0]
    cnt = torch.tensor([min(tile, M - g * tile) for g in range(G)], dtype=torch.float64, device=DEV)
    tot = st_[:, 0].sum(0)
    mean = tot / M
    m2 = (st_[:, 1] + cnt[:, None] * (st_[:, 0] / cnt[:, None] - mean) ** 2).sum(0)
    o = y_rows.double().t()  # [K][M]
    b0 = 1e-4 * o.sum(1).abs() + 1e-4 * o.abs().sum(1).max().item() / M * 10
    b1 = 1e-4 * o.var(1, unbiased=False).abs() + 1e-6
    r0, r1 = float(((tot - o.sum(1)).abs() / b0).max()), float(((m2 / M - o.var(1, unbiased=False)).abs() / b1).max())
    assert r0 <= 1 and r1 <= 1, f"{what}: merged BN partials off (sum {r0:.3g}, variance {r1:.3g} of their bounds)"
    return max(r0, r1)


def _part_ratio(got, terms, what):
    """row partials summed against the float64 sums, bound 1e-4 sum |terms| + 1e-6 (tests/test_gpu_post_res.py)"""
    worst = 0.0
    for k, t in enumerate(terms):
        bound = 1e-4 * t.abs().sum(0) + 1e-6
        r = float(((got[k] - t.sum(0)).abs() / bound).max())
        assert r <= 1, f"{what}: partial quantity {k} at {r:.3g} of its bound"
        worst = max(worst, r)
    return worst


def _report(cid, keys, tiles, ratio, t0):
    torch.cuda.synchronize()
    print(f"strided-case {cid}: config {','.join(sorted(set(keys)))} row_tiles {tiles} "
          f"err/bound {ratio:.3f} wall {(time.perf_counter() - t0) * 1e3:.0f}ms")


# ------------------------------------------------------------------------------------------------
# one call of a direction with a given layout -> (outputs by name, slices to check)
# ------------------------------------------------------------------------------------------------
class _Values:
    """the values of one case, drawn once and shared by the packed and the strided call"""

    def __init__(self, direction, shape, seed):
        N, H, W, C1, C2, K, R, s = shape
        self.op = op = _Op(shape, seed)
        cin = C1 + C2
        g = op.gen
        self.wk, self.wt = op.packed()
        self.g0 = _bf(torch.randn(N, H, W, cin, generator=g, device=DEV))
        z = _bf(torch.randn(N, H, W, cin, generator=g, device=DEV))
        self.z = z
        self.aux = torch.relu(z) if direction == "post1" else z
        self.y2 = _bf(torch.randn(N, H, W, cin, generator=g, device=DEV))
        n = max(cin, C1)
        self.sc = (1 + 0.3 * torch.randn(n, generator=g, device=DEV)).float()
        self.sh = (0.3 * torch.randn(n, generator=g, device=DEV)).float()
        self.mu = (0.1 * torch.randn(n, generator=g, device=DEV)).float()
        self.inv = (1 + 0.2 * torch.rand(n, generator=g, device=DEV)).float()
        self.mu2 = (0.1 * torch.randn(n, generator=g, device=DEV)).float()
        self.inv2 = (0.5 + torch.rand(n, generator=g, device=DEV)).float()
        self.mbits = torch.randint(0, 256, (N * H * W * (cin // 8),), generator=g, device=DEV, dtype=torch.uint8)


def _call(direction, shape, v, lay):
    from unetseg_hip.lib import DT_BF16, lib
    N, H, W, C1, C2, K, R, s = shape
    op, st = v.op, _st()
    pad, P, Q, cin = op.pad, op.P, op.Q, C1 + C2
    Mi, Mo = N * H * W, N * P * Q
    out, slices = {}, []

    def S(M, C, i, fill, values=None, name=""):
        sl = _Slice(M, C, lay[i][0], lay[i][1], BF, fill, values)
        slices.append((name, sl, values is not None and fill == SENTINEL and name[0] != "+"))
        return sl

    if direction.startswith("fwd"):
        x1v, x2v = op.x_parts()
        if direction == "fwd_bnrelu_in":
            x1v = _nhwc(op.x)
        x1 = S(Mi, C1, 0, SENTINEL, x1v, "x1")
        x2 = S(Mi, C2, 1, SENTINEL, x2v, "x2") if C2 else None
        y = S(Mo, K, len(lay) - 1, NAN, None, "y")
        relu = direction in ("fwd_relu", "fwd_all")
        stats = direction in ("fwd_stats", "fwd_all", "fwd_bnrelu_in")
        ld2 = x2.ld if C2 else 0
        R_, s_, pad_ = (1, 1, 0) if direction == "fwd_bnrelu_in" else (R, s, pad)
        tile = lib.conv2d_fwd_tile_m(DT_BF16, C1, x1.ld, C2, ld2, N, H, W, K, R_, R_, s_, pad_)
        G = -(-Mo // tile)
        stt = _flat(G * 2 * K) if stats else None
        if direction == "fwd_bnrelu_in":
            lib.conv2d_fwd_bnrelu_in(DT_BF16, x1.ptr, C1, x1.ld, N, H, W, _P(v.wk), K, _P(v.sc), _P(v.sh), 0, 0, y.ptr,
                                     y.ld, _P(stt), st)
        else:
            lib.conv2d_fwd(DT_BF16, x1.ptr, C1, x1.ld, x2.ptr if C2 else 0, C2, ld2, N, H, W, _P(v.wk), K, R, R, s, pad,
                           _P(op.bias) if relu else 0, int(relu), y.ptr, y.ld, _P(stt), st)
        out["y"] = y.get()
        if stats:
            assert_tail(stt, G * 2 * K, NAN, "BN partials")
            out["stats"] = stt[:G * 2 * K].reshape(G, 2, K)
            out["tile"] = tile
    elif _QUERY[direction][1] == "dgrad":
        dy = S(Mo, K, 0, SENTINEL, _nhwc(op.dy), "dy")
        if direction == "dgrad":
            for acc in (0, 1):
                dx = S(Mi, cin, 1, SENTINEL if acc else NAN, v.g0 if acc else None, "+dx" if acc else "dx")
                lib.conv2d_dgrad(DT_BF16, dy.ptr, dy.ld, N, P, Q, _P(v.wt), K, cin, R, R, s, pad, dx.ptr, dx.ld, H, W, acc, st)
                out[f"dx{acc}"] = dx.get()
        elif direction in ("post1", "post2", "post4"):
            post = int(direction[-1])
            dx = S(Mi, cin, 1, NAN, None, "dx")
            if post == 4:
                auxp, ld_aux = _P(v.mbits), 0
            else:
                aux = S(Mi, cin, 2, SENTINEL, v.aux, "aux")
                auxp, ld_aux = aux.ptr, aux.ld
            coeffs = [_P(v.sc), _P(v.sh), _P(v.mu), _P(v.inv)] if post == 2 else [0, 0, 0, 0]
            args = [DT_BF16, dy.ptr, dy.ld, N, P, Q, _P(v.wt), K, cin, R, R, s, pad]
            rows = lib.conv2d_dgrad_post(*args, 0, dx.ld, H, W, post, auxp, ld_aux, *coeffs, 0, 0, st)
            assert rows > 0, "shape has no fused path"
            part = _flat(rows * 2 * cin)
            rc = lib.conv2d_dgrad_post(*args, dx.ptr, dx.ld, H, W, post, auxp, ld_aux, *coeffs, _P(part), rows, st)
            assert rc == 0
            assert_tail(part, rows * 2 * cin, NAN, "post partials")
            out["dx"], out["part"] = dx.get(), part[:rows * 2 * cin].reshape(rows, 2, cin)
        else:  # post3 / post3_y2
            two = direction == "post3_y2"
            dx = S(Mi, cin, 1, SENTINEL, v.g0, "+dx")
            y1 = S(Mi, cin, 2, SENTINEL, v.z, "y1")
            y2 = S(Mi, cin, 3, SENTINEL, v.y2, "y2") if two else None
            rows = lib.conv2d_dgrad_post_res(DT_BF16, dy.ptr, dy.ld, N, P, Q, _P(v.wt), K, cin, 0, dx.ld, y1.ptr, y1.ld,
                                             0, 0, 0, 0, 0, 0, 0, 0, 0, st)
            assert rows > 0, "shape has no fused residual kernel"
            nq = 3 if two else 2
            part = _flat(rows * nq * cin)
            lib.conv2d_dgrad_post_res(DT_BF16, dy.ptr, dy.ld, N, P, Q, _P(v.wt), K, cin, dx.ptr, dx.ld, y1.ptr, y1.ld,
                                      _P(v.mu), _P(v.inv), _P(v.mbits), y2.ptr if two else 0, y2.ld if two else 0,
                                      _P(v.mu2) if two else 0, _P(v.inv2) if two else 0, _P(part), rows, st)
            assert_tail(part, rows * nq * cin, NAN, "post-3 partials")
            out["dx"], out["part"] = dx.get(), part[:rows * nq * cin].reshape(rows, nq, cin)
    else:  # wgrad / wgrad_bnrelu_in
        x1v, x2v = op.x_parts()
        x1 = S(Mi, C1, 0, SENTINEL, x1v, "x1")
        x2 = S(Mi, C2, 1, SENTINEL, x2v, "x2") if C2 else None
        dy = S(Mo, K, len(lay) - 1, SENTINEL, _nhwc(op.dy), "dy")
        ws_bytes = lib.conv2d_wgrad_workspace(DT_BF16, N, P, Q, K, cin, R, R)
        ws = torch.full((max(ws_bytes, 1) // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
        nw = K * cin * R * R
        dw = _flat(nw)
        for acc in (0, 1):
            if direction == "wgrad":
                lib.conv2d_wgrad(DT_BF16, x1.ptr, C1, x1.ld, x2.ptr if C2 else 0, C2, x2.ld if C2 else 0, N, H, W, dy.ptr,
                                 dy.ld, K, R, R, s, pad, _P(ws), ws_bytes, _P(dw), cin, acc, st)
            else:
                lib.conv2d_wgrad_bnrelu_in(DT_BF16, x1.ptr, C1, x1.ld, N, H, W, dy.ptr, dy.ld, K, _P(v.sc), _P(v.sh),
                                           _P(ws), ws_bytes, _P(dw), C1, acc, st)
            out[f"dw{acc}"] = dw[:nw].reshape(K, cin, R, R).clone()
        assert_tail(dw, nw, NAN, "dw")
    torch.cuda.synchronize()
    return out, slices


def _check_packed(cid, direction, shape, v, out):
    """the packed call against float64 (the references and tolerances of tests/test_gpu_configs.py);
    returns the largest error over its bound"""
    N, H, W, C1, C2, K, R, s = shape
    op = v.op
    pad, cin = op.pad, C1 + C2
    x64, w64, dy64 = op.x.double(), op.w32.double(), op.dy.double()
    if direction.startswith("fwd"):
        if direction == "fwd_bnrelu_in":
            a = torch.relu((_nhwc(op.x).double() * v.sc[:C1].double() + v.sh[:C1].double()).float()).to(BF)
            ref = _ref_fwd(_nchw(a), w64, 1, 0)
        else:
            ref = _ref_fwd(x64, w64, s, pad)
            if direction in ("fwd_relu", "fwd_all"):
                ref = torch.relu(ref + op.bias.double().view(1, -1, 1, 1))
        y = _nchw(out["y"].reshape(N, op.P, op.Q, K))
        _check_bf16(y, ref, f"{cid} y")
        ratio = _ratio_bf16(y, ref)
        if "stats" in out:
            ratio = max(ratio, _merge_stats(out["stats"], out["tile"], N * op.P * op.Q, out["y"], cid))
        return ratio
    if _QUERY[direction][1] == "dgrad":
        ref = _ref_dgrad(dy64, w64, H, W, s, pad)
        if direction == "dgrad":
            dx0, dx1 = _nchw(out["dx0"].reshape(N, H, W, cin)), _nchw(out["dx1"].reshape(N, H, W, cin))
            _check_bf16(dx0, ref, f"{cid} dx")
            acc_ref = _nchw(v.g0) + ref
            # the bound of the accumulated form: half an ulp of the dgrad plus half an ulp of the sum
            err = (dx1 - acc_ref).abs()
            bound = 2.0 ** -8 * (ref.abs() + acc_ref.abs()) + 1e-4 * ref.abs().max().item()
            assert int((err > bound).sum()) == 0, f"{cid} dx accumulated: max err {err.max().item():.3e}"
            return max(_ratio_bf16(dx0, ref), float((err / bound).max()))
        d = _nchw(out["dx"].reshape(N, H, W, cin))
        M = N * H * W
        if direction in ("post1", "post2", "post4"):
            a64 = _nchw(v.aux)
            if direction == "post1":
                mask = a64 > 0
            elif direction == "post2":  # sign of fmaf(z, sc, sh): exact in float64
                mask = (a64 * v.sc[:cin].double().view(1, -1, 1, 1) + v.sh[:cin].double().view(1, -1, 1, 1)) > 0
            else:
                bits = torch.stack([(v.mbits >> e) & 1 for e in range(8)], dim=1).reshape(N, H, W, cin).bool()
                mask = bits.permute(0, 3, 1, 2)
            mref = torch.where(mask, ref, torch.zeros_like(ref))
            _check_bf16(d, mref, f"{cid} d")
            assert (d[~mask] == 0).all(), f"{cid}: masked elements are not zero"
            rows_d = d.permute(0, 2, 3, 1).reshape(M, cin)
            terms = [rows_d]
            if direction == "post2":
                xhat = (v.aux.reshape(M, cin).double() - v.mu[:cin].double()) * v.inv[:cin].double()
                terms.append(rows_d * xhat)
            got = out["part"].double().sum(0)
            return max(_ratio_bf16(d, mref), _part_ratio(got, terms, cid))
        # post 3: mask * bf16(dgrad + old)
        bits = torch.stack([(v.mbits >> e) & 1 for e in range(8)], dim=1).reshape(N, H, W, cin).bool().permute(0, 3, 1, 2)
        acc_ref = _nchw(v.g0) + ref
        mref = torch.where(bits, acc_ref, torch.zeros_like(ref))
        err = (d - mref).abs()
        bound = 2.0 ** -8 * (ref.abs() + acc_ref.abs()) + 1e-4 * ref.abs().max().item()
        assert int((err > bound).sum()) == 0, f"{cid} d: max err {err.max().item():.3e}"
        assert (d[~bits] == 0).all(), f"{cid}: masked elements are not zero"
        rows_d = d.permute(0, 2, 3, 1).reshape(M, cin)
        terms = [rows_d, rows_d * ((v.z.reshape(M, cin).double() - v.mu[:cin].double()) * v.inv[:cin].double())]
        if direction == "post3_y2":
            terms.append(rows_d * ((v.y2.reshape(M, cin).double() - v.mu2[:cin].double()) * v.inv2[:cin].double()))
        return max(float((err / bound).max()), _part_ratio(out["part"].double().sum(0), terms, cid))
    # weight gradients
    if direction == "wgrad_bnrelu_in":
        a = torch.relu((_nhwc(op.x).double() * v.sc[:C1].double() + v.sh[:C1].double()).float()).to(BF)
        ref = _ref_wgrad(_nchw(a), dy64, 1, 1, 0)
    else:
        ref = _ref_wgrad(x64, dy64, R, s, pad)
    m = ref.abs().max().item()
    err = (out["dw0"].double() - ref).abs()
    bound = 1e-3 * ref.abs() + 2e-5 * m
    assert int((err > bound).sum()) == 0, f"{cid}: dw out of tolerance (max err {err.max().item():.3e}, max|ref| {m:.3e})"
    assert torch.equal(out["dw1"], out["dw0"] + out["dw0"]), f"{cid}: accumulated wgrad is not 2x the first"
    return float((err / bound).max())


def test_post_res_2x2_has_no_fused_kernel():
    """(N, H, W, K, C) = (2, 2, 2, 512, 2048) of tests/test_gpu_post_res.py (the 2 x 2 layer4 maps of a 64^2 input)
    takes the 64x128 tile, which has no post-3 instantiation (conv_fast.hip kTnTable): the rows query answers 0
    for the packed and for the padded strides alike, so the op layer runs the unfused pair either way and there
    is no fused call to compare."""
    from unetseg_hip.lib import DT_BF16, dgrad_config, lib
    N, H, W, K, C = 2, 2, 2, 512, 2048
    for lay in (packed_layout([K, C, C, C]), layout([K, C, C, C], False), layout([K, C, C, C], True)):
        assert dgrad_config(DT_BF16, lay[0][0], N, H, W, K, C, 1, 1, 1, 0, lay[1][0], H, W) == ["tn64x128"]
        assert lib.conv2d_dgrad_post_res(DT_BF16, 0, lay[0][0], N, H, W, 0, K, C, 0, lay[1][0], 0, lay[2][0], 0, 0, 0, 0,
                                         lay[3][0], 0, 0, 0, 0, _st()) == 0


@pytest.mark.parametrize("cid", list(STRIDED_CASES))
def test_strided_case(cid, monkeypatch):
    t0 = time.perf_counter()
    direction, shape, expect, env, tail = STRIDED_CASES[cid]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    chs = operand_channels(direction, shape)
    lay = layout(chs, tail)
    keys_p, keys_s = case_keys(direction, shape, packed_layout(chs)), case_keys(direction, shape, lay)
    assert keys_s == keys_p, f"{cid}: the strides {lay} select {keys_s}, the packed call {keys_p}"
    assert keys_s == expect, f"{cid}: selects {keys_s}, the case lists {expect}"
    v = _Values(direction, shape, tgc.RNG + sum(map(ord, cid)))
    packed, _ = _call(direction, shape, v, packed_layout(chs))
    ratio = _check_packed(cid, direction, shape, v, packed)
    strided, slices = _call(direction, shape, v, lay)
    for name in packed:
        if name != "tile":
            _same(strided[name], packed[name], f"{cid} {name}")
    assert strided.get("tile") == packed.get("tile")
    for name, sl, is_input in slices:
        sl.check(f"{cid} {name}", is_input)
    _report(cid, keys_s, row_tiles(keys_s[0], direction, shape), ratio, t0)


# ------------------------------------------------------------------------------------------------
# entry points with their own signatures
# ------------------------------------------------------------------------------------------------
def _head_values(shape, seed):
    N, H, W = shape
    op = _Op((N, H, W, 64, 0, 64, 3, 1), seed)
    wk, _ = op.packed()
    return op, wk


@pytest.mark.parametrize("head_k,tail,hs", [(1, False, "0"), (2, True, "1")])
def test_fwd_head_strided(head_k, tail, hs, monkeypatch):
    """unetseg_conv2d_fwd_head: ldc1 and ldy wide; y and the fp32 logits [n][head_k][h][w]"""
    from unetseg_hip.lib import DT_BF16, lib
    t0 = time.perf_counter()
    monkeypatch.setenv("UNETSEG_HALO_HS", hs)
    N, H, W = 3, 16, 64
    M = N * H * W
    op, wk = _head_values((N, H, W), 4321 + head_k)
    hw = (torch.randn(head_k, 64, generator=op.gen, device=DEV) / 8).float()
    hb = (0.1 * torch.randn(head_k, generator=op.gen, device=DEV)).float()
    res = {}
    for tag, lay in (("packed", packed_layout([64, 64])), ("strided", layout([64, 64], tail))):
        assert lib.conv2d_fwd_head_ok(DT_BF16, lay[0][0], N, H, W, lay[1][0], head_k) == 1, (tag, lay)
        x = _Slice(M, 64, *lay[0], BF, SENTINEL, op.x_parts()[0])
        y = _Slice(M, 64, *lay[1], BF, NAN)
        logits = _flat(N * head_k * H * W)
        lib.conv2d_fwd_head(DT_BF16, x.ptr, x.ld, N, H, W, _P(wk), _P(op.bias), y.ptr, y.ld, head_k, _P(hw), _P(hb),
                            _P(logits), _st())
        torch.cuda.synchronize()
        assert_tail(logits, N * head_k * H * W, NAN, "logits")
        x.check(f"head {tag} x", True)
        y.check(f"head {tag} y", False)
        res[tag] = (y.get(), logits[:N * head_k * H * W].clone())
    _same(res["strided"][0], res["packed"][0], "head y")
    _same(res["strided"][1], res["packed"][1], "head logits")
    yp, lg = res["packed"]
    ref = torch.relu(_ref_fwd(op.x.double(), op.w32.double(), 1, 1) + op.bias.double().view(1, -1, 1, 1))
    _check_bf16(_nchw(yp.reshape(N, H, W, 64)), ref, "head y")
    # logits = head_b + head_w . (stored y): 64 fp32 multiply-adds and the bias add, any order
    y64 = yp.double()
    lref = (y64 @ hw.double().t() + hb.double()).reshape(N, H, W, head_k).permute(0, 3, 1, 2)
    lmag = (y64.abs() @ hw.double().abs().t() + hb.double().abs()).reshape(N, H, W, head_k).permute(0, 3, 1, 2)
    r = assert_elementwise(lg.reshape(N, head_k, H, W), lref, lmag, torch.float32, 65, "head logits")
    _report(f"fwd_head_k{head_k}", ["fwd:halo3"], M // 256, max(r, _ratio_bf16(_nchw(yp.reshape(N, H, W, 64)), ref)), t0)


@pytest.mark.parametrize("tail,hs", [(False, "1"), (True, "0")])
def test_fwd_mask_strided(tail, hs, monkeypatch):
    """unetseg_conv2d_fwd_mask: ldc1 and ldy wide; the mask bits stay [M][8] and name the stored y's sign"""
    from unetseg_hip.lib import DT_BF16, lib
    t0 = time.perf_counter()
    monkeypatch.setenv("UNETSEG_HALO_HS", hs)
    N, H, W = 3, 16, 64
    M = N * H * W
    op, wk = _head_values((N, H, W), 777)
    res = {}
    for tag, lay in (("packed", packed_layout([64, 64])), ("strided", layout([64, 64], tail))):
        assert lib.conv2d_fwd_mask(DT_BF16, 0, lay[0][0], N, H, W, 0, 0, 0, lay[1][0], 0, 0) == 1, (tag, lay)
        x = _Slice(M, 64, *lay[0], BF, SENTINEL, op.x_parts()[0])
        y = _Slice(M, 64, *lay[1], BF, NAN)
        mb = torch.full((M * 8 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        lib.conv2d_fwd_mask(DT_BF16, x.ptr, x.ld, N, H, W, _P(wk), _P(op.bias), y.ptr, y.ld, _P(mb), _st())
        torch.cuda.synchronize()
        assert_tail(mb, M * 8, 0xA5, "mask bits")
        x.check(f"mask {tag} x", True)
        y.check(f"mask {tag} y", False)
        res[tag] = (y.get(), mb[:M * 8].reshape(M, 8).clone())
    _same(res["strided"][0], res["packed"][0], "mask y")
    assert torch.equal(res["strided"][1], res["packed"][1]), "mask bits differ between the strided and the packed call"
    yp, bits = res["packed"]
    ref = torch.relu(_ref_fwd(op.x.double(), op.w32.double(), 1, 1) + op.bias.double().view(1, -1, 1, 1))
    _check_bf16(_nchw(yp.reshape(N, H, W, 64)), ref, "mask y")
    want = ((yp.float() > 0).reshape(M, 8, 8).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1)
    assert torch.equal(bits.to(torch.int32), want), "mask bits are not the sign of the stored y"
    _report("fwd_mask", ["fwd:halo3"], M // 256, _ratio_bf16(_nchw(yp.reshape(N, H, W, 64)), ref), t0)


@pytest.mark.parametrize("dtype,relu,tail", [(torch.float32, 1, False), (BF, 0, True), (BF, 1, False)])
def test_fwd_affine_strided(dtype, relu, tail):
    """unetseg_conv2d_fwd_affine (the generic kernel), two sources with ldc1 != ldc2, fp32 and bf16"""
    from unetseg_hip.lib import DT_BF16, DT_F32, lib
    t0 = time.perf_counter()
    N, H, W, C1, C2, K, R, s = shape = (2, 13, 11, 16, 24, 72, 3, 2)
    dt = DT_BF16 if dtype == BF else DT_F32
    op = _Op(shape, 99 + relu)
    cin, pad, P, Q = C1 + C2, 1, op.P, op.Q
    Mi, Mo = N * H * W, N * P * Q
    wk = torch.empty(K, R, R, cin, dtype=dtype, device=DEV)
    lib.pack_conv_weight(dt, op.w32.data_ptr(), K, cin, R, R, cin, wk.data_ptr(), 0, _st())
    esc = (1 + 0.3 * torch.randn(K, generator=op.gen, device=DEV)).float()
    x1v, x2v = op.x_parts()
    res = {}
    for tag, lay in (("packed", packed_layout([C1, C2, K])), ("strided", layout([C1, C2, K], tail))):
        x1 = _Slice(Mi, C1, *lay[0], dtype, SENTINEL, x1v.to(dtype))
        x2 = _Slice(Mi, C2, *lay[1], dtype, SENTINEL, x2v.to(dtype))
        y = _Slice(Mo, K, *lay[2], dtype, NAN)
        lib.conv2d_fwd_affine(dt, x1.ptr, C1, x1.ld, x2.ptr, C2, x2.ld, N, H, W, _P(wk), K, R, R, s, pad, _P(esc),
                              _P(op.bias), relu, y.ptr, y.ld, _st())
        torch.cuda.synchronize()
        for nm, sl, inp in (("x1", x1, True), ("x2", x2, True), ("y", y, False)):
            sl.check(f"affine {tag} {nm}", inp)
        res[tag] = y.get()
    _same(res["strided"], res["packed"], "affine y")
    x64, w64 = op.x.double(), op.w32.double()
    e, b = esc.double().view(1, -1, 1, 1), op.bias.double().view(1, -1, 1, 1)
    ref = _ref_fwd(x64, w64, s, pad) * e + b
    mag = _ref_fwd(x64.abs(), w64.abs(), s, pad) * e.abs() + b.abs()
    if relu:
        ref = torch.relu(ref)
    got = _nchw(res["packed"].reshape(N, P, Q, K))
    if dtype == BF:
        _check_bf16(got, ref, "affine y")
        ratio = _ratio_bf16(got, ref)
    else:  # an exact fp32 fma chain over cin * R * S products, then the epilogue's fma
        ratio = assert_elementwise(got, ref, mag, torch.float32, cin * R * R + 1, "affine y (fp32)")
    _report(f"fwd_affine_{'bf16' if dtype == BF else 'fp32'}", ["fwd_affine:generic"], -(-Mo // 128), ratio, t0)


@pytest.mark.parametrize("H,W", [(15, 17), (16, 32)])
@pytest.mark.parametrize("C1", [64, 128])
@pytest.mark.parametrize("K", [32, 40])
def test_padk_strided(K, C1, H, W):
    """the narrow 1x1 gradients on a 64-padded dY (the attention gates' theta / phi): unetseg_conv2d_wgrad_rows
    writes rows 0..K-1 of a [64][C1] sentinel-filled dw and leaves the rest; the padded-K unetseg_conv2d_dgrad
    (wt [C1][64], pad columns zero) gives dx.  Both against float64 and packed-vs-strided."""
    from unetseg_hip.lib import DT_BF16, dgrad_config, lib, wgrad_config
    t0 = time.perf_counter()
    N, KP = 2, 64
    M = N * H * W
    g = torch.Generator(device=DEV).manual_seed(K * 1000 + C1 + H)
    x = _bf(torch.randn(M, C1, generator=g, device=DEV))
    dyv = torch.zeros(M, KP, dtype=BF, device=DEV)
    dyv[:, :K] = _bf(torch.randn(M, K, generator=g, device=DEV))
    w = _bf(torch.randn(K, C1, generator=g, device=DEV) / math.sqrt(C1))
    wt = torch.zeros(C1, KP, dtype=BF, device=DEV)
    wt[:, :K] = w.t()
    tail = (K + C1 + H) % 3 == 0
    lays = {"packed": packed_layout([C1, KP, C1]), "strided": layout([C1, KP, C1], tail)}
    kw = {t: wgrad_config(DT_BF16, C1, l[0][0], 0, 0, N, H, W, l[1][0], KP, 1, 1, 1, 0)[0] for t, l in lays.items()}
    kd = {t: dgrad_config(DT_BF16, l[1][0], N, H, W, KP, C1, 1, 1, 1, 0, l[2][0], H, W) for t, l in lays.items()}
    assert kw["strided"] == kw["packed"] and kd["strided"] == kd["packed"], (kw, kd)
    ws_bytes = lib.conv2d_wgrad_workspace(DT_BF16, N, H, W, KP, C1, 1, 1)
    res = {}
    for tag, lay in lays.items():
        xs = _Slice(M, C1, *lay[0], BF, SENTINEL, x)
        dy = _Slice(M, KP, *lay[1], BF, SENTINEL, dyv)
        ws = torch.full((max(ws_bytes, 1) // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
        dw = torch.full((KP, C1), SENTINEL, dtype=torch.float32, device=DEV)
        dws = []
        for acc in (0, 1):
            lib.conv2d_wgrad_rows(DT_BF16, xs.ptr, C1, xs.ld, N, H, W, dy.ptr, dy.ld, KP, 1, 1, 1, 0, _P(ws), ws_bytes,
                                  _P(dw), C1, acc, K, _st())
            dws.append(dw.clone())
        outs = []
        for acc in (0, 1):
            dx = _Slice(M, C1, *lay[2], BF, SENTINEL if acc else NAN, x if acc else None)
            lib.conv2d_dgrad(DT_BF16, dy.ptr, dy.ld, N, H, W, _P(wt), KP, C1, 1, 1, 1, 0, dx.ptr, dx.ld, H, W, acc, _st())
            torch.cuda.synchronize()
            dx.check(f"padk {tag} dx acc={acc}", False)
            outs.append(dx.get())
        xs.check(f"padk {tag} x", True)
        dy.check(f"padk {tag} dy", True)
        res[tag] = dws + outs
    for i, nm in enumerate(("dw", "dw accumulated", "dx", "dx accumulated")):
        _same(res["strided"][i], res["packed"][i], f"padk {nm}")
    dw0, dw1, dx0, dx1 = res["packed"]
    assert_guard(dw0[K:], 0, 0, SENTINEL, "dw rows past dw_rows")
    assert_guard(dw1[K:], 0, 0, SENTINEL, "dw rows past dw_rows (accumulated)")
    ref = dyv[:, :K].double().t() @ x.double()
    m = ref.abs().max().item()
    bound = 1e-3 * ref.abs() + 2e-5 * m
    err = (dw0[:K].double() - ref).abs()
    assert int((err > bound).sum()) == 0, f"dw rows: max err {err.max().item():.3e} (max|ref| {m:.3e})"
    assert torch.equal(dw1[:K], dw0[:K] + dw0[:K]), "accumulated wgrad_rows is not 2x the first"
    dref = dyv[:, :K].double() @ w.double()
    _check_bf16(dx0, dref, "padk dx")
    acc_ref = x.double() + dref
    e1 = (dx1.double() - acc_ref).abs()
    b1 = 2.0 ** -8 * (dref.abs() + acc_ref.abs()) + 1e-4 * dref.abs().max().item()
    assert int((e1 > b1).sum()) == 0, f"padk dx accumulated: max err {e1.max().item():.3e}"
    ratio = max(float((err / bound).max()), _ratio_bf16(dx0, dref), float((e1 / b1).max()))
    _report(f"padk_K{K}_C{C1}_{H}x{W}", [f"wgrad:{kw['packed']}"] + [f"dgrad:{c}" for c in kd["packed"]],
            -(-M // 128), ratio, t0)


@pytest.mark.parametrize("N,H,tn,expect", STEM_CASES)
def test_stem_strided(N, H, tn, expect, monkeypatch):
    """unetseg_stem_fwd / unetseg_stem_wgrad with a wide ldy (y, then dy): the persistent-halo stem kernel and
    the TN 128x64 tile"""
    from unetseg_hip import introspect
    from unetseg_hip.lib import lib, stem_config
    t0 = time.perf_counter()
    if tn:
        monkeypatch.setenv("UNETSEG_STEM_TN", "1")
    K, C = 64, 3
    cfg, _ = stem_config(N, H, H, K)
    assert cfg == expect, cfg
    wkey = introspect.call_configs(("stem_wgrad", N, H, H, C, 0, K, 7, 7, 2, 3, 8, 0))[0]
    g = torch.Generator(device=DEV).manual_seed(N + H)
    x = torch.rand(N, C, H, H, generator=g, device=DEV)
    w = _bf(torch.randn(K, C, 7, 7, generator=g, device=DEV) / math.sqrt(147)).float()
    Pq = (H - 1) // 2 + 1
    M = N * Pq * Pq
    dyv = _bf(torch.randn(M, K, generator=g, device=DEV))
    xp = torch.empty(N, H, H + 8, 8, dtype=BF, device=DEV)
    lib.pack_input_stem(_P(x), N, C, H, H, _P(xp), _st())
    wk = torch.empty(K, 7, 64, dtype=BF, device=DEV)
    lib.stem_pack_weight(_P(w), K, C, _P(wk), _st())
    tile = lib.stem_fwd_tile_m(N, H, H, K)
    G = -(-M // tile)
    ws_bytes = lib.stem_wgrad_workspace(N, H, H, K)
    res = {}
    for tag, lay in (("packed", packed_layout([K, K])), ("strided", layout([K, K], tn))):
        y = _Slice(M, K, *lay[0], BF, NAN)
        stt = _flat(G * 2 * K)
        lib.stem_fwd(_P(xp), N, H, H, _P(wk), K, y.ptr, y.ld, _P(stt), _st())
        dy = _Slice(M, K, *lay[1], BF, SENTINEL, dyv)
        ws = torch.full((ws_bytes // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
        dw = _flat(K * C * 49)
        dws = []
        for acc in (0, 1):
            lib.stem_wgrad(_P(xp), N, H, H, dy.ptr, dy.ld, K, _P(ws), ws_bytes, _P(dw), C, acc, _st())
            dws.append(dw[:K * C * 49].clone())
        torch.cuda.synchronize()
        assert_tail(stt, G * 2 * K, NAN, "stem BN partials")
        assert_tail(dw, K * C * 49, NAN, "stem dw")
        y.check(f"stem {tag} y", False)
        dy.check(f"stem {tag} dy", True)
        res[tag] = [y.get(), stt[:G * 2 * K].reshape(G, 2, K).clone()] + dws
    for i, nm in enumerate(("y", "BN partials", "dw", "dw accumulated")):
        _same(res["strided"][i], res["packed"][i], f"stem {nm}")
    yp, stp, dw0, dw1 = res["packed"]
    xr = _bf(x).double()
    ref = _ref_fwd(xr, w.double(), 2, 3)
    yn = _nchw(yp.reshape(N, Pq, Pq, K))
    _check_bf16(yn, ref, "stem y")
    ratio = max(_ratio_bf16(yn, ref), _merge_stats(stp, tile, M, yp, "stem"))
    dref = _ref_wgrad(xr, _nchw(dyv.reshape(N, Pq, Pq, K)), 7, 2, 3)
    m = dref.abs().max().item()
    err = (dw0.reshape(K, C, 7, 7).double() - dref).abs()
    bound = 1e-3 * dref.abs() + 2e-5 * m
    assert int((err > bound).sum()) == 0, f"stem dw: max err {err.max().item():.3e}"
    assert torch.equal(dw1, dw0 + dw0), "accumulated stem wgrad is not 2x the first"
    _report(f"stem_{H}_{expect}", [f"stem_fwd:{cfg}", wkey], G, max(ratio, float((err / bound).max())), t0)


@pytest.mark.parametrize("direction,shape", FIRST3X3_CASES)
def test_first3x3_strided(direction, shape):
    """the first-3x3 kernel on the 8-channel packed image: ldc1 stays 8 (first3x3_ok), ldy wide"""
    from unetseg_hip.lib import DT_BF16, fwd_config, lib
    t0 = time.perf_counter()
    N, H, W, C1, C2, K, R, s = shape
    assert fwd_config(DT_BF16, 8, 8, 0, 0, N, H, W, K, 3, 3, 1, 1) == "first3x3"
    op = _Op(shape, 31 + N)
    wk, _ = op.packed()
    M = N * H * W
    relu, stats = direction == "fwd_relu", direction == "fwd_stats"
    tile = lib.conv2d_fwd_tile_m(DT_BF16, 8, 8, 0, 0, N, H, W, K, 3, 3, 1, 1)
    G = -(-M // tile)
    x1 = op.x_parts()[0]
    res = {}
    for tag, (ld, c0) in (("packed", (K, 0)), ("strided", layout([K], relu)[0])):
        y = _Slice(M, K, ld, c0, BF, NAN)
        stt = _flat(G * 2 * K) if stats else None
        lib.conv2d_fwd(DT_BF16, _P(x1), 8, 8, 0, 0, 0, N, H, W, _P(wk), K, 3, 3, 1, 1, _P(op.bias) if relu else 0, int(relu),
                       y.ptr, y.ld, _P(stt), _st())
        torch.cuda.synchronize()
        y.check(f"first3x3 {tag} y", False)
        res[tag] = [y.get()] + ([stt[:G * 2 * K].reshape(G, 2, K).clone()] if stats else [])
        if stats:
            assert_tail(stt, G * 2 * K, NAN, "first3x3 BN partials")
    for a, b in zip(res["strided"], res["packed"]):
        _same(a, b, "first3x3")
    ref = _ref_fwd(op.x.double(), op.w32.double(), 1, 1)
    if relu:
        ref = torch.relu(ref + op.bias.double().view(1, -1, 1, 1))
    yn = _nchw(res["packed"][0].reshape(N, H, W, K))
    _check_bf16(yn, ref, "first3x3 y")
    ratio = _ratio_bf16(yn, ref)
    if stats:
        ratio = max(ratio, _merge_stats(res["packed"][1], tile, M, res["packed"][0], "first3x3"))
    _report(f"first3x3_{direction}", ["fwd:first3x3"], G, ratio, t0)
