#!/usr/bin/env python3
"""Record what every host-only conv dispatch query of the C ABI answers over a fixed shape list.

The queries (unetseg_conv2d_*_config / _tile_m / _workspace, the part == NULL row queries of the fused
data gradients, the stem's) launch nothing and need no device: without one the library's CU count falls
back to 256, the MI355X's.  The recording pins the dispatch rules of csrc/conv.hip: tests/golden/
conv_dispatch.json holds it and tests/test_conv_dispatch_cpu.py requires a fresh one to equal it entry by
entry, so a change of the host code that moves a shape to another kernel, tile or split count shows up
on the CPU.

Every UNETSEG_* variable is removed from the environment before the library loads (UNETSEG_LIB_PATH is
honoured first: an A/B build records through the same script).

  python tools/record_conv_dispatch.py > tests/golden/conv_dispatch.json

Output: {"conv": {key: [ints]}, "stem": {key: [ints]}}, one entry per line.
  conv key  "dtype,N,H,W,C1,C2,ld1,ld2,K,ldk,R,stride,pad" (ldk: pixel stride of the K-channel tensor)
  conv ints fwd_config cfg, taps | fwd_tile_m | wgrad_config kind, splits | wgrad_workspace |
            dgrad_config launched, then cfg, taps per parity class | dgrad_post rows for post 1, 2, 4 |
            1x1 stride 1 only: fwd_bnrelu_in_config, dgrad_post_res rows without / with y2 |
            64 -> 64 3x3 stride 1 only: fwd_head_ok for head_k 1, 2, fwd_mask
  stem key  "N,H,W,K"; ints stem_config cfg, splits | stem_fwd_tile_m | stem_wgrad_workspace
"""
import ast
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "unet-embroidery-seg_amd"))

GEOMS = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (1, 2, 0), (7, 2, 3)]
C1S = [8, 64, 136, 192, 256, 1024]
KS = [32, 40, 64, 128, 512]
NS = [1, 3, 8, 16]
SQUARE = [15, 16, 32, 64, 128, 512]
RAGGED = (15, 17)


def case_shapes():
    """the shape tuples of CASES and HALO_CASES in tests/test_gpu_configs.py (read from its source: importing
    the module would pull in torch)"""
    with open(os.path.join(REPO, "tests", "test_gpu_configs.py")) as f:
        tree = ast.parse(f.read())
    out = []
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) in ("CASES", "HALO_CASES"):
            out += [ast.literal_eval(v.elts[1]) for v in node.value.values]
    return out


def shapes():
    """(dtype, N, H, W, C1, C2, ld1, ld2, K, ldk, R, stride, pad), in a fixed order, without repeats"""
    out, seen = [], set()

    def add(dt, N, H, W, C1, C2, K, R, stride, pad, extra=0):
        # what the launching entry points refuse: channels / strides that are no multiple of 8, an empty output
        if C1 % 8 or C2 % 8 or K % 8 or (H + 2 * pad - R) // stride + 1 <= 0 or (W + 2 * pad - R) // stride + 1 <= 0:
            return
        key = (dt, N, H, W, C1, C2, C1 + extra, C2 + extra if C2 else 0, K, K + extra, R, stride, pad)
        if key not in seen:
            seen.add(key)
            out.append(key)

    for N, H, W, C1, C2, K, R, stride in case_shapes():
        add(1, N, H, W, C1, C2, K, R, stride, R // 2)

    def grid(dt, every, c2=0, extra=0):
        full = [(N, hw, C1, K, g) for N in NS for hw in SQUARE + [RAGGED] for C1 in C1S for K in KS for g in GEOMS]
        for N, hw, C1, K, (R, stride, pad) in full[::every]:
            H, W = hw if isinstance(hw, tuple) else (hw, hw)
            add(dt, N, H, W, C1, c2, K, R, stride, pad, extra)

    # the grid (4,200 combinations per variant), trimmed to keep the recording small: every n-th
    # combination, n a prime that divides none of the dimensions' sizes, so every value of a dimension
    # meets every value of the others
    grid(1, 13)
    grid(1, 37, c2=128)
    grid(1, 37, extra=64)
    grid(0, 53)
    # past the 2^31-byte extent of 32-bit buffer offsets (nothing is allocated)
    for C1, K, R, stride, extra in [(64, 64, 3, 1, 64), (64, 64, 3, 1, 0), (128, 128, 1, 1, 0), (64, 256, 1, 1, 0),
                                    (256, 64, 1, 1, 0), (128, 128, 3, 2, 0), (64, 64, 1, 2, 64)]:
        add(1, 64, 512, 512, C1, 0, K, R, stride, R // 2, extra)
    add(1, 32, 512, 512, 64, 0, 64, 3, 1, 1)         # 2^30 bytes: the largest that fits
    add(1, 32, 512, 512, 64, 128, 64, 3, 1, 1, 64)   # second source past it, first within
    add(1, 32, 512, 512, 64, 0, 128, 3, 1, 1)        # input within, output (and dy) at 2^31
    return out


def stem_shapes():
    sizes = [(15, 15), (15, 17), (16, 16), (32, 32), (64, 64), (128, 128), (200, 200), (256, 256), (512, 512)]
    return [(N, H, W, K) for K in (64, 32, 128) for N in ((1, 2, 3, 8, 16) if K == 64 else (16,)) for H, W in sizes]


def record():
    from unetseg_hip import lib as L  # reads UNETSEG_LIB_PATH
    for k in [k for k in os.environ if k.startswith("UNETSEG_")]:
        del os.environ[k]
    lib = L.load()
    i4 = ctypes.c_int * 4
    one = ctypes.c_int
    some = 256  # a placeholder address: the queries only test pointers for NULL
    conv = {}
    for key in shapes():
        dt, N, H, W, C1, C2, ld1, ld2, K, ldk, R, stride, pad = key
        cin = C1 + C2
        ldx = cin + (ldk - K)
        P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        v = []
        taps = one(0)
        v += [lib.unetseg_conv2d_fwd_config(dt, C1, ld1, C2, ld2, N, H, W, K, R, R, stride, pad, ctypes.byref(taps))]
        v += [taps.value, lib.unetseg_conv2d_fwd_tile_m(dt, C1, ld1, C2, ld2, N, H, W, K, R, R, stride, pad)]
        sp = one(0)
        v += [lib.unetseg_conv2d_wgrad_config(dt, C1, ld1, C2, ld2, N, H, W, ldk, K, R, R, stride, pad,
                                              ctypes.byref(sp))]
        v += [sp.value, lib.unetseg_conv2d_wgrad_workspace(dt, N, P, Q, K, cin, R, R)]
        cfg, tp = i4(), i4()
        v += [lib.unetseg_conv2d_dgrad_config(dt, ldk, N, P, Q, K, cin, R, R, stride, pad, ldx, H, W, cfg, tp)]
        for i in range(stride * stride):
            v += [cfg[i], tp[i]]
        for post in (1, 2, 4):
            v += [lib.unetseg_conv2d_dgrad_post(dt, None, ldk, N, P, Q, None, K, cin, R, R, stride, pad, None, ldx, H, W,
                                                post, None, ldx, None, None, None, None, None, 0, None)]
        if R == 1 and stride == 1 and C2 == 0:
            v += [lib.unetseg_conv2d_fwd_bnrelu_in_config(dt, C1, ld1, N, H, W, K)]
            for y2 in (None, some):
                v += [lib.unetseg_conv2d_dgrad_post_res(dt, None, ldk, N, P, Q, None, K, cin, None, ldx, None, ldx, None,
                                                        None, None, y2, ldx, None, None, None, 0, None)]
        if R == 3 and stride == 1 and C1 == 64 and C2 == 0 and K == 64:
            v += [lib.unetseg_conv2d_fwd_head_ok(dt, ld1, N, H, W, ldk, hk) for hk in (1, 2)]
            v += [lib.unetseg_conv2d_fwd_mask(dt, None, ld1, N, H, W, None, None, None, ldk, None, None)]
        conv[",".join(map(str, key))] = v
    stem = {}
    for key in stem_shapes():
        sp = one(0)
        cfg = lib.unetseg_stem_config(*key, ctypes.byref(sp))
        stem[",".join(map(str, key))] = [cfg, sp.value, lib.unetseg_stem_fwd_tile_m(*key),
                                         lib.unetseg_stem_wgrad_workspace(*key)]
    return {"conv": conv, "stem": stem}


def dump(rec, f):
    f.write("{\n")
    for si, (sec, entries) in enumerate(rec.items()):
        f.write(f'"{sec}": {{\n')
        f.write(",\n".join(f'"{k}":[{",".join(map(str, v))}]' for k, v in entries.items()))
        f.write("\n}" + ("," if si + 1 < len(rec) else "") + "\n")
    f.write("}\n")


if __name__ == "__main__":
    dump(record(), sys.stdout)
