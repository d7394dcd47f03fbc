#!/usr/bin/env python3
"""Record what the host-only geometry queries of the memory-bound op families answer over a fixed shape list.

The queries size the partial buffers and workspaces their launches write, so a launch and its query must
agree.  They launch nothing and need no device.  tests/golden/elem_geometry.json holds the recording and
tests/test_elem_geometry_cpu.py requires a fresh one to equal it entry by entry, so a change of the host code
of csrc/elem.hip, upsample.hip, pointwise.hip, resize.hip or the loss files that moves a shape to another
block count shows up on the CPU.

Some knobs are read at every call and others are latched on first use, so every knob setting is recorded in
a child process of its own, started with no other UNETSEG_* variable (UNETSEG_LIB_PATH is honoured: an A/B
build records through the same script).

  python tools/record_elem_geometry.py > tests/golden/elem_geometry.json

Output: {setting: {query: {key: value or [ints]}}}, one entry per line; the two knob settings hold only the
query their knob reaches.
  reduce_tiles   "dtype,M,C" -> [blocks, tv, ppb]
  up_bwd_tiles   "dtype,n,h,w,c"
  pw             "M" -> [pw_small_tile, pw_small_tiles, pw_head_tiles, attn_bwd1_tiles]
  channel_stats  "M,tile"
  loss_ws        "B,P" -> [bce, lovasz, masked_loss]
  mc_ws          "B,C,P" -> [mc_loss, lovasz_softmax per image, lovasz_softmax flat]
"""
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "unet-embroidery-seg_amd"))

# knob setting -> the queries recorded under it (None: all)
SETTINGS = {"unset": None, "UNETSEG_RED_TARGET=2048": ["reduce_tiles"], "UNETSEG_UP_STREAM=0": ["up_bwd_tiles"]}

# every model's activations at the bench sizes: batch 8 or 16, 512^2 input, levels 512 .. 16, and a superset
# of the channel counts of the five models (encoders, decoders' concatenations, dense blocks, gates)
BATCHES = (8, 16)
LEVELS = (512, 256, 128, 64, 32, 16)
CHANNELS = (16, 32, 64, 96, 128, 192, 256, 320, 384, 512, 768, 1024, 2048)


def vec(dt):
    return 8 if dt == 1 else 4


def reduce_shapes():
    out = []
    for dt in (1, 0):
        V = vec(dt)
        for B in BATCHES:
            for s in LEVELS:
                out += [(dt, B * s * s, C) for C in (CHANNELS if dt == 1 else (64, 256, 1024))]
        # the edges of the rule: 1, 2, 64 and 128 channel vectors; M = 1, around one block's pixels (the
        # smallest block: 8 pixel rows of 256 / tv threads each), and 2^20
        for cv in (1, 2, 64, 128):
            ppb = 8 * (256 // min(cv, 64))
            out += [(dt, M, cv * V) for M in (1, ppb - 1, ppb, ppb + 1, 1 << 20)]
        out += [(dt, 1000, 3 * V), (dt, 12345, 24 * V), (dt, 0, 8 * V)]
    return out


def up_shapes():
    out = []
    for dt in (1, 0):
        V = vec(dt)
        for B in BATCHES:
            for s in LEVELS[1:]:
                out += [(dt, B, s, s, C) for C in (64, 128, 256, 512, 1024)]
        # h a multiple of 16, of 8 only, of neither
        for h in (16, 48, 8, 24, 40, 12, 15, 20, 1):
            out += [(dt, 2, h, 32, 8 * V), (dt, 16, h, 64, 16 * V)]
        # both sides of the 2048-block rule (16 rows per block keep >= 2048 blocks, else 8): x blocks * n * h / 16
        for n, h, w, cv in ((16, 128, 256, 1), (16, 128, 255, 1), (16, 128, 257, 1), (8, 128, 256, 2),
                            (8, 128, 256, 1), (1, 16, 256, 128), (1, 32, 256, 128), (1, 32, 128, 256)):
            out.append((dt, n, h, w, cv * V))
        # w * (c / V) on both sides of 256 (one x block or two)
        for w, cv in ((16, 8), (32, 8), (33, 8), (255, 1), (256, 1), (257, 1), (1, 256), (3, 128)):
            out += [(dt, 4, 16, w, cv * V), (dt, 4, 12, w, cv * V)]
    seen, uniq = set(), []
    for k in out:
        if k not in seen:
            seen.add(k)
            uniq.append(k)
    return uniq


def pw_ms():
    ms = {B * s * s for B in BATCHES for s in LEVELS} | {0, 1, 127, 128, 129}
    # both sides of each halving of the pixel tile: 512 blocks of 2048, 1024, 512, 256 pixels
    for t in (2048, 1024, 512, 256, 128):
        ms |= {511 * t - 1, 511 * t, 511 * t + 1, 512 * t - 1, 512 * t, 512 * t + 1}
    # the head's 2048-pixel tile and the gate's 128-pixel one
    ms |= {2047, 2048, 2049, 1 << 20, (1 << 20) + 1}
    return sorted(ms)


def record():
    from unetseg_hip import lib as L  # reads UNETSEG_LIB_PATH
    lib = L.load()
    one = ctypes.c_int
    rec = {}
    red = rec["reduce_tiles"] = {}
    for dt, M, C in reduce_shapes():
        tv, ppb = one(-1), one(-1)
        g = lib.unetseg_reduce_tiles(dt, M, C, ctypes.byref(tv), ctypes.byref(ppb))
        red[f"{dt},{M},{C}"] = [g, tv.value, ppb.value]
    rec["up_bwd_tiles"] = {",".join(map(str, k)): lib.unetseg_upsample2x_bwd_tiles(*k) for k in up_shapes()}
    rec["pw"] = {str(M): [lib.unetseg_pw_small_tile(M), lib.unetseg_pw_small_tiles(M), lib.unetseg_pw_head_tiles(M),
                          lib.unetseg_attn_bwd1_tiles(M)] for M in pw_ms()}
    rec["channel_stats"] = {f"{M},{t}": lib.unetseg_channel_stats_tiles(M, t)
                            for M in (1, 255, 256, 257, 16 * 64 * 64, 16 * 512 * 512) for t in (1, 64, 256, 2048)}
    bp = [(B, P) for B in (1, 16) for P in (1, 255, 256, 257, 4095, 4096, 4097, 64 * 64, 480 * 480, 512 * 512)]
    rec["loss_ws"] = {f"{B},{P}": [lib.unetseg_bce_workspace(B, P), lib.unetseg_lovasz_workspace(B, P),
                                   lib.unetseg_masked_loss_workspace(B, P)] for B, P in bp}
    rec["mc_ws"] = {f"{B},{C},{P}": [lib.unetseg_mc_loss_workspace(B, C, P),
                                     lib.unetseg_lovasz_softmax_workspace(B, C, P, 1),
                                     lib.unetseg_lovasz_softmax_workspace(B, C, P, 0)]
                    for B in (1, 16) for P in (1, 4097, 512 * 512) for C in (2, 5, 32)}
    return rec


def dump(rec, f):
    f.write("{\n")
    for si, (setting, queries) in enumerate(rec.items()):
        f.write(f'"{setting}": {{\n')
        for qi, (q, entries) in enumerate(queries.items()):
            f.write(f'"{q}": {{\n')
            f.write(",\n".join(f'"{k}":{json.dumps(v, separators=(",", ":"))}' for k, v in entries.items()))
            f.write("\n}" + ("," if qi + 1 < len(queries) else "") + "\n")
        f.write("}" + ("," if si + 1 < len(rec) else "") + "\n")
    f.write("}\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        json.dump(record(), sys.stdout)
        return
    base = {k: v for k, v in os.environ.items() if not k.startswith("UNETSEG_") or k == "UNETSEG_LIB_PATH"}
    rec = {}
    for setting, keep in SETTINGS.items():
        env = dict(base)
        if setting != "unset":
            k, v = setting.split("=")
            env[k] = v
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                           text=True, timeout=120)
        if r.returncode != 0:
            sys.exit(f"{setting}: {r.stderr[-3000:]}")
        got = json.loads(r.stdout)
        rec[setting] = {q: v for q, v in got.items() if keep is None or q in keep}
    dump(rec, sys.stdout)


if __name__ == "__main__":
    main()
