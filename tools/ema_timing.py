"""Time the Adam step with and without the fused weight average (csrc/optim.hip) on the unet_resnet50 arena.

    python tools/ema_timing.py [--reps 50] [--out profiles/ema_timing.json] [--commit <id>]

Four things on flat fp32 arrays of the model's parameter count, each a HIP-event window around one call, the median
over ``reps`` after five warm-up calls, the four interleaved call by call so they see the same clocks:
* adam         unetseg_adam alone: 4 reads + 3 writes per element (7 streams, 28 B);
* adam_ema     unetseg_adam_ema, the update and the average in one pass: 5 reads + 4 writes (9 streams, 36 B);
* two_pass     unetseg_adam, then the average as a pass of its own written with a torch op (ema.lerp_(p, 1 - d): it
               reads the fresh p back, 2 reads + 1 write, 12 B): 10 streams, 40 B, two launches in one window;
* swap         unetseg_swap_f32, the in-place exchange averaged() makes twice per evaluation: 2 reads + 2 writes, 16 B.
From the byte counts the fused call should take about 9 / 7 of Adam alone and less than the two passes.
The record carries the commit, the clocks read right after the timed calls and each call's achieved GB/s.
A record, not a pass/fail bar.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WARM = 5
MODEL = "unet_resnet50"
BYTES = {"adam": 28, "adam_ema": 36, "two_pass": 40, "ema_pass_torch": 12, "swap": 16}


def arena_size():
    from model.model_factory import build_model
    return sum(p.numel() for p in build_model(MODEL, num_classes=2).parameters())


def clocks():
    rec = {"max_sclk_mhz": None, "sclk_mhz": None}
    try:
        rec["max_sclk_mhz"] = torch.cuda.get_device_properties(0).clock_rate / 1e3
    except Exception:  # noqa: BLE001 - diagnostics only
        pass
    try:
        rec["sclk_mhz"] = float(torch.cuda.clock_rate())
    except Exception:  # noqa: BLE001 - needs the SMI python binding
        pass
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_timing: needs the GPU (a timing taken elsewhere says nothing)")
    from unetseg_hip.arena import ema_one_minus_decay
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P

    n = arena_size()
    torch.cuda.set_stream(torch.cuda.Stream("cuda"))
    gen = torch.Generator(device="cuda").manual_seed(11)
    p, g, m, ema = (torch.randn(n, device="cuda", generator=gen) * 0.05 for _ in range(4))
    v = torch.rand(n, device="cuda", generator=gen) * 1e-3
    st = torch.cuda.current_stream().cuda_stream
    omd = ema_one_minus_decay(0.999, False, 1000)
    hp = (1e-4, 0.9, 0.999, 1e-8, 1e-4, 1000)

    def adam():
        lib.adam(P(p), P(g), P(m), P(v), n, *hp, None, st)

    def adam_ema():
        lib.adam_ema(P(p), P(g), P(m), P(v), P(ema), n, *hp, omd, None, st)

    def ema_pass_torch():
        ema.lerp_(p, omd)

    def two_pass():
        adam()
        ema_pass_torch()

    def swap():
        lib.swap_f32(P(p), P(ema), n, st)

    calls = {"adam": adam, "adam_ema": adam_ema, "two_pass": two_pass, "ema_pass_torch": ema_pass_torch, "swap": swap}
    for fn in calls.values():
        for _ in range(WARM):
            fn()
    us = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    clk = clocks()
    rec = {"model": MODEL, "elements": n, "reps": a.reps, "warmup": WARM, "calls": {}}
    for k, ts in us.items():
        med = statistics.median(ts)
        rec["calls"][k] = {"median_us": round(med, 1), "range_us": [round(min(ts), 1), round(max(ts), 1)],
                           "bytes_per_element": BYTES[k], "gb_per_s": round(BYTES[k] * n / med * 1e-3, 1)}
    c = rec["calls"]
    rec["adam_ema_over_adam"] = round(c["adam_ema"]["median_us"] / c["adam"]["median_us"], 3)
    rec["adam_ema_over_two_pass"] = round(c["adam_ema"]["median_us"] / c["two_pass"]["median_us"], 3)
    rec["expected_adam_ema_over_adam"] = round(9 / 7, 3)
    rec["clocks"] = clk
    try:  # --commit names the tree where it is not a git checkout
        rec["commit"] = a.commit or subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        rec["commit"] = None
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
