"""Time the boundary passes (csrc/boundary.hip) beside their streaming floor.

    python tools/boundary_timing.py [--reps 7] [--shapes 16x512x512,1x2048x2048,1x4096x6144]
                                    [--out profiles/boundary_timing.json]

Operations: ``edges``, ``sqdist`` and ``counts`` of unetseg_hip/boundary.py (``counts`` is the whole chain
a batch of an evaluation pays: two edge maps, two distance transforms, one counting pass).  Inputs: a
few large discs, 0.5-density noise, and a single site in one corner, the worst case of the windowed row
pass (for ``edges`` and ``counts`` that is a one-pixel class-1 region against a prediction one pixel
off).  Each figure is the median over ``reps`` of one HIP-event window around one call, after two warm-up
calls, in one process.  The floor is the bytes the passes cannot avoid moving over the copy rate measured
here as tools/hbm_bw.py measures it (a 1 GiB device copy, read + write): edges reads a map and writes
bytes, 5 B / pixel; sqdist as a column pass (1 + 4 B) and a row pass (4 + 4 B), 13 B; the counting pass
reads two maps, two edge maps and two transforms, 18 B, so the chain is 2 * 5 + 2 * 13 + 18 = 54 B.
``evaluate_binary`` over the synthetic test split at 512 x 512 (unet_plain, batch 4) is timed end to end
with and without ``boundary``.  A record, not a pass/fail bar.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

BYTES = {"edges": 5, "sqdist": 13, "counts": 54}


def copy_rate():
    """bytes / s of a 1 GiB device-to-device copy, read + write (tools/hbm_bw.py's first figure)"""
    n = 1 << 30
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        y.copy_(x)
    e1.record()
    e1.synchronize()
    return 2 * n / (e0.elapsed_time(e1) / 20 * 1e-3)


def discs(N, H, W):
    y = torch.arange(H, device="cuda")[:, None].float()
    x = torch.arange(W, device="cuda")[None, :].float()
    a = torch.zeros(H, W, dtype=torch.int32, device="cuda")
    for cy, cx, r in ((0.3, 0.3, 0.22), (0.7, 0.6, 0.25), (0.35, 0.8, 0.12), (0.8, 0.15, 0.1)):
        a[(y - cy * H) ** 2 + (x - cx * W) ** 2 < (r * min(H, W)) ** 2] = 1
    return a.expand(N, H, W).contiguous()


def noise(N, H, W):
    g = torch.Generator(device="cuda").manual_seed(0)
    return (torch.rand(N, H, W, generator=g, device="cuda") < 0.5).to(torch.int32)


def corner(N, H, W):
    a = torch.zeros(N, H, W, dtype=torch.int32, device="cuda")
    a[:, 0, 0] = 1
    return a


def median_us(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def time_evaluate(reps, n_images=16, size=512, batch=4):
    """seconds of evaluate_binary over the synthetic test split, without and with the boundary metrics"""
    from model.model_factory import build_model
    from torch.utils.data import DataLoader
    from utils.synthetic import SyntheticSegDataset, collate
    from utils.train_and_eval import evaluate_binary

    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model("unet_plain", num_classes=2).cuda()
    batches = list(DataLoader(SyntheticSegDataset(n_images, [size, size], 2, seed=888_000), batch_size=batch,
                              shuffle=False, num_workers=0, collate_fn=collate))  # decoded once, outside the window
    out = {}
    for name, opt in (("plain", None), ("boundary", {"tolerance": 2.0, "biou_d": None})):
        ts = []
        for _ in range(reps + 1):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = evaluate_binary(model, batches, torch.device("cuda"), "bce", None, boundary=opt)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name + "_s"] = round(statistics.median(ts[1:]), 5)
        out[name + "_keys"] = sorted(m)
    out.update(images=n_images, size=size, batch=batch, model="unet_plain")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="16x512x512,1x2048x2048,1x4096x6144")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-evaluate", action="store_true")
    a = ap.parse_args()
    from unetseg_hip import boundary

    rate = copy_rate()
    rec = {"copy_bytes_per_s": round(rate), "reps": a.reps, "chunk": boundary.chunk(), "rows": []}
    for shape in a.shapes.split(","):
        N, H, W = (int(v) for v in shape.split("x"))
        for name, make in (("discs", discs), ("noise", noise), ("corner", corner)):
            t = make(N, H, W)
            p = torch.roll(t, (1, 2), (1, 2))  # the prediction: the target a pixel down, two to the right
            sites = boundary.edges(t) if name != "corner" else t.to(torch.uint8)
            ops = {"edges": lambda: boundary.edges(t), "sqdist": lambda: boundary.sqdist(sites),
                   "counts": lambda: boundary.counts(p, t)}
            for op, fn in ops.items():
                us = median_us(fn, a.reps)
                floor = BYTES[op] * N * H * W / rate * 1e6
                rec["rows"].append({"shape": [N, H, W], "input": name, "sites": int((sites != 0).sum()), "op": op,
                                    "median_us": round(us, 1), "floor_us": round(floor, 1),
                                    "over_floor": round(us / floor, 1)})
                print(json.dumps(rec["rows"][-1]), flush=True)
            del t, p, sites
    if not a.no_evaluate:
        rec["evaluate_binary"] = time_evaluate(min(a.reps, 3))
        print(json.dumps(rec["evaluate_binary"]), flush=True)
    try:
        rec["commit"] = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        rec["commit"] = None
    rec["device"] = torch.cuda.get_device_name(0)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
