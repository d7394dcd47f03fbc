"""Time the contour trace (csrc/contours.hip, unetseg_hip/contours.py) beside ``ccl.label`` and the Python
reference tracer.

    python tools/contours_timing.py [--reps 9] [--out profiles/contours_timing.json]

Inputs: the synthetic generator's masks (utils/synthetic.py: a few filled ellipses per image, 8-connected) and
percolation noise (density 0.59, 4-connected: many loops, some of them long), at 512 x 512 with N = 8 and at
2048 x 2048 with N = 1.  ``trace`` and ``ccl.label`` are timed on the same tensors in the same process: after
three warm-up calls, ``reps`` calls each inside its own HIP-event window; the median, the minimum and the maximum
are kept.  ``trace`` waits on the host twice per call (it reads the crack count, then the loop and vertex counts)
and labels the map itself, so its window holds those waits, torch's scans and sort and one ``ccl.label``.  The
reference tracer (tests/contours_ref.py, pure Python) is timed once on one 512 x 512 image of each input with the
wall clock.  A record, not a pass/fail bar.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic(N, S):
    from utils.synthetic import make_batch

    return make_batch(N, S, seed=7)[1].to(torch.int32).cuda()


def percolation(N, S):
    g = torch.Generator(device="cuda").manual_seed(0)
    return (torch.rand(N, S, S, generator=g, device="cuda") < 0.59).to(torch.int32)


def event_us(fn, reps, warmup=3):
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
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import contours_ref
    from unetseg_hip import ccl, contours

    rec = {"reps": a.reps, "warmup": 3, "tile": list(contours.tile()), "rows": [], "cpu_reference": []}
    for name, make, conn in (("synthetic", synthetic, 8), ("percolation_0.59", percolation, 4)):
        for N, S in ((8, 512), (1, 2048)):
            m = make(N, S)
            loops, vertices = contours.trace(m, conn)
            t = event_us(lambda: contours.trace(m, conn), a.reps)
            l = event_us(lambda: ccl.label(m, conn), a.reps)
            row = {"input": name, "shape": [N, S, S], "connectivity": conn, "loops": int(loops.shape[0]),
                   "vertices": int(vertices.shape[0]), "cracks": int(loops[:, 7].sum()),
                   "longest_loop": int(loops[:, 7].max()) if loops.shape[0] else 0, "trace": t, "ccl_label": l,
                   "trace_over_label": round(t["median_us"] / l["median_us"], 2)}
            if S == 512:  # the CPU tracer on the first image, once
                im = m[0].cpu().numpy()
                t0 = time.perf_counter()
                want = contours_ref.trace(im, conn)
                cpu_s = time.perf_counter() - t0
                one = event_us(lambda: contours.trace(m[0], conn), a.reps)
                got = contours.trace(m[0], conn)
                same = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and
                            np.array_equal(got[1].cpu().numpy(), want[1]))
                rec["cpu_reference"].append({"input": name, "shape": [S, S], "connectivity": conn,
                                             "reference_s": round(cpu_s, 3), "trace": one, "equal": same,
                                             "reference_over_trace": round(cpu_s * 1e6 / one["median_us"], 1)})
                print(json.dumps(rec["cpu_reference"][-1]), flush=True)
            rec["rows"].append(row)
            print(json.dumps(row), flush=True)
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
