"""Time the hard-skeleton thinning and the clDice counts (csrc/skeleton.hip), and val.py with and without them.

    python tools/skeleton_timing.py [--reps 20] [--out profiles/skeleton_timing.json] [--no-val]

Maps: the targets of utils.synthetic.make_batch at 16 x 512^2 and 8 x 512^2 (about 27 % foreground), and the worst
case, a full 8 x 512^2 map, all at the default pass cap.
* calls: HIP-event windows around single calls, median over ``reps`` after three warm-up calls.
* launches: a call is 2 + ceil(max_passes / K) launches whatever the data.  ``launches_needed`` is the smallest
  number of thinning launches after which no image reports unconverged (found on the host beforehand); the rest
  return at once.  What one such launch costs is taken from an empty map, whose every launch but the first returns
  at once: (t(default cap) - t(cap K)) / (launches - 1).  ``early_share`` is that cost times the launches that
  were not needed, over the call.
* floor: one pass over the packed map moves 1 + 1 bytes per pixel; over the copy rate measured here (a 1 GiB
  device copy, read + write) that is the least a launch that does work can take.  ``per_working_launch_us`` is
  (call - early launches - the call at cap 0) / launches_needed, beside it.
* counts: skeleton.counts (both thinnings on the stacked maps and the count launch), and for scale the same
  process's boundary.counts on the same pair.
* val.py: ``--task binary --data-path synthetic`` on random unet_resnet50 weights, the wall time of whole runs
  with and without --skeleton-metrics in alternating order; without the flag the run issues the parent commit's
  calls, so it stands for the parent here.
A record, not a pass/fail bar.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from cldice_timing import copy_rate, median_us  # noqa: E402  (tools/ is the script's directory)


def launches_needed(skeleton, m, K):
    """thinning launches until no image of m still loses pixels"""
    n = 1
    while int(skeleton.thin(m, n * K, return_unconverged=True)[1].sum().item()):
        n += 1
    return n


def time_maps(reps, rate):
    from unetseg_hip import boundary, skeleton
    from utils.synthetic import make_batch

    _, _, K = skeleton.tile()
    rows = []
    early_us = None
    cases = [("empty", 8), ("synthetic", 16), ("synthetic", 8), ("full", 8)]
    for kind, B in cases:
        S = 512
        if kind == "synthetic":
            m = make_batch(B, S, seed=1234)[1].to("cuda", torch.int32).contiguous()
        else:
            m = torch.full((B, S, S), 1 if kind == "full" else 0, dtype=torch.int32, device="cuda")
        cap = skeleton.default_max_passes(S, S)
        launches = -(-cap // K)
        need = launches_needed(skeleton, m, K)
        t = median_us(lambda: skeleton.thin(m), reps)
        t0 = median_us(lambda: skeleton.thin(m, 0), reps)
        row = {"map": kind, "shape": [B, S, S], "foreground_share": round(float((m != 0).float().mean()), 4),
               "max_passes": cap, "launches": launches, "launches_needed": need, "thin_us": round(t, 1),
               "pack_and_finish_us": round(t0, 1)}
        if kind == "empty":
            tk = median_us(lambda: skeleton.thin(m, K), reps)
            early_us = (t - tk) / (launches - 1)
            row["early_launch_us"] = round(early_us, 2)
        else:
            early = early_us * (launches - need)
            floor = 2.0 * B * S * S / rate * 1e6
            row.update({"early_share": round(early / t, 3),
                        "per_working_launch_us": round((t - early - t0) / need, 1),
                        "pass_floor_us": round(floor, 1)})
            if kind == "synthetic":
                p = torch.roll(m, (2, 3), (1, 2))
                row["skeleton_counts_us"] = round(median_us(lambda: skeleton.counts(p, m), reps), 1)
                row["boundary_counts_us"] = round(median_us(lambda: boundary.counts(p, m), reps), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def time_val(rounds, images, batch):
    """wall seconds of whole val.py runs with and without --skeleton-metrics, alternating"""
    import val
    from model.model_factory import build_model

    torch.manual_seed(3)
    with tempfile.TemporaryDirectory() as d:
        w = os.path.join(d, "w.pth")
        torch.save(build_model("unet_resnet50", num_classes=2).state_dict(), w)
        base = ["--task", "binary", "--data-path", "synthetic", "--weights", w, "--synthetic-test", str(images),
                "--batch-size", str(batch)]
        arms = {"plain": base, "skeleton": base + ["--skeleton-metrics"]}
        secs = {k: [] for k in arms}
        metrics = {}
        for r in range(rounds + 1):  # the first round warms up
            for k, argv in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    metrics[k] = val.val(val.parse_args(argv))
                torch.cuda.synchronize()
                if r:
                    secs[k].append(time.perf_counter() - t0)
    return {"command": "val.py --task binary --data-path synthetic", "model": "unet_resnet50", "images": images,
            "batch": batch, "size": 512, "rounds": rounds,
            "plain_s": round(statistics.median(secs["plain"]), 3), "plain_range_s": [round(min(secs["plain"]), 3),
                                                                                     round(max(secs["plain"]), 3)],
            "skeleton_s": round(statistics.median(secs["skeleton"]), 3),
            "skeleton_range_s": [round(min(secs["skeleton"]), 3), round(max(secs["skeleton"]), 3)],
            "clDice": metrics["skeleton"]["clDice"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-val", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skeleton_timing: needs the GPU (a timing taken elsewhere says nothing)")
    rate = copy_rate()
    rec = {"copy_bytes_per_s": round(rate), "reps": a.reps, "maps": time_maps(a.reps, rate)}
    if not a.no_val:
        rec["val"] = time_val(a.rounds, a.images, a.batch)
        print(json.dumps(rec["val"]), flush=True)
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
