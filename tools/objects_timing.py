"""Time the object-level counts (csrc/objects.hip) and an evaluate_binary pass with and without them.

    python tools/objects_timing.py [--reps 30] [--out profiles/objects_timing.json] [--no-eval]

Maps: the targets of utils.synthetic.make_batch at 16 x 512^2 and 1 x 2048^2 (a few large ellipses) with the
prediction the target shifted by (2, 3) pixels, once as it is and once with 1 % of its pixels flipped (thousands
of one-pixel objects and holes).
* calls: HIP-event windows around single calls, median and range over ``reps`` after three warm-up calls.
* floor: ``ccl.label`` + ``ccl.stats`` on the same two maps, which the feature cannot avoid; ``ratio_to_floor`` is
  ``objects.counts`` over it.
* parts: the label stage (the floor's kernels into the workspace), the pair stage (two memsets and the pair
  kernel), the match stage (one memset, the match and the count kernel).
* pair kernel A/B: the product kernel, which gathers a block's runs in an LDS table, against the same kernel with
  the aggregation compiled out (every run head goes to the global table), alternating in one process.
* evaluate_binary: the wall time of whole passes over a fixed list of batches on unet_resnet50 with and without
  ``objects={}``, alternating; without the option the pass issues the parent commit's calls.
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
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WARM = 3


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def timed(fns, reps):
    """{name: {"us": median, "range_us": [min, max]}} of the calls, taken in alternating order"""
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_us(fn))
    return {k: {"us": round(statistics.median(v), 1), "range_us": [round(min(v), 1), round(max(v), 1)]}
            for k, v in ts.items()}


def time_maps(reps):
    from unetseg_hip import ccl, objects
    from utils.synthetic import make_batch

    rows = []
    for B, S in ((16, 512), (1, 2048)):
        t = make_batch(B, S, seed=1234)[1].to("cuda", torch.int32).contiguous()
        shifted = torch.roll(t, (2, 3), (1, 2))
        flip = torch.rand(t.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) < 0.01
        for kind, p in (("shifted", shifted), ("shifted + 1 % flips", torch.where(flip, 1 - shifted, shifted))):
            p = p.contiguous()
            lab = objects._Labelled(p, t, 8)
            out = torch.zeros(objects.N_COUNTS, dtype=torch.int64, device="cuda")
            lab.pairs(1)

            def floor():
                for m in (p, t):
                    ccl.stats(ccl.label(m, 8))

            r = timed({"counts": lambda: objects.counts(p, t, out=out), "floor": floor,
                       "label_stage": lambda: objects._Labelled(p, t, 8), "match_stage": lambda: lab.match(1, out),
                       "pair_stage": lambda: lab.pairs(1, True), "pair_stage_plain": lambda: lab.pairs(1, False)}, reps)
            c = objects.counts(p, t).tolist()
            row = {"shape": [B, S, S], "pred": kind, "target_objects": c[0], "pred_objects": c[1], "pairs": c[17],
                   "dropped_insertions": c[18], "workspace_bytes": lab.size,
                   "workspace_bytes_per_pixel": round(lab.size / (B * S * S), 2), **r,
                   "ratio_to_floor": round(r["counts"]["us"] / r["floor"]["us"], 3),
                   "plain_over_aggregated": round(r["pair_stage_plain"]["us"] / r["pair_stage"]["us"], 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def time_eval(rounds, batches_n, batch):
    """wall seconds of whole evaluate_binary passes with and without objects={}, alternating"""
    from model.model_factory import build_model
    from utils.synthetic import make_batch
    from utils.train_and_eval import evaluate_binary

    torch.manual_seed(3)
    model = build_model("unet_resnet50", num_classes=2).cuda()
    batches = [(*make_batch(batch, 512, seed=900 + k), None) for k in range(batches_n)]
    arms = {"plain": None, "objects": {}}
    secs = {k: [] for k in arms}
    metrics = {}
    for r in range(rounds + 1):  # the first round warms up
        for k, opt in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                metrics[k] = evaluate_binary(model, batches, torch.device("cuda"), "bce", None, objects=opt)
            torch.cuda.synchronize()
            if r:
                secs[k].append(time.perf_counter() - t0)
    rec = {"call": "evaluate_binary", "model": "unet_resnet50", "batches": batches_n, "batch": batch, "size": 512,
           "rounds": rounds}
    for k, v in secs.items():
        rec[k + "_s"] = round(statistics.median(v), 4)
        rec[k + "_range_s"] = [round(min(v), 4), round(max(v), 4)]
    rec["existing_keys_equal"] = all(metrics["objects"][k] == v for k, v in metrics["plain"].items())
    rec["PQ"] = metrics["objects"]["PQ"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objects_timing: needs the GPU (a timing taken elsewhere says nothing)")
    from unetseg_hip import objects

    rec = {"reps": a.reps, "pair_tile": list(objects.tile()), "maps": time_maps(a.reps)}
    if not a.no_eval:
        rec["evaluate_binary"] = time_eval(a.rounds, a.batches, a.batch)
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
