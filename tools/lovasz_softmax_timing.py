"""Time the Lovasz-softmax loss (forward + backward) beside the binary Lovasz hinge and CE + Dice.

    python tools/lovasz_softmax_timing.py [--batch 8] [--classes 5] [--size 512] [--reps 50]
                                          [--out profiles/lovasz_softmax_timing.json]

Each figure is the median of ``reps`` HIP-event timings after ten warm-up calls, all in one process:
the Lovasz-softmax in both modes (and its value-only forward, which skips the dL/dp scatter and the
Jacobian pass), the hinge at twice the batch, and the existing CE + Dice pair.  Both Lovasz paths run
the same four radix passes, so the time per sorted key is the figure to compare.  A record, not a
pass/fail bar.
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


def events(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unetseg_hip import losses

    B, C, S = a.batch, a.classes, a.size
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, C, S, S, generator=g) * 2).cuda().requires_grad_(True)
    t = torch.randint(0, C + 1, (B, S, S), generator=g).cuda()
    oh = torch.eye(C + 1, device="cuda")[t.reshape(-1)].reshape(B, S, S, C + 1)
    w = torch.ones(C, device="cuda")
    xb = (torch.randn(2 * B, 2, S, S, generator=g) * 2).cuda().requires_grad_(True)
    tb = torch.randint(0, 2, (2 * B, S, S), generator=g).cuda()

    def fwd_bwd(fn, leaf):
        def run():
            leaf.grad = None
            fn().backward()
        return run

    def value_only(per_image):
        def run():
            with torch.no_grad():
                losses.lovasz_softmax_loss(x, t, C, per_image)
        return run

    rec = {"shape": {"B": B, "C": C, "size": S}, "reps": a.reps}
    keys = B * C * S * S
    for name, per_image in (("lovasz_softmax_per_image", True), ("lovasz_softmax_batch", False)):
        r = events(fwd_bwd(lambda: losses.lovasz_softmax_loss(x, t, C, per_image), x), a.reps)
        r["keys"] = keys
        r["ns_per_key"] = round(r["median_ms"] * 1e6 / keys, 4)
        r["value_only"] = events(value_only(per_image), a.reps)
        rec[name] = r
    hk = 2 * B * S * S
    r = events(fwd_bwd(lambda: losses.binary_segmentation_loss(xb, tb, "lovasz_hinge"), xb), a.reps)
    r["keys"] = hk
    r["ns_per_key"] = round(r["median_ms"] * 1e6 / hk, 4)
    rec["lovasz_hinge_2B"] = r
    rec["ce_plus_dice"] = events(fwd_bwd(lambda: losses.ce_loss(x, t, w, C) + losses.dice_loss(x, oh), x), a.reps)
    for k in ("lovasz_softmax_per_image", "lovasz_softmax_batch"):
        rec[k]["per_key_vs_hinge"] = round(rec[k]["ns_per_key"] / rec["lovasz_hinge_2B"]["ns_per_key"], 3)
    try:
        rec["commit"] = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        rec["commit"] = None
    rec["device"] = torch.cuda.get_device_name(0)
    out = json.dumps(rec, indent=1)
    print(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
