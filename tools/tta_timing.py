"""Time the two test-time-augmentation kernels beside the ATen compositions they replace.

    python tools/tta_timing.py [--batch 2] [--size 512] [--reps 30] [--inner 20] [--out profiles/tta_timing.json]

Views: ``unetseg_tta_views`` on a [B,3,S,S] batch against flip / rot90 / cat.  Merge:
``unetseg_tta_merge`` on [K*B,C,S,S] logits, C in {2, 5}, against softmax, the inverse flip / rot90,
stack, mean, log.  Modes d4 (K = 8) and hflip (K = 2).  Each figure is the median over ``reps`` of one
HIP-event window around ``inner`` back-to-back calls, divided by ``inner``, after ten warm-up calls, all
in one process, the two sides alternating.  Beside each kernel stands its byte floor: every input and
output byte once, (1 + K) B 3 S S 4 for the views and (K + 1) B C S S 4 for the merge, over 6.3 TB/s.
The outputs are compared first (views bit for bit).  A record, not a pass/fail bar.
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

HBM_BYTES_PER_S = 6.3e12


def ks(mask):
    return [k for k in range(8) if mask >> k & 1]


def aten_views(x, mask):
    return torch.cat([torch.rot90(torch.flip(x, dims=[-1]) if k & 1 else x, k >> 1, dims=(-2, -1)) for k in ks(mask)])


def aten_merge(lg, mask):
    kk = ks(mask)
    slabs = lg.view(len(kk), -1, *lg.shape[1:])
    back = []
    for s, k in zip(slabs, kk):
        p = torch.rot90(torch.softmax(s, 1), -(k >> 1), dims=(-2, -1))
        back.append(torch.flip(p, dims=[-1]) if k & 1 else p)
    return torch.stack(back).mean(0).log()


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def pair(hip, aten, reps, inner, warmup=10):
    for _ in range(warmup):
        hip()
        aten()
    th, ta = [], []
    for _ in range(reps):
        th.append(window(hip, inner))
        ta.append(window(aten, inner))

    def stat(ts):
        return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
    return stat(th), stat(ta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from unetseg_hip import tta

    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(0)
    rec = {"shape": {"B": B, "size": S}, "reps": a.reps, "inner": a.inner, "rows": []}
    for mode in ("d4", "hflip"):
        mask = tta.MODES[mode]
        K = len(ks(mask))
        x = torch.rand(B, 3, S, S, generator=g).cuda()
        assert torch.equal(tta.views(x, mask), aten_views(x, mask))
        hip, aten = pair(lambda: tta.views(x, mask), lambda: aten_views(x, mask), a.reps, a.inner)
        floor = (1 + K) * B * 3 * S * S * 4 / HBM_BYTES_PER_S * 1e6
        rec["rows"].append({"kernel": "tta_views", "mode": mode, "C": 3, "hip": hip, "aten": aten,
                            "floor_us": round(floor, 2), "floor_over_hip": round(floor / hip["median_us"], 3),
                            "aten_over_hip": round(aten["median_us"] / hip["median_us"], 2)})
        for C in (2, 5):
            lg = (8 * torch.randn(K * B, C, S, S, generator=g)).cuda()
            err = (tta.merge(lg, mask).double() - aten_merge(lg.double(), mask)).abs().max().item()
            hip, aten = pair(lambda: tta.merge(lg, mask), lambda: aten_merge(lg, mask), a.reps, a.inner)
            floor = (K + 1) * B * C * S * S * 4 / HBM_BYTES_PER_S * 1e6
            rec["rows"].append({"kernel": "tta_merge", "mode": mode, "C": C, "hip": hip, "aten": aten,
                                "floor_us": round(floor, 2), "floor_over_hip": round(floor / hip["median_us"], 3),
                                "aten_over_hip": round(aten["median_us"] / hip["median_us"], 2),
                                "max_abs_err_vs_float64_aten": err})
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
