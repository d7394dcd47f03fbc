"""Time the score histogram (csrc/curve.hip, unetseg_curve_hist) beside unetseg_confusion_masked on the same tensors.

    python tools/curve_timing.py [--rounds 9] [--inner 50] [--bins 1000] [--out profiles/curve_timing.json]

Shapes [16,2,512,512] and [8,1,512,512], int64 targets, ignore_index 255 with no pixel ignored (both kernels make
the comparison).  Three score distributions:
* uniform: logits of probabilities drawn uniformly from (0, 1): every bin of the histogram is hit equally, so this
  is the most LDS adds and the most global atomics at the flush;
* normal: N(0, 1) logits;
* saturated: a disc of 5 % of each image at +12 on a -12 ground, blurred with a 5 x 5 box so that its rim spreads
  over the middle bins: about 95 % / 5 % of the pixels in the two end bins, what a trained model produces.
Timing: a HIP-event window around ``inner`` back-to-back calls, divided by ``inner``; ``rounds`` such windows per
kernel, the two kernels alternating, after a warm-up window of each; median and range over the rounds.  The tensors
of the large shape are 67 MB and the small one's 25 MB: back-to-back calls may find them in the 256 MB last-level
cache, the same for both kernels.  ``floor_us`` is the bytes a call must read (4 nch + 8 per pixel) over the
copy rate of a 1 GiB device copy (tools/hbm_bw.py's first figure, read + write), which does not fit that cache.
``ratio`` = curve_hist / confusion_masked, the figure to watch: confusion_masked reads the same bytes and keeps
four counters.  A record, not a pass/fail bar.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from cldice_timing import copy_rate  # noqa: E402  (tools/ is the script's directory)

IGNORE = 255


def scores(kind, B, S, gen):
    """(z fp32 [B,S,S], target int64 [B,S,S]) on the GPU"""
    if kind == "uniform":
        p = torch.rand(B, S, S, generator=gen, device="cuda").clamp_(1e-6, 1 - 1e-6)
        z = torch.log(p / (1 - p))
    elif kind == "normal":
        z = torch.randn(B, S, S, generator=gen, device="cuda")
    else:
        r = math.sqrt(0.05 / math.pi) * S
        yy, xx = torch.meshgrid(torch.arange(S, device="cuda"), torch.arange(S, device="cuda"), indexing="ij")
        cy = torch.randint(int(r) + 3, S - int(r) - 3, (B, 1, 1), generator=gen, device="cuda")
        cx = torch.randint(int(r) + 3, S - int(r) - 3, (B, 1, 1), generator=gen, device="cuda")
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        hard = torch.where(disc, 12.0, -12.0)
        z = torch.nn.functional.avg_pool2d(hard.unsqueeze(1), 5, 1, 2, count_include_pad=False)[:, 0]
        return z.contiguous(), disc.to(torch.int64).contiguous()
    tgt = (torch.rand(B, S, S, generator=gen, device="cuda") < torch.sigmoid(z)).to(torch.int64)
    return z.contiguous(), tgt.contiguous()


def window_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def stats(ts):
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}


def time_case(kind, B, nch, S, K, rounds, inner, rate, gen):
    from unetseg_hip import curve
    from unetseg_hip.lib import lib

    z, tgt = scores(kind, B, S, gen)
    out = z.unsqueeze(1) if nch == 1 else torch.stack([-0.5 * z, 0.5 * z], 1)  # o1 - o0 = z exactly
    out = out.contiguous()
    P = S * S
    edges = curve.edges(K, out.device)
    hist = torch.zeros(2, K, dtype=torch.int64, device="cuda")
    conf = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    arms = {"curve_hist": lambda: lib.curve_hist(out.data_ptr(), nch, tgt.data_ptr(), B, P, IGNORE, edges.data_ptr(), K,
                                                 hist.data_ptr(), st),
            "confusion_masked": lambda: lib.confusion_masked(out.data_ptr(), nch, tgt.data_ptr(), B, P, IGNORE,
                                                             conf.data_ptr(), st)}
    ts = {k: [] for k in arms}
    for r in range(rounds + 1):  # the first round warms up
        for k, fn in arms.items():
            t = window_us(fn, inner)
            if r:
                ts[k].append(t)
    calls = (rounds + 1) * inner
    h = hist.cpu()
    assert int(h.sum()) == calls * B * P and int(conf.sum()) == calls * B * P  # both counted every pixel of every call
    one = h // calls
    ends = int(one[:, 0].sum() + one[:, -1].sum())
    nbytes = B * P * (4 * nch + 8)
    row = {"scores": kind, "shape": [B, nch, S, S], "bins": K, "end_bin_share": round(ends / (B * P), 4),
           "bins_hit": int((one.sum(0) > 0).sum()), "bytes": nbytes, "floor_us": round(nbytes / rate * 1e6, 2),
           "curve_hist": stats(ts["curve_hist"]), "confusion_masked": stats(ts["confusion_masked"])}
    row["ratio"] = round(row["curve_hist"]["median_us"] / row["confusion_masked"]["median_us"], 3)
    row["curve_hist_over_floor"] = round(row["curve_hist"]["median_us"] / row["floor_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--bins", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curve_timing: needs the GPU (a timing taken elsewhere says nothing)")
    rate = copy_rate()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    rows = []
    for B, nch in ((16, 2), (8, 1)):
        for kind in ("uniform", "normal", "saturated"):
            rows.append(time_case(kind, B, nch, 512, a.bins, a.rounds, a.inner, rate, gen))
            print(json.dumps(rows[-1]), flush=True)
    rec = {"copy_bytes_per_s": round(rate), "rounds": a.rounds, "inner": a.inner, "cases": rows}
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
