"""Time the soft-clDice loss (csrc/cldice.hip) beside its traffic floor, and a training step with and without it.

    python tools/cldice_timing.py [--reps 20] [--iters 3] [--out profiles/cldice_timing.json] [--no-train]

Batches: [16,2,512,512] and [8,1,512,512] logits (4 randn) on the targets of utils.synthetic.make_batch.
* kernels: HIP-event windows around single C calls, median over ``reps`` after three warm-up calls.  A skeleton call
  is iters + 1 launches of one kernel, so the level-0 launch is the call at iters 0 and a later level is
  (call at iters - call at 0) / iters; the same for the backward.  The loss's elementwise launches (maps, sums,
  final, gz) are the entry point less its two forwards and its backward.
* floor: the bytes a launch must move per pixel of the batch over the copy rate measured here (a 1 GiB device copy,
  read + write).  Forward level 0: 4 + 4, later levels 8 + 8.  Backward: top level of the loss 12 + 8, a middle
  level 16 + 8, level 0 12 + 4 (through the skeleton entry point the top level reads gskel instead of y: the same).
  Entry point at iters k >= 1: maps 4 nch + 8 + 12, two forwards 2 (8 + 16 k), sums 16, backward 20 + 24 (k - 1) + 16,
  gz 12 + 4.
* training step: unet_resnet50, B = 16, 512 x 512, bf16, Lovasz hinge, eager steps with cldice_weight 0.3 and 0 in
  alternating blocks of ``--block`` steps, each block inside one event window; the medians of the blocks' ms / step.
  A weight-0 step issues the parent commit's calls (tools/record_step_calls.py), so it stands for the parent here.
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-embroidery-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

BATCHES = ((16, 2, 512), (8, 1, 512))
WARM = 3
WEIGHT = 0.3


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


def median_us(fn, reps, warmup=WARM):
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


def entry_bytes(nch, k):
    bwd = 16 if k == 0 else 20 + 24 * (k - 1) + 16
    return (4 * nch + 20) + 2 * (8 + 16 * k) + 16 + bwd + 16


def make_calls(B, nch, S, k):
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P
    from utils.synthetic import make_batch
    _, y = make_batch(B, S, seed=1234)
    tgt = y.to("cuda", torch.int64).contiguous()
    g = torch.Generator().manual_seed(B + nch)
    out = (4 * torch.randn(B, nch, S, S, generator=g)).cuda()
    gz = torch.empty(B, S * S, device="cuda")
    loss = torch.empty((), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    nb = lib.cldice_workspace(B, S, S, k)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    x = torch.sigmoid(out[:, -1] - out[:, 0] if nch == 2 else out[:, 0]).contiguous()
    gsk = torch.randn_like(x)
    skel, gx = torch.empty_like(x), torch.empty_like(x)
    sws = {i: torch.empty(max(lib.soft_skel_workspace(B, S, S, i), 16), dtype=torch.uint8, device="cuda") for i in (0, k)}

    def entry():
        lib.cldice_fwd(P(out), nch, P(tgt), B, S, S, -1, k, 1.0, 1.0, P(ws), nb, P(gz), 0, P(loss), st)

    def fwd(i):
        return lambda: lib.soft_skel_fwd(P(x), B, S, S, i, P(sws[i]), sws[i].numel(), P(skel), st)

    def bwd(i):
        return lambda: lib.soft_skel_bwd(P(x), B, S, S, i, P(sws[i]), sws[i].numel(), P(gsk), P(gx), st)

    return entry, fwd, bwd, float((tgt == 1).float().mean())


def time_training(block, rounds, k):
    """ms / step of eager unet_resnet50 B=16 512^2 bf16 steps with cldice_weight WEIGHT and 0, interleaved"""
    from model.model_factory import create_model
    from unetseg_hip.arena import FusedAdam
    from unetseg_hip.losses import binary_segmentation_loss
    from utils.synthetic import make_batch

    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        model = create_model("unet_resnet50", weights="", num_classes=2).cuda().train()
    model.compute_dtype = "bf16"
    opt = FusedAdam(model, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-4, overlap=True)
    x, y = (t.cuda() for t in make_batch(16, 512, seed=1234))

    def step(w):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = binary_segmentation_loss(model(x), y, "lovasz_hinge", cldice_weight=w, cldice_iters=k)
        loss.backward()
        opt.step()

    ms = {0.0: [], WEIGHT: []}
    for w in ms:
        for _ in range(3):
            step(w)
    for _ in range(rounds):
        for w in (WEIGHT, 0.0):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                step(w)
            e1.record()
            e1.synchronize()
            ms[w].append(e0.elapsed_time(e1) / block)
    r = lambda v: [round(min(v), 3), round(max(v), 3)]
    return {"model": "unet_resnet50", "batch": 16, "size": 512, "dtype": "bf16", "loss": "lovasz_hinge", "eager": True,
            "iters": k, "block_steps": block, "blocks": rounds,
            "weight_0_ms": round(statistics.median(ms[0.0]), 3), "weight_0_range_ms": r(ms[0.0]),
            f"weight_{WEIGHT}_ms": round(statistics.median(ms[WEIGHT]), 3), f"weight_{WEIGHT}_range_ms": r(ms[WEIGHT])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cldice_timing: needs the GPU (a timing taken elsewhere says nothing)")
    if a.iters < 1:
        raise SystemExit("cldice_timing: --iters >= 1")
    torch.cuda.set_stream(torch.cuda.Stream("cuda"))
    rate = copy_rate()
    k = a.iters
    rec = {"copy_bytes_per_s": round(rate), "reps": a.reps, "iters": k, "batches": []}
    for B, nch, S in BATCHES:
        entry, fwd, bwd, fg = make_calls(B, nch, S, k)
        px = B * S * S
        fl = lambda nbytes: nbytes * px / rate * 1e6
        f0, fk = median_us(fwd(0), a.reps), median_us(fwd(k), a.reps)
        b0, bk = median_us(bwd(0), a.reps), median_us(bwd(k), a.reps)
        us = median_us(entry, a.reps)

        def item(t, nbytes):
            return {"median_us": round(t, 1), "bytes_per_pixel": nbytes, "floor_us": round(fl(nbytes), 1),
                    "over_floor": round(t / fl(nbytes), 2)}

        row = {"logits": [B, nch, S, S], "foreground_share": round(fg, 4),
               "entry_point": item(us, entry_bytes(nch, k)),
               "skel_fwd_level_0": item(f0, 8), "skel_fwd_later_level": item((fk - f0) / k, 16),
               "skel_fwd_call": item(fk, 8 + 16 * k),
               "skel_bwd_single_level": item(b0, 12), "skel_bwd_later_level": item((bk - b0) / k, 24),
               "skel_bwd_call": item(bk, 20 + 24 * (k - 1) + 16),
               "elementwise_rest": item(us - 2 * fk - bk, (4 * nch + 20) + 16 + 16)}
        rec["batches"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_train:
        rec["training_step"] = time_training(a.block, a.rounds, k)
        print(json.dumps(rec["training_step"]), flush=True)
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
