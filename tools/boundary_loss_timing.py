"""Time the boundary loss (csrc/boundary_loss.hip) beside its traffic floor, and a training step with and without it.

    python tools/boundary_loss_timing.py [--reps 20] [--out profiles/boundary_loss_timing.json]
                                         [--passes-from DIR] [--no-train]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/boundary_loss_timing.py --kernels-only

Batches: [16,2,512,512] and [8,1,512,512] logits (4 randn) on the targets of utils.synthetic.make_batch.
* entry point: the median over ``reps`` of one HIP-event window around one unetseg_boundary_loss_fwd call (gz
  written, no phi), after three warm-up calls; beside it unetseg_edt_sqdist alone on the same 2 B site maps.
* passes: the entry point is one C call, so the time of each of its launches comes from a kernel trace taken in a
  run of its own (second command line above; ``--kernels-only`` issues the same calls and times nothing) and read
  back with ``--passes-from DIR``: per kernel the median of the last ``reps`` launches of each batch.
* floor: the bytes a pass must move per pixel of the batch over the copy rate measured here (a 1 GiB device
  copy, read + write): sites 8 + 2; the transform over both site maps 2 x 13 (tools/boundary_timing.py's count:
  a column pass 1 + 4 and a row pass 4 + 4; its launches are listed with what they move themselves, 2 x 5, 2 x 8 and
  2 x 8); loss 4 nch + 8 + 8 + 4.
* training step: unet_resnet50, B = 16, 512 x 512, bf16, Lovasz hinge, eager steps with weight 0.01 and weight 0 in
  alternating blocks of ``--block`` steps, each block inside one event window; the medians of the blocks' ms / step.
A record, not a pass/fail bar.
"""
import argparse
import contextlib
import csv
import glob
import io
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

BATCHES = ((16, 2, 512), (8, 1, 512))
WARM = 3
#: kernel-name fragment -> bytes per pixel of the batch the launch moves
PASSES = {"bl_sites_kernel": 10, "bl_count_kernel": 0, "edt_col_local_kernel": 10, "edt_col_merge_kernel": 16,
          "edt_row_kernel": 16, "bl_loss_kernel": None, "bl_final_kernel": 0}


def loss_bytes(nch):
    return 4 * nch + 8 + 8 + 4


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


def make_call(B, nch, S):
    """() -> one unetseg_boundary_loss_fwd call on a synthetic batch, its buffers allocated once"""
    from unetseg_hip.lib import lib
    from unetseg_hip.ops import P
    from utils.synthetic import make_batch
    _, y = make_batch(B, S, seed=1234)
    tgt = y.to("cuda", torch.int64).contiguous()
    g = torch.Generator().manual_seed(B + nch)
    out = (4 * torch.randn(B, nch, S, S, generator=g)).cuda()
    gz = torch.empty(B, S * S, device="cuda")
    loss = torch.empty((), device="cuda")
    nb = lib.boundary_loss_workspace(B, S, S)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    inv = 1.0 / math.sqrt(2 * S * S)

    def call():
        lib.boundary_loss_fwd(P(out), nch, P(tgt), B, S, S, 1, -1, inv, 1.0, P(ws), nb, P(gz), 0, None, P(loss), st)

    sites = torch.cat([tgt == 1, tgt != 1]).to(torch.uint8).contiguous()
    d2 = torch.empty(2 * B, S, S, dtype=torch.int32, device="cuda")

    def edt():
        lib.edt_sqdist(P(sites), 2 * B, S, S, P(d2), st)

    return call, edt, float((tgt == 1).float().mean())


def read_passes(dirname, reps):
    """per batch: kernel -> median us of its last `reps` launches, from a rocprofv3 kernel trace of --kernels-only"""
    files = glob.glob(os.path.join(dirname, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {dirname}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    out = []
    per_batch = WARM + reps
    for i, _ in enumerate(BATCHES):
        rec = {}
        for frag in PASSES:
            d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if frag in r["Kernel_Name"]]
            if len(d) != per_batch * len(BATCHES):
                raise SystemExit(f"{frag}: {len(d)} launches in the trace, expected {per_batch * len(BATCHES)}")
            rec[frag] = statistics.median(d[i * per_batch + WARM:(i + 1) * per_batch])
        out.append(rec)
    return out


def time_training(block, rounds):
    """ms / step of eager unet_resnet50 B=16 512^2 bf16 steps with boundary_weight 0.01 and 0, interleaved"""
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
            loss = binary_segmentation_loss(model(x), y, "lovasz_hinge", boundary_weight=w)
        loss.backward()
        opt.step()

    ms = {0.0: [], 0.01: []}
    for w in ms:
        for _ in range(3):
            step(w)
    for _ in range(rounds):
        for w in (0.01, 0.0):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                step(w)
            e1.record()
            e1.synchronize()
            ms[w].append(e0.elapsed_time(e1) / block)
    return {"model": "unet_resnet50", "batch": 16, "size": 512, "dtype": "bf16", "loss": "lovasz_hinge", "eager": True,
            "block_steps": block, "blocks": rounds,
            "weight_0_ms": round(statistics.median(ms[0.0]), 3), "weight_0_range_ms": [round(min(ms[0.0]), 3), round(max(ms[0.0]), 3)],
            "weight_0.01_ms": round(statistics.median(ms[0.01]), 3),
            "weight_0.01_range_ms": [round(min(ms[0.01]), 3), round(max(ms[0.01]), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="issue the calls and time nothing (for a kernel trace)")
    ap.add_argument("--passes-from", default=None, help="directory of that trace: adds the per-pass times")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_loss_timing: needs the GPU (a timing taken elsewhere says nothing)")
    torch.cuda.set_stream(torch.cuda.Stream("cuda"))
    if a.kernels_only:
        for B, nch, S in BATCHES:
            call, _, _ = make_call(B, nch, S)
            for _ in range(WARM + a.reps):
                call()
            torch.cuda.synchronize()
        return
    rate = copy_rate()
    passes = read_passes(a.passes_from, a.reps) if a.passes_from else None
    rec = {"copy_bytes_per_s": round(rate), "reps": a.reps, "batches": []}
    for i, (B, nch, S) in enumerate(BATCHES):
        call, edt, fg = make_call(B, nch, S)
        px = B * S * S
        total_b = 10 + 26 + loss_bytes(nch)
        us, us_edt = median_us(call, a.reps), median_us(edt, a.reps)
        row = {"logits": [B, nch, S, S], "foreground_share": round(fg, 4),
               "entry_point": {"median_us": round(us, 1), "bytes_per_pixel": total_b,
                               "floor_us": round(total_b * px / rate * 1e6, 1),
                               "over_floor": round(us / (total_b * px / rate * 1e6), 1)},
               "edt_sqdist_2B_alone": {"median_us": round(us_edt, 1), "bytes_per_pixel": 26,
                                       "floor_us": round(26 * px / rate * 1e6, 1),
                                       "over_floor": round(us_edt / (26 * px / rate * 1e6), 1)}}
        if passes is not None:
            row["passes"] = {}
            for frag, nbytes in PASSES.items():
                nbytes = loss_bytes(nch) if nbytes is None else nbytes
                floor = nbytes * px / rate * 1e6
                row["passes"][frag] = {"median_us": round(passes[i][frag], 1), "bytes_per_pixel": nbytes,
                                       "floor_us": round(floor, 1),
                                       "over_floor": round(passes[i][frag] / floor, 1) if floor else None}
        rec["batches"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_train:
        rec["training_step"] = time_training(a.block, a.rounds)
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
