"""Time predict.predict_labels_tiled against the letterbox predict.predict_labels on one synthetic image.

    python tools/predict_tiled_timing.py [--size 2048] [--model unet_resnet50] [--tile 512] [--overlap 64]
                                         [--tile-batch 8] [--reps 5] [--out profiles/<name>.json]

Each figure is the median wall time of ``reps`` calls after two warm-up calls, image upload and label
download included (what a caller of the function waits for); the three tile kernels are also timed
alone with HIP events on the tiles of the same image (C = the model's class count).  The record
carries the commit and the card's clocks under load.  A record for later work, not a pass/fail bar.
"""
import argparse
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

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def wall(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def events(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--model", default="unet_resnet50")
    ap.add_argument("--num-classes", type=int, default=2)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import predict
    from bench import card_state
    from model.model_factory import build_model
    from unetseg_hip.lib import lib
    from utils import tiling

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = build_model(a.model, num_classes=a.num_classes).to(dev).eval()
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:a.size, 0:a.size]
    arr = np.stack([xx * 255 // (a.size - 1), yy * 255 // (a.size - 1), (xx + yy) * 7 % 256], -1)
    arr = np.clip(arr + rng.integers(-40, 40, arr.shape), 0, 255).astype(np.uint8)
    image = Image.fromarray(arr)
    kw = dict(tile=a.tile, overlap=a.overlap, tile_batch=a.tile_batch)

    res = {"image": f"{a.size}x{a.size} synthetic RGB", "model": a.model, "num_classes": a.num_classes, **kw,
           "tiles": list(tiling.grid(a.size, a.size, a.tile, a.overlap)), "reps": a.reps}
    res["tiled_fp32"] = wall(lambda: predict.predict_labels_tiled(model, image, dev, **kw), a.reps)
    res["card_under_load"] = card_state(dev)
    res["tiled_bf16"] = wall(lambda: predict.predict_labels_tiled(model, image, dev, bf16=True, **kw), a.reps)
    res["letterbox_480"] = wall(lambda: predict.predict_labels(model, image, dev), a.reps)

    # the tile kernels alone, over the whole image in ranges of tile_batch
    H = W = a.size
    C, t, o = a.num_classes, a.tile, a.overlap
    nx, ny = tiling.grid(H, W, t, o)
    st = torch.cuda.current_stream(dev).cuda_stream
    img = torch.from_numpy(arr).to(dev)
    rngs = tiling.ranges(nx * ny, a.tile_batch)
    x = torch.empty(a.tile_batch, 3, t, t, device=dev)
    lg = torch.randn(a.tile_batch, C, t, t, device=dev)
    acc = torch.zeros(C, H, W, device=dev)
    probs, labels = torch.empty_like(acc), torch.empty(H, W, dtype=torch.int32, device=dev)
    res["kernels_ms"] = {
        "gather_all_tiles": events(lambda: [lib.tile_gather(img.data_ptr(), H, W, t, o, t0, nt, 128, x.data_ptr(), st)
                                            for t0, nt in rngs], a.reps),
        "accum_all_tiles": events(lambda: [lib.tile_accum(lg.data_ptr(), C, H, W, t, o, t0, nt, acc.data_ptr(), st)
                                           for t0, nt in rngs], a.reps),
        "finish_labels_only": events(lambda: lib.tile_finish(acc.data_ptr(), C, H, W, t, o, None, labels.data_ptr(),
                                                             st), a.reps),
        "finish_with_probs": events(lambda: lib.tile_finish(acc.data_ptr(), C, H, W, t, o, probs.data_ptr(),
                                                            labels.data_ptr(), st), a.reps),
    }
    try:
        res["commit"] = subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    res["device"] = torch.cuda.get_device_name(dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
