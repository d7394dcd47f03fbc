"""Evaluation entry point on the HIP path (reference: val.py:22-155).

Loads a state_dict (weights_only) into the named model and reports the binary metrics
(evaluate_binary: Dice / IoU / Precision / Recall / Accuracy, eps 1e-7) or, for multitask, seg
IoU / Dice (eps 1e-6) plus overall and per-class classification accuracy, or for multiclass the
reference's `evaluate` (CE + Dice loss, pixel / mean accuracy, mean / frequency-weighted IoU).
Data: the HF parquet test split (utils/hf_dataloader.py, device augmentation) or the seeded
synthetic test split (`--data-path synthetic`, binary / multitask only).

`--boundary-metrics` adds boundary precision / recall / F1 at `--boundary-tolerance` pixels, Boundary
IoU at `--boundary-iou-d` pixels and HD95 (unetseg_hip/boundary.py), printed after the usual lines.
`--skeleton-metrics` adds clDice, Skeleton Precision and Skeleton Recall on hard skeletons
(unetseg_hip/skeleton.py; `--skeleton-max-passes` caps the thinning passes), printed after those.
`--object-metrics` adds the object-level keys of unetseg_hip/objects.py on connected components of
`--object-connectivity` (after dropping predicted components below `--object-min-area` pixels): PQ, SQ, Object
F1 / Precision / Recall, Object F1@[.5:.95], Detection Recall, False Object Rate, Split Rate and Merge Rate,
printed last.

`--curve-metrics` (binary and multitask) adds the operating-point and calibration keys of
unetseg_hip/curve.py from a score histogram of `--curve-bins` bins counted on the device: the best-IoU
threshold with its IoU and F1, IoU at 0.5, AP, AUROC and ECE, and with `--threshold T` the IoU / F1 /
precision / recall at T.  It writes `curve.csv` (the confusion counts at every threshold) and
`threshold.json` into `--curve-out` (default: the experiment folder that holds the weights).

`--tta MODE` evaluates the model under flip / quarter-turn test-time augmentation
(unetseg_hip/tta.py): the metrics and the reported loss are then computed on the merged
log-probabilities, which stand in for the logits.
"""
from __future__ import annotations

import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from model.model_factory import SUPPORTED_MODELS, build_model  # noqa: E402
from unetseg_hip import losses  # noqa: E402
from unetseg_hip import curve as curve_mod  # noqa: E402
from unetseg_hip.metricset import MetricSet  # noqa: E402
from unetseg_hip.tta import MODES as TTA_MODES, TTA  # noqa: E402
from utils import metric_args  # noqa: E402
from utils.hf_dataloader import DeviceLoader, HFUnetDataset, make_collate  # noqa: E402
from utils.synthetic import SyntheticSegDataset, collate  # noqa: E402
from utils.train_and_eval import LogColor, evaluate, evaluate_binary  # noqa: E402
from utils.utils import check_loss_term_args  # noqa: E402

CLASS_NAMES = ["动物类", "植物类", "复合类"]  # val.py:84


def metric_options(args):
    """the `boundary`, `skeleton`, `curve` and `objects` arguments of the evaluate loops from the flags: the shared
    ones, and this entry point's --boundary-* and --threshold; None for a family whose flag is off"""
    opts = metric_args.metric_options(args)
    if args.boundary_metrics:
        opts["boundary"] = {"tolerance": args.boundary_tolerance, "biou_d": args.boundary_iou_d or None}
    if opts["curve"] is not None:
        opts["curve"]["threshold"] = args.threshold
    return opts


def print_keys(m, keys):
    print("\t".join(f"{LogColor.RED}{k}{LogColor.RESET}" for k in keys))
    print("\t".join(f"{m[k]:.4f}" for k in keys))


def curve_folder(args):
    """--curve-out, or the experiment folder of the weights (the parent of their `weights` folder), or the
    folder the weights lie in"""
    if args.curve_out:
        return args.curve_out
    d = os.path.dirname(os.path.abspath(args.weights))
    return os.path.dirname(d) if os.path.basename(d) == "weights" else d


def report(args, ms, m):
    """print the keys of the families that are on, and with the curve write curve.csv and threshold.json"""
    for keys in ms.keys:
        print_keys(m, keys)
    if ms.curve is not None:
        folder = curve_folder(args)
        os.makedirs(folder, exist_ok=True)
        curve_mod.write_csv(os.path.join(folder, "curve.csv"), ms.curve.table())
        curve_mod.write_threshold(os.path.join(folder, "threshold.json"), m, ms.curve.K)
    return m


def val(args):
    opts = metric_options(args)
    # the multitask loop below counts into `ms`; evaluate_binary and evaluate build a set of their own from `opts`,
    # and `ms` then names the keys to print and lends its curve accumulator, whose table is written afterwards
    ms = MetricSet(**opts)
    num_classes = args.num_classes + 1 if args.task == "multiclass" else 2  # val.py:22-27
    device = torch.device(args.device)
    input_shape = [args.input_size] * 2
    if args.data_path != "synthetic":  # val.py:31-56
        ds = HFUnetDataset(args.data_path, input_shape, num_classes, augmentation=False, split="test",
                           config=args.data_config, task="binary" if args.task == "multitask" else args.task,
                           cache_dir=args.cache_dir, return_cls_label=args.task == "multitask")
        print(f"Test samples: {len(ds)}")
        loader = DeviceLoader(DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=0,
                                         collate_fn=make_collate(ds)), device, onehot=args.task == "multiclass")
    else:
        if args.task == "multiclass":
            raise ValueError("the synthetic set is binary; the multiclass task needs a real --data-path")
        ds = SyntheticSegDataset(args.synthetic_test, input_shape, 2, seed=888_000,
                                 return_cls_label=args.task == "multitask")
        loader = DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=0, collate_fn=collate)
    if args.task == "multitask":
        model = build_model(args.model, num_classes=1, num_seg_classes=1, num_cls_classes=3)
    else:
        model = build_model(args.model, num_classes=num_classes)
    model.load_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
    model.to(device)
    print(f"Model loaded from: {args.weights}")
    if args.tta != "none":  # the loops below put the wrapper, and through it the model, in eval mode
        model = TTA(model, args.tta)

    if args.task == "binary":
        m = evaluate_binary(model, loader, device, loss_name=args.loss, pos_weight=None, ignore_index=None,
                            boundary_weight=args.boundary_loss_weight, boundary_normalize=not args.boundary_loss_pixels,
                            cldice_weight=args.cldice_weight, cldice_iters=args.cldice_iters,
                            **{**opts, "curve": ms.curve})
        print(f"{LogColor.RED}Dice{LogColor.RESET}\t{LogColor.RED}IoU{LogColor.RESET}\t{LogColor.RED}Precision"
              f"{LogColor.RESET}\t{LogColor.RED}Recall{LogColor.RESET}\t{LogColor.RED}Accuracy{LogColor.RESET}")
        print(f"{m['Dice']:.4f}\t{m['IoU']:.4f}\t{m['Precision']:.4f}\t{m['Recall']:.4f}\t{m['Accuracy']:.4f}")
        return report(args, ms, m)
    if args.task == "multiclass":
        m = evaluate(model, loader, device, dice_loss=True, focal_loss=False, num_classes=num_classes,
                     lovasz_softmax=args.loss == "lovasz_softmax",
                     **{k: v for k, v in opts.items() if k != "curve"})  # the curve is of the binary head
        print({k: v for k, v in m.items() if not any(k in keys for keys in ms.keys)})
        return report(args, ms, m)

    model.eval()
    conf = torch.zeros(4, dtype=torch.int64, device=device)
    per_cls = torch.zeros(3, 2, dtype=torch.int64, device=device)  # [class][correct, count]
    with torch.no_grad():
        for images, seg_t, _, cls_t in loader:
            images, seg_t, cls_t = images.to(device), seg_t.to(device), cls_t.to(device)
            seg_logits, cls_logits = model(images)
            losses.binary_confusion(seg_logits, seg_t, conf)
            ms.add(seg_logits, seg_t)
            pred = cls_logits.argmax(1)
            for c in range(3):
                sel = cls_t == c
                per_cls[c, 0] += (pred[sel] == c).sum()
                per_cls[c, 1] += sel.sum()
    tp, fp, fn, _ = (float(v) for v in conf.tolist())
    iou = tp / (tp + fp + fn + 1e-6)
    dice = 2 * tp / ((tp + fp) + (tp + fn) + 1e-6)
    pc = per_cls.tolist()
    acc = 100.0 * sum(c for c, _ in pc) / max(sum(n for _, n in pc), 1)
    print("=" * 50)
    print(f"Segmentation: IoU {iou:.4f}  Dice {dice:.4f}")
    print(f"Classification: overall accuracy {acc:.2f}%")
    for name, (c, n) in zip(CLASS_NAMES, pc):
        if n:
            print(f"    {name}: {100.0 * c / n:.2f}% ({n} samples)")
    print("=" * 50)
    m = {"IoU": iou, "Dice": dice, "Cls Acc": acc}
    m.update(ms.metrics())
    return report(args, ms, m)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="U-Net evaluation on the MI355X HIP path")
    p.add_argument("--data-path", default="./hf_datasets/merged_dataset_v2",
                   help="HF parquet dataset directory, or 'synthetic' (the seeded synthetic test split)")
    p.add_argument("--data-config", default="no-ai", choices=["full", "no-ai", "sam3"])
    p.add_argument("--weights", default="weights/unet_resnet_voc.pth")
    p.add_argument("--task", default="binary", choices=["binary", "multiclass", "multitask"])
    p.add_argument("--model", default="unet_resnet50", choices=sorted(SUPPORTED_MODELS.keys()))
    # val.py:176: ce / focal are accepted; the binary evaluation then refuses them as the reference's
    # binary_segmentation_loss does (ValueError "Unsupported loss_name")
    # lovasz_softmax: the multiclass evaluation reports Lovasz-softmax + Dice as its loss instead of CE + Dice
    p.add_argument("--loss", default="lovasz_hinge", choices=["bce", "lovasz_hinge", "ce", "focal", "lovasz_softmax"])
    p.add_argument("--num-classes", default=4, type=int)
    p.add_argument("--device", default="cuda")
    p.add_argument("--input-size", default=512, type=int)
    p.add_argument("--batch-size", default=1, type=int)
    p.add_argument("--cache-dir", default=".hf-cache/datasets")
    p.add_argument("--synthetic-test", default=16, type=int)
    p.add_argument("--tta", default="none", choices=list(TTA_MODES),
                   help="test-time augmentation: average the probabilities over the mirror (hflip), the mirror and "
                        "the half turn (flips) or all eight flips and quarter turns (d4); the reported loss is then "
                        "computed on the merged log-probabilities, not on the model's logits")
    p.add_argument("--boundary-metrics", action="store_true",
                   help="also report boundary precision / recall / F1, Boundary IoU and HD95 (class 1; multiclass: "
                        "the mean over the classes with a target edge)")
    p.add_argument("--boundary-tolerance", default=2.0, type=float,
                   help="pixel tolerance of boundary precision / recall / F1")
    p.add_argument("--boundary-iou-d", default=0, type=int,
                   help="Boundary-IoU band width in pixels; 0 = 2 %% of the image diagonal")
    metric_args.add_metric_args(p)
    p.add_argument("--threshold", default=None, type=float,
                   help="with --curve-metrics: also report IoU / F1 / precision / recall at this probability "
                        "threshold, a multiple of 1 / --curve-bins")
    p.add_argument("--curve-out", default="",
                   help="folder of curve.csv and threshold.json; default: the experiment folder that holds --weights")
    p.add_argument("--boundary-loss-weight", default=0.0, type=float,
                   help="the training run's boundary-loss weight, so the reported loss (m['Loss'], --task binary) is "
                        "that objective; the multitask evaluation reports no loss")
    p.add_argument("--boundary-loss-pixels", action="store_true",
                   help="boundary loss in pixel units instead of fractions of the image diagonal")
    p.add_argument("--cldice-weight", default=0.0, type=float,
                   help="the training run's soft-clDice weight, so the reported loss (--task binary) is that objective")
    p.add_argument("--cldice-iters", default=3, type=int, help="levels of the soft skeleton (0 .. 64)")
    args = p.parse_args(argv)
    metric_args.check_metric_args(p, args, metric_options)
    if args.threshold is not None and not args.curve_metrics:
        p.error("--threshold needs --curve-metrics")
    check_loss_term_args(p, args)
    return args


if __name__ == "__main__":
    val(parse_args())
