"""The flags of the optional evaluation metrics that train.py and val.py share, their checks, and the option dicts
the evaluate loops (utils/train_and_eval.py) and unetseg_hip.metricset.MetricSet take."""
from unetseg_hip.curve import Accumulator as CurveAccumulator


def add_metric_args(p):
    p.add_argument("--skeleton-metrics", action="store_true",
                   help="also report clDice, Skeleton Precision and Skeleton Recall on hard (thinned) skeletons (class "
                        "1; multiclass: the mean over the classes with a target skeleton)")
    p.add_argument("--skeleton-max-passes", default=None, type=int,
                   help="cap of the thinning passes; default min(H, W) // 2 + 8.  An image still losing pixels at the "
                        "cap is an error, not a silently wrong score")
    p.add_argument("--curve-metrics", action="store_true",
                   help="also report the best-IoU threshold with its IoU and F1, IoU at 0.5, AP, AUROC and ECE of the "
                        "binary head from a score histogram (--task binary and multitask)")
    p.add_argument("--curve-bins", default=1000, type=int,
                   help="bins K of the score histogram (even, a multiple of 10, at most 4096); threshold k stands for "
                        "probability k / K")
    p.add_argument("--object-metrics", action="store_true",
                   help="also report PQ, SQ, Object F1 / Precision / Recall, Object F1@[.5:.95], Detection Recall, "
                        "False Object Rate, Split Rate and Merge Rate of the connected components (class 1; "
                        "multiclass: the mean over the classes with a target object)")
    p.add_argument("--object-connectivity", default=8, type=int, choices=[4, 8],
                   help="connectivity of the objects of --object-metrics")
    p.add_argument("--object-min-area", default=0, type=int,
                   help="with --object-metrics: drop predicted components below this area first, as predict.py "
                        "--min-area does")


def metric_options(args):
    """the `boundary`, `skeleton`, `curve` and `objects` arguments of the evaluate loops from the shared flags: a
    family's options dict, or None when its flag is off (no shared flag turns the boundary metrics on)"""
    return {"boundary": None,
            "skeleton": {"max_passes": args.skeleton_max_passes} if args.skeleton_metrics else None,
            "curve": {"bins": args.curve_bins} if args.curve_metrics else None,
            "objects": {"connectivity": args.object_connectivity, "min_area": args.object_min_area}
            if args.object_metrics else None}


def check_metric_args(p, args, options=metric_options):
    """p.error on what the shared flags must not be; `options`: the entry point's own `metric_options`, when it adds
    to the dicts"""
    if args.skeleton_max_passes is not None and args.skeleton_max_passes < 0:
        p.error("--skeleton-max-passes must be >= 0")
    if args.object_min_area < 0:
        p.error("--object-min-area must be >= 0")
    if args.curve_metrics:
        if args.task == "multiclass":
            p.error("--curve-metrics needs --task binary or multitask (one-vs-rest softmax scores are out of scope)")
        try:
            CurveAccumulator(options(args)["curve"])
        except ValueError as e:
            p.error(f"--curve-metrics: {e}")
