"""Single-image / folder inference on the HIP path (reference: predict.py:32-175).

Per image, as the reference: RGB conversion, 480x480 letterbox (PIL BICUBIC resize onto a
(128,128,128) canvas), /255, eval-mode forward, softmax, crop of the letterbox window, bilinear
resize to the original size, argmax, palette colours, optional 0.3 / 0.7 blend with the original,
``<name>_mask.png`` in ``run/predict/expN``.  Here the letterbox runs in the loader's augmentation
kernels (csrc/augment.hip, bit-exact with PIL; its /255 equals the reference's float32 division for
every byte value), the model on the HIP kernels, and softmax + crop + resize + argmax is one kernel
(unetseg_softmax_resize_argmax).  The reference resizes with cv2.INTER_LINEAR (half-pixel centres,
edge clamp) and blends with cv2.addWeighted; cv2 is absent here, so the label map follows that
published rule (parity unpinned, see tests/test_gpu_predict.py) and the blend is
round-half-even of 0.3 a + 0.7 b in float32.

``--tile T`` (no reference counterpart) runs the model over the image at its native resolution
instead: overlapping T x T tiles cut on the device, batched eval-mode forwards, and the per-tile
class probabilities blended back into one map (csrc/tiles.hip, utils/tiling.py).  The default,
``--tile 0``, is the letterbox path above, unchanged.

``--tta MODE`` (no reference counterpart) wraps the loaded model in ``unetseg_hip.tta.TTA``: every
forward runs on the flips / quarter turns of its input and returns the log of the mean class
probabilities (csrc/tta.hip), which both paths take as logits.  The default, ``none``, wraps nothing.

``--min-area N`` / ``--max-hole N`` (no reference counterpart) clean the label map of either path on
the device, before the download: every connected component of a non-zero class smaller than N pixels
becomes background, then every background component smaller than N pixels that touches no image border
is filled with the class above it (csrc/ccl.hip, unetseg_hip/ccl.py).  ``--connectivity`` (8 or 4) is
that of the non-zero classes; the background takes the dual.  ``--components`` also writes
``<name>_components.json`` beside the mask: class, area and box of every component of the cleaned
map.  The defaults (0, 0, 8, off) launch nothing and leave the output as it was.

``--skeleton`` (no reference counterpart) thins the cleaned label map on the device (csrc/skeleton.hip,
unetseg_hip/skeleton.py: Guo-Hall thinning per class) and writes the centerlines to ``<name>_skeleton.png``
beside the mask, in the class colours on black; with ``--components`` every entry of the component list
gains ``skeleton_px``, the number of skeleton pixels of that component.  Off by default: nothing is launched
and the other outputs stay byte for byte what they were.

``--polygons`` (no reference counterpart) traces the outlines of the cleaned label map on the device
(csrc/contours.hip, unetseg_hip/contours.py: crack following by parallel list ranking) and writes ``<name>.json``
beside the mask, a labelme document in the reference's own annotation format (labelme_converter.py reads such
files): one polygon per component, then one ``_background_`` polygon per hole (and once more, as one exact keyhole
polygon at the end, each component of an 8-connected class that crosses a later one at a saddle), simplified
with closed-loop Douglas-Peucker at ``--polygon-epsilon`` pixels (default 1.0; 0 keeps the exact pixel outline) and labelled
from ``--class-names a,b,c`` (class 0 first) or ``class_<c>``.  With ``--components`` every entry of the component
list gains ``perimeter``, the length of the component's outlines in pixel sides.  Off by default: nothing is
launched and the other outputs stay byte for byte what they were.
"""
from __future__ import annotations

import argparse
import colorsys
import json
import os
import sys
import time
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from model.model_factory import SUPPORTED_MODELS, build_model  # noqa: E402
from unetseg_hip import ccl, contours, skeleton as skel  # noqa: E402
from unetseg_hip.lib import lib  # noqa: E402
from unetseg_hip.tta import MODES as TTA_MODES, TTA  # noqa: E402
from utils import tiling  # noqa: E402
from utils.hf_dataloader import RawSample, pack_batch  # noqa: E402
from utils.utils import cvtColor, letterbox_params  # noqa: E402

INPUT_SHAPE = (480, 480)  # predict.py:55
TILE_FILL = 128  # outside the image a tile shows the letterbox canvas grey the models were trained against
VOC_COLORS = [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128), (128, 0, 128), (0, 128, 128),
              (128, 128, 128), (64, 0, 0), (192, 0, 0), (64, 128, 0), (192, 128, 0), (64, 0, 128), (192, 0, 128),
              (64, 128, 128), (192, 128, 128), (0, 64, 0), (128, 64, 0), (0, 192, 0), (128, 192, 0), (0, 64, 128),
              (128, 64, 128)]


def time_synchronized():
    """predict.py:16-30"""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return time.time()


def colors_for(num_classes):
    """predict.py:62-70"""
    if num_classes <= 21:
        return VOC_COLORS
    hsv = [(x / num_classes, 1., 1.) for x in range(num_classes)]
    return [(int(r * 255), int(g * 255), int(b * 255)) for r, g, b in (colorsys.hsv_to_rgb(*t) for t in hsv)]


def load_model(model_name, model_path, num_classes, device):
    """predict.py:32-38 (weights_only load)"""
    net = build_model(model_name, num_classes=num_classes)
    net.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
    net.eval()
    net.to(device)
    return net


def letterbox(image, device):
    """resize_image + preprocess_input on the device: fp32 [1,3,480,480] and (nw, nh)"""
    iw, ih = image.size
    nw, nh, dx, dy = letterbox_params(iw, ih, INPUT_SHAPE[1], INPUT_SHAPE[0])
    s = RawSample(image=np.asarray(image, np.uint8), mask=np.zeros((1, 1), np.uint8), nw=nw, nh=nh, dx=dx, dy=dy,
                  flip=False, r=None)
    x = pack_batch([s], INPUT_SHAPE, 1, "binary").to_device(device, onehot=False)[0]
    return x, nw, nh


def finish_labels(labels, min_area=0, max_hole=0, connectivity=8, components=False, skeleton=False,
                  polygons=False):
    """the device label map cleaned (unetseg_hip.ccl.clean) and downloaded; with ``components`` also the
    cleaned map's component table int32 [K][7], (image, class, area, ymin, xmin, ymax, xmax); with
    ``skeleton`` the cleaned map is thinned on the device (unetseg_hip.skeleton.thin) and the skeleton map
    int32 [H][W] follows, and the table has an eighth column, the component's skeleton pixels; with
    ``polygons`` the cleaned map's outlines are traced on the device (unetseg_hip.contours.trace) and the
    component list of ``contours.polygons`` comes last"""
    labels = ccl.clean(labels, min_area, max_hole, connectivity)
    if not (skeleton or polygons):
        if components:
            return labels.cpu().numpy(), ccl.components(labels, connectivity).cpu().numpy()
        return labels.cpu().numpy()
    sk = unconverged = None
    if skeleton:
        sk, unconverged = skel.thin(labels, return_unconverged=True)
    done = (labels.cpu().numpy(),)
    if components:
        done += (ccl.components(labels, connectivity, skeleton=sk).cpu().numpy(),)
    if skeleton:
        done += (sk.cpu().numpy(),)
    if polygons:
        done += (contours.polygons(*contours.trace(labels, connectivity)),)
    if skeleton and int(unconverged.sum().item()):  # read after the downloads above: no extra wait
        raise RuntimeError(f"thinning had not converged after {skel.default_max_passes(*labels.shape[-2:])} passes")
    return done


def predict_labels(model, image, device, min_area=0, max_hole=0, connectivity=8, components=False, skeleton=False,
                   polygons=False):
    """predict.py:72-93: the argmax label map int32 [H][W] at the image's original size, cleaned as
    ``finish_labels`` says (and followed by the component table when ``components`` is set, by the
    skeleton map when ``skeleton`` is, and by the polygon list when ``polygons`` is)"""
    x, nw, nh = letterbox(image, device)
    with torch.no_grad():
        pr = model(x)[0].float().contiguous()
    C, H, W = pr.shape
    ow, oh = image.size
    labels = torch.empty(oh, ow, dtype=torch.int32, device=device)
    lib.softmax_resize_argmax(pr.data_ptr(), C, H, W, (INPUT_SHAPE[0] - nh) // 2, (INPUT_SHAPE[1] - nw) // 2, nh, nw,
                              oh, ow, labels.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    return finish_labels(labels, min_area, max_hole, connectivity, components, skeleton, polygons)


def predict_labels_tiled(model, image, device, tile=512, overlap=64, tile_batch=8, bf16=False, return_probs=False,
                         min_area=0, max_hole=0, connectivity=8, components=False, skeleton=False, polygons=False):
    """the argmax label map int32 [H][W] of the image at its native resolution: overlapping tiles
    (utils/tiling.py) gathered on the device, ``model`` (any callable [B,3,t,t] fp32 -> [B,C,t,t]
    logits, C >= 2) run over ranges of ``tile_batch`` tiles, the window-weighted softmax of every tile
    accumulated in ascending tile order and normalised, the label map cleaned as ``finish_labels`` says.
    With ``return_probs`` also the blended fp32 probabilities [C][H][W] (of the map before cleaning);
    with ``components`` the component table comes after those, with ``skeleton`` the skeleton map, and with
    ``polygons`` the polygon list last."""
    tiling.check(tile, overlap)
    rgb = np.array(image, np.uint8)  # a writable C-contiguous copy (a PIL image's buffer is read-only)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected an RGB image [H][W][3], got shape {rgb.shape}")
    H, W = rgb.shape[:2]
    nx, ny = tiling.grid(H, W, tile, overlap)
    img = torch.from_numpy(rgb).to(device)
    st = torch.cuda.current_stream(device).cuda_stream
    acc = None
    for t0, nt in tiling.ranges(nx * ny, tile_batch):
        x = torch.empty(nt, 3, tile, tile, dtype=torch.float32, device=device)
        lib.tile_gather(img.data_ptr(), H, W, tile, overlap, t0, nt, TILE_FILL, x.data_ptr(), st)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            lg = model(x)
        if lg.dim() != 4 or lg.shape[0] != nt or tuple(lg.shape[2:]) != (tile, tile):
            raise ValueError(f"the model returned {tuple(lg.shape)} for {nt} tiles of {tile}")
        C = lg.shape[1]
        if C < 2 or C > 32:
            raise ValueError(f"tiled inference blends softmax probabilities of 2..32 classes, got C={C}")
        lg = lg.float().contiguous()
        if acc is None:
            acc = torch.zeros(C, H, W, dtype=torch.float32, device=device)
        elif acc.shape[0] != C:
            raise ValueError(f"the model returned {C} classes after {acc.shape[0]}")
        lib.tile_accum(lg.data_ptr(), C, H, W, tile, overlap, t0, nt, acc.data_ptr(), st)
    labels = torch.empty(H, W, dtype=torch.int32, device=device)
    probs = torch.empty_like(acc) if return_probs else None
    lib.tile_finish(acc.data_ptr(), acc.shape[0], H, W, tile, overlap, probs.data_ptr() if return_probs else None,
                    labels.data_ptr(), st)
    done = finish_labels(labels, min_area, max_hole, connectivity, components, skeleton, polygons)
    if return_probs:
        if components or skeleton or polygons:
            return (done[0], probs.cpu().numpy()) + tuple(done[1:])
        return done, probs.cpu().numpy()
    return done


def check_tiling(tile, overlap, tile_batch=8):
    """the command line's tiling options: tile 0 = letterbox; else a multiple of 32 (the encoders halve
    the input five times) with 0 <= overlap <= tile // 2"""
    if tile == 0:
        return
    if tile < 0 or tile % 32:
        raise ValueError(f"--tile must be 0 (letterbox) or a positive multiple of 32, got {tile}")
    if overlap < 0 or overlap > tile // 2:
        raise ValueError(f"--overlap must lie in [0, tile // 2 = {tile // 2}], got {overlap}")
    if tile_batch <= 0:
        raise ValueError(f"--tile-batch must be positive, got {tile_batch}")


def check_clean(min_area, max_hole, connectivity):
    """the command line's cleanup options: thresholds >= 0 (0 = off), connectivity 4 or 8"""
    if min_area < 0:
        raise ValueError(f"--min-area must not be negative, got {min_area}")
    if max_hole < 0:
        raise ValueError(f"--max-hole must not be negative, got {max_hole}")
    if connectivity not in (4, 8):
        raise ValueError(f"--connectivity must be 4 or 8, got {connectivity}")


def check_polygons(epsilon, class_names, num_classes):
    """the command line's polygon options: epsilon >= 0; at most one name per class, class 0 included"""
    if epsilon < 0:
        raise ValueError(f"--polygon-epsilon must not be negative, got {epsilon}")
    if class_names is not None and len(class_names) > num_classes:
        raise ValueError(f"--class-names gives {len(class_names)} names for {num_classes} classes (class 0 included)")


def parse_class_names(text):
    """``a,b,c`` -> ["a", "b", "c"] (class 0 first); None or empty -> None"""
    if not text:
        return None
    return [t.strip() for t in text.split(",")]


def components_json(table, polys=None):
    """the component table as the list ``--components`` writes: class, area, bbox [x0, y0, x1, y1], in table order;
    a table with the skeleton column adds skeleton_px, and the polygon list (``contours.polygons`` of the same map
    and connectivity: the same components in the same order) adds perimeter"""
    if polys is not None and len(polys) != len(table):
        raise ValueError(f"{len(polys)} polygons for {len(table)} components")
    return [dict({"class": int(r[1]), "area": int(r[2]), "bbox": [int(r[4]), int(r[3]), int(r[6]), int(r[5])]},
                 **({"skeleton_px": int(r[7])} if len(r) > 7 else {}),
                 **({"perimeter": int(polys[k]["perimeter"])} if polys is not None else {}))
            for k, r in enumerate(table)]


def polygons_json(polys, height, width, image_path, class_names=None, epsilon=1.0):
    """the labelme document ``--polygons`` writes (``contours.labelme``); a class without a name is ``class_<c>``"""
    names = None
    if class_names is not None:
        top = max([p["class"] for p in polys], default=0)
        names = list(class_names) + [f"class_{c}" for c in range(len(class_names), top + 1)]
    return contours.labelme(polys, height, width, image_path, names, epsilon)


def blend(old, seg, alpha=0.7):
    """cv2.addWeighted(old, 1 - alpha, seg, alpha, 0) for uint8 (float32 arithmetic, round half even)"""
    f = np.float32
    v = old.astype(f) * f(1 - alpha) + seg.astype(f) * f(alpha)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def detect_image(file_path, model, num_classes, exp_folder, mix_type=True, device=None, tile=0, overlap=64,
                 tile_batch=8, bf16=False, min_area=0, max_hole=0, connectivity=8, components=False, skeleton=False,
                 polygons=False, polygon_epsilon=1.0, class_names=None):
    """predict.py:41-109; tile > 0 takes the label map from predict_labels_tiled; ``components`` writes
    the cleaned map's component list to ``<name>_components.json`` beside the mask, ``skeleton`` the cleaned
    map's centerlines to ``<name>_skeleton.png``, ``polygons`` its outlines to ``<name>.json`` (labelme)"""
    try:
        image = Image.open(file_path)
    except (FileNotFoundError, IOError) as e:
        print(f"Error opening image: {e}")
        return None
    device = device or torch.device("cuda")
    image = cvtColor(image)
    old_img = image.copy()
    # only the cleanup options that are set: without any, the two calls are what they were before cleanup existed
    post = {k: v for k, v in (("min_area", min_area), ("max_hole", max_hole), ("components", components),
                                  ("skeleton", skeleton), ("polygons", polygons)) if v}
    if post:
        post["connectivity"] = connectivity
    if tile:
        pr = predict_labels_tiled(model, image, device, tile=tile, overlap=overlap, tile_batch=tile_batch, bf16=bf16,
                                  **post)
    else:
        pr = predict_labels(model, image, device, **post)
    polys = None
    if polygons:
        pr, polys = pr[:-1], pr[-1]
        pr = pr[0] if len(pr) == 1 else pr
    if skeleton:
        table, sk_map = pr[1] if components else None, pr[-1]
        pr = pr[0]
    elif components:
        pr, table = pr
    oh, ow = pr.shape
    seg_img = np.reshape(np.array(colors_for(num_classes), np.uint8)[np.reshape(pr, [-1])], [oh, ow, -1])
    out = Image.fromarray(blend(np.array(old_img), seg_img)) if mix_type else Image.fromarray(np.uint8(seg_img))
    save_path = os.path.join(exp_folder, os.path.splitext(os.path.basename(file_path))[0] + "_mask.png")
    out.save(save_path)
    print(f"Mask saved at: {save_path}")
    if components:
        with open(save_path[:-len("_mask.png")] + "_components.json", "w") as f:
            json.dump(components_json(table, polys), f)
    if skeleton:
        palette = np.array(colors_for(num_classes), np.uint8)
        palette[0] = 0  # the background stays black whatever the palette
        Image.fromarray(palette[sk_map]).save(save_path[:-len("_mask.png")] + "_skeleton.png")
    if polygons:
        with open(save_path[:-len("_mask.png")] + ".json", "w") as f:
            json.dump(polygons_json(polys, oh, ow, os.path.basename(file_path), class_names, polygon_epsilon), f)
    return save_path


def create_val_exp_folder(root="run"):
    """utils/create_exp_folder.py:33-56: run/predict/expN (first free N >= 1)"""
    base = os.path.join(root, "predict")
    os.makedirs(os.path.join(base, "exp"), exist_ok=True)
    n = 1
    while os.path.exists(os.path.join(base, f"exp{n}")):
        n += 1
    path = os.path.join(base, f"exp{n}")
    os.mkdir(path)
    return path


def predict(args):
    """predict.py:112-145"""
    check_tiling(args.tile, args.overlap, args.tile_batch)
    check_clean(args.min_area, args.max_hole, args.connectivity)
    num_classes = args.num_classes + 1
    class_names = parse_class_names(args.class_names)
    check_polygons(args.polygon_epsilon, class_names, num_classes)
    exp_folder = create_val_exp_folder(args.out_dir)
    assert os.path.exists(args.weights), f"weights {args.weights} not found."
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP inference path needs a GPU (no CPU fallback)")
    device = torch.device("cuda")
    model = load_model(args.model, args.weights, num_classes, device)
    if args.tta != "none":  # the letterbox input and a tile are square: every mode is valid on both paths
        model = TTA(model, args.tta)
    if os.path.isdir(args.data_path):
        files = [str(p) for p in Path(args.data_path).rglob("*") if p.suffix in [".jpg", ".png", ".jpeg"]]
    elif os.path.isfile(args.data_path):
        files = [args.data_path]
    else:
        raise ValueError(f"Unsupported input path: {args.data_path}")
    t0 = time_synchronized()
    saved = [detect_image(f, model, num_classes, exp_folder, mix_type=args.mix_type, device=device, tile=args.tile,
                          overlap=args.overlap, tile_batch=args.tile_batch, bf16=args.bf16, min_area=args.min_area,
                          max_hole=args.max_hole, connectivity=args.connectivity, components=args.components,
                          skeleton=args.skeleton, polygons=args.polygons, polygon_epsilon=args.polygon_epsilon,
                          class_names=class_names)
             for f in files if f.endswith((".jpg", ".png", ".jpeg"))]
    print(f"inference time for: {time_synchronized() - t0}")
    return saved


def parse_args(argv=None):
    """predict.py:148-175"""
    p = argparse.ArgumentParser(description="U-Net predict on the MI355X HIP path")
    p.add_argument("--data_path", default="VOCdevkit/VOC2012/JPEGImages/2007_000129.jpg")
    p.add_argument("--weights", default="run/train/exp10/weights/best_model_20.pth")
    p.add_argument("--num-classes", default=20, type=int)
    p.add_argument("--model", default="unet_resnet50", choices=sorted(SUPPORTED_MODELS.keys()))
    p.add_argument("--mix_type", default=True, action="store_true")
    p.add_argument("--out-dir", default="run")
    p.add_argument("--tile", default=0, type=int,
                   help="0: letterbox to 480x480; T > 0 (a multiple of 32): native resolution in T x T tiles")
    p.add_argument("--overlap", default=64, type=int, help="pixels neighbouring tiles share (<= tile // 2)")
    p.add_argument("--tile-batch", default=8, type=int, help="tiles per forward")
    p.add_argument("--bf16", action="store_true", help="tiled path: run the forward under bf16 autocast")
    p.add_argument("--tta", default="none", choices=list(TTA_MODES),
                   help="test-time augmentation: average the class probabilities over the mirror (hflip), the "
                        "mirror and the half turn (flips) or all eight flips and quarter turns (d4) of each input")
    p.add_argument("--min-area", default=0, type=int,
                   help="components of a non-zero class smaller than this many pixels become background (0: off)")
    p.add_argument("--max-hole", default=0, type=int,
                   help="background components smaller than this many pixels that touch no image border are "
                        "filled with the class above them, after --min-area (0: off)")
    p.add_argument("--connectivity", default=8, type=int, choices=[4, 8],
                   help="of the non-zero classes; the background takes the other")
    p.add_argument("--components", action="store_true",
                   help="also write <name>_components.json: class, area and bbox [x0, y0, x1, y1] of every "
                        "component of the cleaned label map")
    p.add_argument("--skeleton", action="store_true",
                   help="also write <name>_skeleton.png: the centerlines (Guo-Hall thinning) of the cleaned label map in "
                        "the class colours on black; with --components the list gains skeleton_px per component")
    p.add_argument("--polygons", action="store_true",
                   help="also write <name>.json: the outlines of the cleaned label map as a labelme document, one "
                        "polygon per component and one _background_ polygon per hole; with --components the list "
                        "gains perimeter per component")
    p.add_argument("--polygon-epsilon", default=1.0, type=float,
                   help="Douglas-Peucker tolerance of --polygons in pixels (0: the exact pixel outline)")
    p.add_argument("--class-names", default=None,
                   help="comma-separated labels of --polygons, class 0 first (default: class_<c>)")
    return p.parse_args(argv)


if __name__ == "__main__":
    predict(parse_args())
