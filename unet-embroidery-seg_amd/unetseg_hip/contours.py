"""Vector contours of class maps on the HIP path (csrc/contours.hip), and their way into a labelme document.

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU; class 0 is background; components and roots are those
of ``ccl.label(cls, connectivity)``.  Pixel (y, x) covers the square [x, x+1] x [y, y+1] and a lattice corner is
(x, y) with 0 <= x <= W, 0 <= y <= H.  A *crack* is a side of a pixel of a non-zero class whose 4-neighbour across
it has another class or lies outside the image; cracks run clockwise on screen (the owner on the right of travel)
and have the id ``(y * W + x) * 4 + side`` (0 top, 1 right, 2 bottom, 3 left).  At a crack's head corner the trace
turns towards the pixel ahead on the far side where the class is 8-connected and that pixel has the owner's class,
else goes straight on where the pixel ahead on the owner's side has it, else turns right round the owner; a
4-connected class prefers the right turn instead (the two differ at a 2 x 2 saddle only).  That successor map is a
bijection, so the cracks fall into closed loops.  A loop's *leader* is its smallest crack id; it is the outer loop
of its component iff ``leader == 4 * root``, every other loop is a hole.  A *vertex* is the tail corner of a crack
whose direction differs from its predecessor's.

``trace`` returns the loops and their vertices as device tensors; ``polygons``, ``simplify`` and ``labelme`` are
host code on that small result.  Everything is integer and a function of the input only.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import ccl
from .classmap import _map, _stream
from .lib import lib

#: columns of a ``loops`` row
LOOP_COLUMNS = ("image", "class", "root", "hole", "first", "count", "area", "cracks")
#: pixels of one image the kernels take: crack ids stay below 2^31
MAX_PIXELS = 1 << 29
LABELME_VERSION = "5.0.1"
BACKGROUND = "_background_"


def tile():
    """(tw, th): a block of the crack-mask kernel holds a tile of this size, and its one-pixel halo, in LDS"""
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    lib.contours_tile(ctypes.addressof(tw), ctypes.addressof(th))
    return tw.value, th.value


def workspace_bytes(M):
    """bytes of the workspace of ``M`` cracks (it scales with the cracks, not with the pixels)"""
    return lib.contours_workspace(int(M))


def _layout(M):
    at = (ctypes.c_int64 * 8)()
    lib.contours_layout(int(M), ctypes.addressof(at))
    return [int(v) for v in at]


def _empty(device):
    return (torch.zeros(0, 8, dtype=torch.int32, device=device), torch.zeros(0, 2, dtype=torch.int32, device=device))


def trace(cls, connectivity=8):
    """(loops int32 [L,8], vertices int32 [V,2]) on the device.  A ``loops`` row is (image, class, root, hole, first,
    count, area, cracks): ``vertices[first:first + count]`` are the loop's corners (x, y) in travel order from the
    first vertex at or after the leader's tail, ``area`` its signed shoelace area (positive for an outer loop,
    negative for a hole) and ``cracks`` its length in pixel sides.  Loops are ordered by (image, root, leader): a
    component's outer loop, then its holes.  The host reads two sizes (the crack count, then L and V); the rest
    runs on the current stream.  An empty batch launches nothing."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    c = _map(cls)
    N, H, W = c.shape
    dev = c.device
    if c.numel() == 0:
        return _empty(dev)
    if H * W > MAX_PIXELS:
        raise ValueError(f"contours: H * W = {H} * {W} exceeds the 2^29 pixels of one image")
    st = _stream(c)
    segs_x = (W + 63) // 64
    mask = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    seg = torch.empty(N * H * segs_x, dtype=torch.int32, device=dev)
    lib.contours_mask(c.data_ptr(), N, H, W, mask.data_ptr(), seg.data_ptr(), st)
    ends = torch.cumsum(seg, 0, dtype=torch.int64)  # crack-id order: a segment is 64 pixels of one row
    M = int(ends[-1].item())  # the first host read
    if M == 0:
        return _empty(dev)
    if M > 2**31 - 1:
        raise ValueError(f"contours: {M} cracks in the batch exceed the 2^31 - 1 that dense indices hold")
    size = workspace_bytes(M)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    base = ends - seg
    off = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    lib.contours_link(c.data_ptr(), mask.data_ptr(), base.data_ptr(), N, H, W, connectivity, M, off.data_ptr(),
                      ws.data_ptr(), size, st)
    del off, base, ends, seg
    lib.contours_rank(N, H, W, M, ws.data_ptr(), size, st)
    a_gid, a_lead, a_nv, a_fail = (_layout(M)[k] for k in (0, 3, 5, 7))
    gid = ws[a_gid:a_gid + 8 * M].view(torch.int64)
    lead = ws[a_lead:a_lead + 4 * M].view(torch.int32)
    nv = ws[a_nv:a_nv + 4 * M].view(torch.int32)
    is_leader = lead == torch.arange(M, dtype=torch.int32, device=dev)
    fail = ws[a_fail:a_fail + 4].view(torch.int32)
    sizes = torch.stack([is_leader.sum(), (nv * is_leader).sum(), fail[0].long()]).tolist()  # the second host read
    L, V, failed = sizes
    if failed:
        raise RuntimeError(f"contours: {failed} cracks found no successor among the cracks, which is a bug")
    # the leaders in ascending dense order, which is (image, leader) order; no host read: the size is known
    slot = torch.where(is_leader, torch.cumsum(is_leader, 0) - 1, L)
    leaders = torch.empty(L + 1, dtype=torch.int64, device=dev).scatter_(
        0, slot, torch.arange(M, dtype=torch.int64, device=dev))[:L]
    del slot, is_leader
    root = ccl.label(c, connectivity).view(-1)
    pix = gid[leaders] >> 2  # the leader's pixel in the flat batch
    comp = pix // (H * W) * (H * W) + root[pix].long()  # (image, root) as one ascending key
    order = torch.sort(comp, stable=True).indices  # ties keep the leader order
    leaders = leaders[order].to(torch.int32)
    count = nv[leaders.long()]
    first = (torch.cumsum(count, 0, dtype=torch.int64) - count).to(torch.int32)
    loops = torch.empty(L, 8, dtype=torch.int32, device=dev)
    vertices = torch.empty(V, 2, dtype=torch.int32, device=dev)
    lib.contours_emit(c.data_ptr(), root.data_ptr(), N, H, W, M, leaders.data_ptr(), first.data_ptr(), L,
                      loops.data_ptr(), vertices.data_ptr(), V, ws.data_ptr(), size, st)
    return loops, vertices


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def polygons(loops, vertices):
    """host list, one entry per component in table order: ``{image, class, root, outer: [[x, y], ...], holes:
    [[[x, y], ...], ...], area, perimeter}``; ``area`` is the sum of the signed areas of the component's loops (its
    pixels), ``perimeter`` the sum of their ``cracks``"""
    loops, vertices = _host(loops), _host(vertices)
    out = []
    for image, c, root, hole, first, count, area, cracks in loops.tolist():
        pts = vertices[first:first + count].tolist()
        if not hole:
            out.append({"image": image, "class": c, "root": root, "outer": pts, "holes": [], "area": 0,
                        "perimeter": 0})
        p = out[-1]
        if p["image"] != image or p["root"] != root:
            raise ValueError("loops are not ordered by (image, root, leader): a hole precedes its outer loop")
        if hole:
            p["holes"].append(pts)
        p["area"] += area
        p["perimeter"] += cracks
    return out


def _seg_dist(p, a, b):
    """distances of the points p [K,2] from the segment a b"""
    ab = b - a
    den = float(ab @ ab)
    t = np.clip((p - a) @ ab / den, 0.0, 1.0) if den > 0 else np.zeros(len(p))
    return np.hypot(*(p - (a + t[:, None] * ab)).T)


def simplify(points, epsilon):
    """closed-loop Douglas-Peucker in float64: the loop is cut at its first vertex and at the vertex farthest from
    it (the lowest index on ties) and each half simplified with tolerance ``epsilon``: a vertex is dropped when it
    lies within ``epsilon`` of the kept chord.  ``epsilon <= 0`` returns the input; a loop never drops below three
    points (the vertex farthest from the two anchors' chord is kept then)."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    n = len(pts)
    if epsilon <= 0 or n <= 3:
        return points
    far = int(np.argmax(np.hypot(*(pts - pts[0]).T)))
    ring = np.concatenate([pts, pts[:1]])  # index n is the first vertex again
    keep = np.zeros(n + 1, bool)
    keep[[0, far, n]] = True
    stack = [(0, far), (far, n)]
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        d = _seg_dist(ring[i + 1:j], ring[i], ring[j])
        k = int(np.argmax(d))
        if d[k] > epsilon:
            keep[i + 1 + k] = True
            stack += [(i, i + 1 + k), (i + 1 + k, j)]
    keep = keep[:n]
    if keep.sum() < 3:
        d = _seg_dist(pts, pts[0], pts[far])
        d[keep] = -1.0
        keep[int(np.argmax(d))] = True
    kept = pts[keep]
    if isinstance(points, np.ndarray):
        return kept.astype(points.dtype)
    return [[type(points[0][0])(x), type(points[0][1])(y)] for x, y in kept.tolist()]


def _crossed(polys):
    """indices of the components that a later component's hole may paint over.  Where several classes are
    8-connected, two components of different classes can cross at a saddle, so part of a component can lie inside a
    hole of a component with a larger root.  Such a part hangs on the rest through a corner where the hole's loop
    turns and which is a vertex of the crossing component too (an edge step out of a hole would cross a crack of
    the hole's owner), so sharing a vertex with a later component's hole is necessary for it; the test is
    conservative, which costs a shape and never a pixel."""
    owner = {}
    for k, p in enumerate(polys):
        for h in p["holes"]:
            for x, y in h:
                owner[(p["image"], x, y)] = k  # ascending k: the last owner is the largest
    return [k for k, p in enumerate(polys)
            if any(owner.get((p["image"], x, y), -1) > k for ring in [p["outer"]] + p["holes"] for x, y in ring)]


def _keyhole(outer, holes):
    """one closed path that covers, by the even-odd rule, the outer ring less the holes: the outer ring, then
    per hole a bridge of one horizontal and one vertical lattice segment from the first vertex to the hole, the
    hole's ring and the bridge back.  Each bridge is walked twice, so it encloses nothing."""
    o0 = list(outer[0])
    path = [list(q) for q in outer] + [o0]
    for h in holes:
        b0 = list(h[0])
        elbow = [b0[0], o0[1]]
        path += [elbow] + [list(q) for q in h] + [b0, elbow, o0]
    return path


def labelme(polys, height, width, image_path, class_names=None, epsilon=1.0):
    """the labelme document of one image's ``polygons``: per component, in table order, one ``polygon`` shape
    labelled ``class_names[c]`` (``class_<c>`` without names) and then one labelled ``_background_`` per hole, all
    with ``group_id`` = the component's index.  Painted in this order, later shapes over earlier ones, the shapes
    reproduce the map at ``epsilon = 0``: whatever lies wholly inside a hole has a larger root and comes later.  The
    one exception are components of different 8-connected classes that cross at a saddle: part of the earlier one
    can lie inside a hole of the later one.  Every component that shares a vertex with a later component's hole
    (``_crossed``) is therefore painted once more at the end of the document, as one polygon that covers its own
    pixels and nothing else (``_keyhole``), so no order among these matters; a binary map and a 4-connected one
    never need it.  Points are lattice corners, each ring simplified with ``simplify(., epsilon)``."""
    if epsilon < 0:
        raise ValueError(f"epsilon must not be negative, got {epsilon}")
    shapes = []

    def name(c):
        if class_names is not None and not 0 <= c < len(class_names):
            raise ValueError(f"class {c} has no name among the {len(class_names)} given")
        return class_names[c] if class_names is not None else f"class_{c}"

    def shape(label, pts, group):
        shapes.append({"label": label, "points": [[float(x), float(y)] for x, y in pts], "group_id": group,
                       "shape_type": "polygon", "flags": {}})

    for k, p in enumerate(polys):
        shape(name(p["class"]), simplify(p["outer"], epsilon), k)
        for h in p["holes"]:
            shape(BACKGROUND, simplify(h, epsilon), k)
    for k in _crossed(polys):
        p = polys[k]
        shape(name(p["class"]), _keyhole(simplify(p["outer"], epsilon), [simplify(h, epsilon) for h in p["holes"]]), k)
    return {"version": LABELME_VERSION, "flags": {}, "shapes": shapes, "imagePath": str(image_path),
            "imageData": None, "imageHeight": int(height), "imageWidth": int(width)}
