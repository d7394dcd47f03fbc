"""Connected components of class maps on the HIP path (csrc/ccl.hip).

A class map is an int32 tensor [H,W] or [N,H,W] on the GPU; values are compared for equality only and
class 0 is background.  Two pixels of one image are joined iff they have equal class and are edge
neighbours, or diagonal neighbours where that class is 8-connected: the non-zero classes have
``connectivity`` (4 or 8), class 0 the dual (4 for 8, 8 for 4), so a hole is what it should be.

``label`` names every pixel by its root, the smallest raster index ``y * W + x`` of its component
(canonical: no launch order or tile size shows in it).  ``stats`` holds area and box at the root
positions, ``components`` compacts them into a table, ``clean`` drops small components and fills small
holes.  ``label``, ``stats`` and ``clean`` run on the current stream and never wait on the host.
"""
from __future__ import annotations

import ctypes

import torch

from .classmap import _map, _stream
from .lib import lib


def tile():
    """(tw, th): the label pass works on tiles of this size, so its seams lie at their multiples"""
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    lib.ccl_tile(ctypes.addressof(tw), ctypes.addressof(th))
    return tw.value, th.value


def label(cls, connectivity=8):
    """int32, the shape of ``cls``: the root of every pixel's component"""
    c = _map(cls)
    N, H, W = c.shape
    root = torch.empty_like(c)
    lib.ccl_label(c.data_ptr(), N, H, W, connectivity, root.data_ptr(), _stream(c))
    return root.view(cls.shape)


def stats(root):
    """int32 [4, *root.shape]: planes area, ymax, xmin, xmax of ``root`` (what ``label`` returned),
    meaningful at root positions; elsewhere area is 0 and the rest unspecified.  ymin is the root's row."""
    r = _map(root, "root")
    N, H, W = r.shape
    st = torch.empty(4, N, H, W, dtype=torch.int32, device=r.device)
    lib.ccl_stats(r.data_ptr(), N, H, W, st.data_ptr(), _stream(r))
    return st.view(4, *root.shape)


def components(cls, connectivity=8, skeleton=None):
    """int32 [K,7] on the device: (image, class, area, ymin, xmin, ymax, xmax) of every component of a
    non-zero class, ordered by (image, root index).  The compaction is torch (it sizes its result on
    the host).  ``skeleton``: a map of the shape of ``cls`` that is ``cls`` or 0 at every pixel
    (``skeleton.thin(cls)``); the table is then [K,8], the last column the component's non-zero pixels of it,
    counted on the device with integer adds."""
    c = _map(cls)
    N, H, W = c.shape
    root = label(c, connectivity)
    st = stats(root).view(4, -1)
    flat = c.view(-1)
    at = torch.nonzero((st[0] > 0) & (flat != 0)).view(-1)  # ascending: (image, root index)
    image, idx = at // (H * W), at % (H * W)
    area, ymax, xmin, xmax = (st[k][at].long() for k in range(4))
    cols = [image, flat[at].long(), area, idx // W, xmin, ymax, xmax]
    if skeleton is not None:
        sk = _map(skeleton, "skeleton")
        if sk.shape != c.shape or sk.device != c.device:
            raise ValueError(f"skeleton {tuple(sk.shape)} on {sk.device} and cls {tuple(c.shape)} on {c.device} differ")
        on = torch.nonzero(sk.view(-1) != 0).view(-1)
        # a pixel's root is an index inside its image: the image's offset makes it one into the flat batch
        where = on // (H * W) * (H * W) + root.view(-1)[on].long()
        px = torch.zeros(N * H * W, dtype=torch.int64, device=c.device).index_add_(0, where, torch.ones_like(where))
        cols.append(px[at])
    return torch.stack(cols, 1).to(torch.int32)


def _filtered(c, connectivity, step, threshold):
    N, H, W = c.shape
    root = label(c, connectivity)
    st = stats(root)
    out = torch.empty_like(c)
    threshold = min(threshold, 2**31 - 1)  # no area is larger
    lib.ccl_filter(c.data_ptr(), root.data_ptr(), st.data_ptr(), N, H, W, step, threshold, out.data_ptr(), _stream(c))
    return out


def clean(cls, min_area=0, max_hole=0, connectivity=8):
    """``cls`` without its small components and small holes, as a new map, in two steps:

    1. every component of a non-zero class with area < ``min_area`` becomes class 0;
    2. on that result, every class-0 component with area < ``max_hole`` that touches no image border
       takes the class of the pixel directly above its root (for a binary map: it is filled with 1).

    A threshold of 0 or 1 removes nothing, and its step is not run; with both so, ``cls`` itself comes
    back and nothing is launched."""
    if min_area < 0 or max_hole < 0:
        raise ValueError(f"min_area and max_hole must not be negative, got {min_area} and {max_hole}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    c = _map(cls)
    if min_area <= 1 and max_hole <= 1:
        return cls
    if min_area > 1:
        c = _filtered(c, connectivity, 1, min_area)
    if max_hole > 1:
        c = _filtered(c, connectivity, 2, max_hole)
    return c.view(cls.shape)
