"""numpy / Python restatement of the connected-component semantics (csrc/ccl.hip, unetseg_hip/ccl.py).

A class map is an integer array [H][W] or [N][H][W]; class 0 is background.  Two pixels of one image
are joined iff they have equal class and are edge neighbours, or diagonal neighbours where that class
is 8-connected: the non-zero classes have ``connectivity``, class 0 the dual (4 for 8, 8 for 4).

``label``: root[i] = the smallest raster index y * W + x of pixel i's component.  The adjacency rule is
stated once, in ``_pairs``; a plain union-find (the smaller root wins) joins the pairs.  ``stats`` and
``clean`` restate the contract literally.  No scipy.
"""
import numpy as np


def _diag8(cls, connectivity):
    """per pixel: diagonal neighbours join for this pixel's class"""
    return np.where(cls != 0, connectivity, 12 - connectivity) == 8


def _pairs(cls, connectivity):
    """every joined pair (i, j) of raster indices of one image, j the neighbour right of / below i"""
    H, W = cls.shape
    idx = np.arange(H * W).reshape(H, W)
    d8 = _diag8(cls, connectivity)
    out = []
    # (dy, dx): right, down, down-right, down-left
    for dy, dx, diagonal in ((0, 1, False), (1, 0, False), (1, 1, True), (1, -1, True)):
        a = (slice(0, H - dy), slice(max(0, -dx), W - max(0, dx)))
        b = (slice(dy, H), slice(max(0, dx), W - max(0, -dx)))
        same = cls[a] == cls[b]
        if diagonal:
            same &= d8[a]
        out.append(np.stack([idx[a][same], idx[b][same]], 1))
    return np.concatenate(out)


def _label2d(cls, connectivity):
    H, W = cls.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in _pairs(cls, connectivity).tolist():
        a, b = find(i), find(j)
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    return np.array([find(i) for i in range(H * W)], np.int32).reshape(H, W)


def _each(fn, x, *args):
    x = np.asarray(x)
    if x.ndim == 2:
        return fn(x, *args)
    return np.stack([fn(im, *args) for im in x])


def label(cls, connectivity=8):
    """int32, the shape of cls: the smallest raster index of every pixel's component"""
    assert connectivity in (4, 8)
    return _each(_label2d, cls, connectivity)


def _stats2d(root):
    H, W = root.shape
    area, ymax, xmin, xmax = [0] * (H * W), [0] * (H * W), [W] * (H * W), [0] * (H * W)
    for y, row in enumerate(root.tolist()):
        for x, r in enumerate(row):
            area[r] += 1
            ymax[r] = max(ymax[r], y)
            xmin[r] = min(xmin[r], x)
            xmax[r] = max(xmax[r], x)
    return np.array([area, ymax, xmin, xmax], np.int32).reshape(4, H, W)


def stats(root):
    """int32 [4, *root.shape]: area, ymax, xmin, xmax at the root positions (area 0 elsewhere, where the
    other planes mean nothing)"""
    root = np.asarray(root)
    if root.ndim == 2:
        return _stats2d(root)
    return np.stack([_stats2d(r) for r in root], 1)


def is_root(root):
    """bool, the shape of root: the pixel is its component's root"""
    root = np.asarray(root)
    H, W = root.shape[-2:]
    return root == np.arange(H * W, dtype=root.dtype).reshape(H, W)


def components(cls, connectivity=8):
    """int32 [K][7]: (image, class, area, ymin, xmin, ymax, xmax) of every component of a non-zero
    class, ordered by (image, root index)"""
    cls = np.asarray(cls)
    maps = cls[None] if cls.ndim == 2 else cls
    rows = []
    for n, im in enumerate(maps):
        root = _label2d(im, connectivity)
        st = _stats2d(root)
        W = im.shape[1]
        for r in np.flatnonzero(is_root(root).reshape(-1)):
            y, x = divmod(int(r), W)
            if im[y, x] != 0:
                rows.append((n, im[y, x], st[0, y, x], y, st[2, y, x], st[1, y, x], st[3, y, x]))
    return np.array(rows, np.int32).reshape(-1, 7)


def _clean2d(cls, min_area, max_hole, connectivity):
    H, W = cls.shape
    out = cls.copy()
    # step 1: small components of the non-zero classes become background
    root = _label2d(out, connectivity)
    area = _stats2d(root)[0].reshape(-1)
    out[(out != 0) & (area[root] < min_area)] = 0
    # step 2, on step 1's result: small background components off every border take the class above their root
    root = _label2d(out, connectivity)
    st = _stats2d(root).reshape(4, -1)
    step1 = out.copy()
    for r in np.flatnonzero(is_root(root).reshape(-1)):
        y, x = divmod(int(r), W)
        if step1[y, x] != 0 or st[0, r] >= max_hole:
            continue
        if y == 0 or st[1, r] == H - 1 or st[2, r] == 0 or st[3, r] == W - 1:
            continue
        out[root == r] = step1[y - 1, x]
    return out


def clean(cls, min_area=0, max_hole=0, connectivity=8):
    """the map after the two steps of the contract; the input is left alone"""
    assert connectivity in (4, 8) and min_area >= 0 and max_hole >= 0
    return _each(_clean2d, cls, min_area, max_hole, connectivity)
