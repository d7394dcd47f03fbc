"""Sequential restatement of the contour contract (csrc/contours.hip, unetseg_hip/contours.py).

A class map is an integer array [H][W] or [N][H][W]; class 0 is background; components and roots are those of
``ccl_ref.label(cls, connectivity)``.  Pixel (y, x) covers the square [x, x+1] x [y, y+1]; a lattice corner is
(x, y) with 0 <= x <= W and 0 <= y <= H.

A *crack* is a side of a pixel of a non-zero class whose 4-neighbour across that side has another class or lies
outside the image.  Side 0 is the top (x, y) -> (x+1, y), 1 the right (x+1, y) -> (x+1, y+1), 2 the bottom
(x+1, y+1) -> (x, y+1), 3 the left (x, y+1) -> (x, y): clockwise on screen, the owner on the right of travel.
Crack id = (y * W + x) * 4 + side.  ``successor`` states the turning rule; ``trace`` walks the loops with a
visited set, literally.  ``rasterise`` is the even-odd fill of pixel centres that the labelme checks use.
"""
import numpy as np

import ccl_ref

# direction of travel (dx, dy) of a crack of each side; the owner lies towards DIR[(side + 1) % 4]
DIR = ((1, 0), (0, 1), (-1, 0), (0, -1))
# tail corner of a side, as an offset from the pixel's (x, y)
TAIL = ((0, 0), (1, 0), (1, 1), (0, 1))


def is_crack(cls, y, x, s):
    H, W = cls.shape
    if cls[y, x] == 0:
        return False
    ox, oy = DIR[(s + 3) % 4]  # away from the owner
    ny, nx = y + oy, x + ox
    return not (0 <= ny < H and 0 <= nx < W) or cls[ny, nx] != cls[y, x]


def successor(cls, y, x, s, connectivity):
    """(y, x, side) of the crack that follows crack (y, x, s)"""
    H, W = cls.shape
    c = cls[y, x]

    def inside(py, px):
        return 0 <= py < H and 0 <= px < W and cls[py, px] == c

    dx, dy = DIR[s]
    lx, ly = DIR[(s + 3) % 4]
    F = (y + dy, x + dx)  # ahead on the owner's side
    D = (y + dy + ly, x + dx + lx)  # ahead on the other side
    f_in, d_in = inside(*F), inside(*D)
    if connectivity == 8:
        turn = "left" if d_in else "straight" if f_in else "right"
    else:
        turn = "right" if not f_in else "straight" if not d_in else "left"
    if turn == "left":
        return D[0], D[1], (s + 3) % 4
    if turn == "straight":
        return F[0], F[1], s
    return y, x, (s + 1) % 4


def _trace2d(cls, connectivity, image, first):
    H, W = cls.shape
    root = ccl_ref.label(cls, connectivity)
    seen = set()
    found = []  # (root, leader, class, vertices, area2, cracks)
    for cid in range(H * W * 4):
        y, x, s = cid // 4 // W, cid // 4 % W, cid % 4
        if cid in seen or not is_crack(cls, y, x, s):
            continue
        # cid is the smallest id of its loop: every smaller crack has been walked already
        chain = []
        cur = (y, x, s)
        while True:
            k = (cur[0] * W + cur[1]) * 4 + cur[2]
            if k in seen:
                break
            assert is_crack(cls, *cur) and root[cur[0], cur[1]] == root[y, x]
            seen.add(k)
            chain.append(cur)
            cur = successor(cls, cur[0], cur[1], cur[2], connectivity)
        assert cur == (y, x, s), "the successor map is not a bijection"
        verts = []
        for i, (py, px, ps) in enumerate(chain):
            if chain[i - 1][2] != ps:  # the predecessor of the leader is the last crack of the loop
                verts.append((px + TAIL[ps][0], py + TAIL[ps][1]))
        area2 = sum(verts[i][0] * verts[(i + 1) % len(verts)][1] - verts[(i + 1) % len(verts)][0] * verts[i][1]
                    for i in range(len(verts)))
        assert area2 % 2 == 0
        found.append((int(root[y, x]), cid, int(cls[y, x]), verts, area2 // 2, len(chain)))
    found.sort(key=lambda r: (r[0], r[1]))
    loops, vertices = [], []
    for r, leader, c, verts, area, cracks in found:
        hole = int(leader != 4 * r)
        assert (area > 0) == (hole == 0)
        loops.append((image, c, r, hole, first + len(vertices), len(verts), area, cracks))
        vertices += verts
    return loops, vertices


def trace(cls, connectivity=8):
    """(loops int32 [L][8], vertices int32 [V][2]) of a map [H][W] or a batch [N][H][W]"""
    assert connectivity in (4, 8)
    cls = np.asarray(cls)
    maps = cls[None] if cls.ndim == 2 else cls
    loops, vertices = [], []
    for n, im in enumerate(maps):
        lo, ve = _trace2d(im, connectivity, n, len(vertices))
        loops += lo
        vertices += ve
    return np.array(loops, np.int32).reshape(-1, 8), np.array(vertices, np.int32).reshape(-1, 2)


def rasterise(shapes, H, W):
    """int32 [H][W]: the shapes painted in order, later over earlier; a shape is (value, points) and covers the
    pixels whose centre (x + 0.5, y + 0.5) lies inside the closed polygon by the even-odd rule"""
    out = np.zeros((H, W), np.int32)
    xs = np.arange(W) + 0.5
    for value, pts in shapes:
        pts = np.asarray(pts, np.float64).reshape(-1, 2)
        for y in range(H):
            yc = y + 0.5
            inside = np.zeros(W, bool)
            for (x0, y0), (x1, y1) in zip(pts, np.roll(pts, -1, 0)):
                if (y0 <= yc) != (y1 <= yc):  # the edge crosses this row of centres
                    inside ^= xs < x0 + (yc - y0) * (x1 - x0) / (y1 - y0)
            out[y, inside] = value
    return out


def labelme_shapes(doc, class_names=None):
    """the (value, points) list of a labelme document: ``_background_`` is 0, ``class_<c>`` or class_names[c] is c"""
    shapes = []
    for sh in doc["shapes"]:
        assert sh["shape_type"] == "polygon"
        lab = sh["label"]
        if lab == "_background_":
            v = 0
        elif class_names is not None and lab in class_names:
            v = list(class_names).index(lab)
        else:
            v = int(lab[len("class_"):])
        shapes.append((v, sh["points"]))
    return shapes


# ---- the maps of the tests -------------------------------------------------------------------------------------
CPU_SIZES = ((1, 1), (1, 70), (70, 1), (2, 2), (33, 33), (37, 130))
GPU_SIZES = ((31, 31), (63, 63), (64, 64), (65, 65), (129, 129), (130, 37))
DENSITIES = (0.30, 0.41, 0.50, 0.59, 0.70)


def noise(H, W, density, C=2, seed=0):
    """percolation noise: a pixel is non-zero with probability ``density``, its class uniform in 1 .. C-1"""
    rng = np.random.default_rng([seed, H, W, int(density * 100), C])
    on = rng.random((H, W)) < density
    return np.where(on, rng.integers(1, C, (H, W)), 0).astype(np.int32)


def size_cases(H, W):
    """the noise maps of one size: every density, C in {2, 5}"""
    return [noise(H, W, d, C, seed=i) for i, d in enumerate(DENSITIES) for C in (2, 5)]


def tile_sizes(T, axis, other=37):
    """T-1, T, T+1, 2T+1 on one axis, a small odd size on the other"""
    return [(t, other) if axis == "H" else (other, t) for t in (T - 1, T, T + 1, 2 * T + 1)]


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2 == 0).astype(np.int32)


def spiral(S):
    """a one-pixel path spiralling inwards through an S x S square, walls of one pixel between its arms"""
    m = np.zeros((S, S), np.int32)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):  # go on, or turn right once
            ny, nx = y + dy, x + dx
            ay, ax = ny + dy, nx + dx  # the pixel after the next must stay free: it keeps the wall
            ok = 0 <= ny < S and 0 <= nx < S and m[ny, nx] == 0 and not (0 <= ay < S and 0 <= ax < S and m[ay, ax])
            if ok:
                # the next pixel must not touch an earlier arm sideways
                sy, sx = dx, -dy
                side = [(ny + sy, nx + sx), (ny - sy, nx - sx)]
                ok = all(not (0 <= py < S and 0 <= px < S and m[py, px]) for py, px in side)
            if ok:
                y, x = ny, nx
                m[y, x] = 1
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def rings(S=29):
    """ring inside ring inside ring, of classes 1, 2, 1, with a dot in the middle: islands in holes"""
    m = np.zeros((S, S), np.int32)
    for k, c in ((1, 1), (4, 2), (7, 1), (10, 3)):
        m[k:S - k, k:S - k] = c
        m[k + 1:S - k - 1, k + 1:S - k - 1] = 0
    m[S // 2, S // 2] = 1
    return m


def comb(H=9, W=41):
    """a bar with one-pixel teeth one pixel apart"""
    m = np.zeros((H, W), np.int32)
    m[1, 1:W - 1] = 1
    m[1:H - 1, 1:W - 1:2] = 1
    return m
