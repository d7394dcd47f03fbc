"""Tile grid and blend window of the tiled full-resolution inference (predict.predict_labels_tiled).

Pure Python (no numpy, no torch): the host code and the tests share it, and csrc/tiles.hip restates
it on the device.  One axis of extent L is cut into tiles of ``tile`` pixels that overlap their
neighbour by ``overlap`` pixels (0 <= overlap <= tile // 2), stride ``s = tile - overlap``:

    n = max(1, ceil((L - overlap) / s))        tiles, origins i * s

Tiles may hang over the far edge and are never shifted back, so a pixel lies in at most 2 tiles per
axis (4 in the plane).  Tiles are numbered row-major: index = iy * nx + ix.

The 1-D blend window over u in [0, tile) is, in float32,

    w(u) = min(1, (u + 1) / (overlap + 1), (tile - u) / (overlap + 1))

a ramp over the overlap at either end; in an interior overlap the two ramps sum to 1.  A pixel's
weight in a tile is w(ux) * w(uy), and the blended probability is
sum_i w_i softmax(logits_i) / sum_i w_i over its covering tiles in ascending tile index (the
division only matters at the image border, where a single ramped tile covers the pixel).
"""
import struct


def _f32(x):
    """x rounded to float32 (a float64 quotient of two small integers rounds to the float32 quotient)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def check(tile, overlap):
    if tile <= 0:
        raise ValueError(f"tile must be positive, got {tile}")
    if overlap < 0 or overlap > tile // 2:
        raise ValueError(f"overlap must lie in [0, tile // 2 = {tile // 2}], got {overlap}")


def count(extent, tile, overlap):
    """tiles along one axis of ``extent`` pixels"""
    check(tile, overlap)
    if extent <= 0:
        raise ValueError(f"extent must be positive, got {extent}")
    s = tile - overlap
    return max(1, -((overlap - extent) // s))


def origins(extent, tile, overlap):
    """first pixel of every tile along one axis"""
    s = tile - overlap
    return [i * s for i in range(count(extent, tile, overlap))]


def grid(height, width, tile, overlap):
    """(nx, ny): tiles per row and per column"""
    return count(width, tile, overlap), count(height, tile, overlap)


def tile_origin(index, height, width, tile, overlap):
    """(y0, x0) of tile ``index`` (row-major)"""
    nx, ny = grid(height, width, tile, overlap)
    if not 0 <= index < nx * ny:
        raise IndexError(index)
    s = tile - overlap
    return (index // nx) * s, (index % nx) * s


def covering(x, extent, tile, overlap):
    """indices, ascending, of the tiles along one axis that contain pixel x (1 or 2 of them)"""
    n = count(extent, tile, overlap)
    s = tile - overlap
    hi = min(x // s, n - 1)
    return [i for i in (hi - 1, hi) if i >= 0 and i * s <= x < i * s + tile]


def window(tile, overlap):
    """the 1-D window as ``tile`` float32 values (held in Python floats)"""
    check(tile, overlap)
    d = float(overlap + 1)
    return [min(1.0, _f32((u + 1) / d), _f32((tile - u) / d)) for u in range(tile)]


def ranges(n_tiles, batch):
    """(t0, nt) of successive tile ranges of at most ``batch`` tiles"""
    if batch <= 0:
        raise ValueError(f"tile batch must be positive, got {batch}")
    return [(t0, min(batch, n_tiles - t0)) for t0 in range(0, n_tiles, batch)]
