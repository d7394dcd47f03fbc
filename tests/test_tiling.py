"""CPU: the tile grid of the tiled inference path (utils/tiling.py) and the host side of its C ABI.

utils/tiling.py is the statement of the grid and the window that csrc/tiles.hip restates on the
device; here its counts, origins, coverage and window sums are checked against the numbers worked
out by hand in the feature's description, unetseg_tile_count is held to it, and every argument the
launching entry points must refuse is refused with status 1 (the argument-check status; a launch
failure would be 2) and a message, before any HIP call -- this container has no GPU.
"""
import ctypes
import os
import re
import struct

import pytest

from conftest import REPO

# (extent, tile, overlap) -> tiles along that axis
CASES = [((37, 16, 4), 3), ((53, 16, 4), 5), ((10, 16, 4), 1), ((32, 16, 0), 2), ((33, 16, 8), 4), ((16, 16, 8), 1)]
NEW = ("unetseg_tile_count", "unetseg_tile_gather", "unetseg_tile_accum", "unetseg_tile_finish")


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _raw():
    from unetseg_hip import lib

    assert os.path.exists(lib.LIB_PATH), "libunetseg_hip.so not built (run __graft_entry__.build())"
    return lib.load()


@pytest.mark.parametrize("case,n", CASES)
def test_grid_counts_and_origins(case, n):
    from utils import tiling

    L, t, o = case
    assert tiling.count(L, t, o) == n
    assert tiling.origins(L, t, o) == [i * (t - o) for i in range(n)]
    # the last tile reaches the far edge, and no tile starts past it
    assert tiling.origins(L, t, o)[-1] + t >= L
    assert tiling.origins(L, t, o)[-1] < L


def test_grid_is_row_major():
    from utils import tiling

    assert tiling.grid(37, 53, 16, 4) == (5, 3)
    assert tiling.tile_origin(0, 37, 53, 16, 4) == (0, 0)
    assert tiling.tile_origin(4, 37, 53, 16, 4) == (0, 48)
    assert tiling.tile_origin(5, 37, 53, 16, 4) == (12, 0)
    assert tiling.tile_origin(14, 37, 53, 16, 4) == (24, 48)
    with pytest.raises(IndexError):
        tiling.tile_origin(15, 37, 53, 16, 4)
    assert tiling.ranges(15, 8) == [(0, 8), (8, 7)]
    assert tiling.ranges(3, 8) == [(0, 3)]


@pytest.mark.parametrize("case,n", CASES)
def test_every_pixel_in_one_or_two_tiles(case, n):
    from utils import tiling

    L, t, o = case
    org = tiling.origins(L, t, o)
    for x in range(L):
        brute = [i for i, a in enumerate(org) if a <= x < a + t]
        assert 1 <= len(brute) <= 2
        assert tiling.covering(x, L, t, o) == brute


@pytest.mark.parametrize("t,o", [(16, 4), (16, 8), (16, 0), (64, 32), (512, 64)])
def test_window(t, o):
    from utils import tiling

    w = tiling.window(t, o)
    assert len(w) == t and all(_f32(v) == v for v in w)  # float32 values
    assert w == w[::-1]
    assert w[0] == _f32(1.0 / (o + 1))
    assert max(w) == (1.0 if 2 * o < t else _f32(o / (o + 1.0)))  # o = t / 2: the two ramps meet below 1
    assert all(v == 1.0 for v in w[o:t - o])
    # interior overlap: pixel k of the overlap is u = s + k in the left tile and u = k in the right one
    s = t - o
    for k in range(o):
        assert _f32(w[s + k] + w[k]) == 1.0


def test_bad_grid_parameters():
    from utils import tiling

    for t, o in ((0, 0), (-16, 0), (16, -1), (16, 9), (15, 8)):
        with pytest.raises(ValueError):
            tiling.check(t, o)
    tiling.check(15, 7)
    with pytest.raises(ValueError):
        tiling.count(0, 16, 4)


def test_tile_count_agrees_with_python():
    from unetseg_hip import lib
    from utils import tiling

    raw = _raw()
    for (L, t, o), n in CASES:
        for other in (L, 1, 100):
            nx, ny = ctypes.c_int(-1), ctypes.c_int(-1)
            assert raw.unetseg_tile_count(other, L, t, o, ctypes.byref(nx), ctypes.byref(ny)) == 0
            assert (nx.value, ny.value) == (n, tiling.count(other, t, o)) == tiling.grid(other, L, t, o)
            assert lib.tile_count(L, other, t, o) == (ny.value, nx.value)
    assert lib.tile_count(2048, 2048, 512, 64) == (5, 5) == tiling.grid(2048, 2048, 512, 64)


def test_new_names_in_header_table_and_library():
    from unetseg_hip import lib
    from unetseg_hip.gen_fastcall import supported

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "unetseg_hip.h")).read(), flags=re.S)
    raw = _raw()
    bound = {n for n, _, _ in supported()}
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in lib.SIGNATURES and name in lib.exported_symbols()
        assert hasattr(raw, name)
        assert name in bound
    fast = lib._fast()
    if fast is not None:
        assert all(hasattr(fast, n[len("unetseg_"):]) for n in NEW)


# a non-null pointer that is never dereferenced: every case below fails an argument check
PTR = 4096
BIG = 2 ** 31 - 1


def _gather(img=PTR, H=37, W=53, tile=16, overlap=4, t0=0, nt=15, fill=128, out=PTR):
    return ("tile_gather", (img, H, W, tile, overlap, t0, nt, fill, out, None))


def _accum(lg=PTR, C=2, H=37, W=53, tile=16, overlap=4, t0=0, nt=15, acc=PTR):
    return ("tile_accum", (lg, C, H, W, tile, overlap, t0, nt, acc, None))


def _finish(acc=PTR, C=2, H=37, W=53, tile=16, overlap=4, probs=None, labels=PTR):
    return ("tile_finish", (acc, C, H, W, tile, overlap, probs, labels, None))


REFUSED = [
    # null required pointers (probs alone may be null)
    (_gather(img=None), "null"), (_gather(out=None), "null"),
    (_accum(lg=None), "null"), (_accum(acc=None), "null"),
    (_finish(acc=None), "null"), (_finish(labels=None), "null"),
    # tile <= 0
    (_gather(tile=0, overlap=0), "tile must be positive"), (_accum(tile=-16, overlap=0), "tile must be positive"),
    (_finish(tile=0, overlap=0), "tile must be positive"),
    # overlap < 0 or > tile / 2
    (_gather(overlap=-1), "overlap"), (_gather(overlap=9), "overlap"), (_accum(overlap=9), "overlap"),
    (_accum(tile=15, overlap=8), "overlap"), (_finish(overlap=-1), "overlap"), (_finish(overlap=9), "overlap"),
    # C outside [2, 32]
    (_accum(C=1), "C=1"), (_accum(C=33), "C=33"), (_finish(C=1), "C=1"), (_finish(C=33), "C=33"),
    (_finish(C=0), "C=0"),
    # t0 < 0, nt <= 0, t0 + nt > nx * ny (the 37 x 53 grid has 15 tiles)
    (_gather(t0=-1), "tile range"), (_gather(nt=0), "tile range"), (_gather(t0=1, nt=15), "tile range"),
    (_gather(t0=15, nt=1), "tile range"), (_accum(t0=-1), "tile range"), (_accum(nt=-3), "tile range"),
    (_accum(t0=8, nt=8), "tile range"), (_accum(t0=BIG, nt=BIG), "tile range"),
    # sizes the index types cannot hold: H * W * C * 4 past 64 bits, more tiles than the 32-bit tile index
    (_accum(C=32, H=BIG, W=BIG, tile=BIG, overlap=0, nt=1), "64-bit"),
    (_finish(C=32, H=BIG, W=BIG, tile=BIG, overlap=0), "64-bit"),
    (_gather(H=BIG, W=BIG, tile=1, overlap=0, nt=1), "32-bit tile index"),
    (_accum(H=BIG, W=BIG, tile=1, overlap=0, nt=1), "32-bit tile index"),
    (_finish(H=BIG, W=BIG, tile=1, overlap=0), "32-bit tile index"),
    (_finish(H=1 << 20, W=1 << 20, tile=1 << 20, overlap=0), "launch grid"),
    # others
    (_gather(H=0), "image size"), (_accum(W=-5), "image size"), (_finish(H=0), "image size"),
    (_gather(fill=256), "fill"), (_gather(fill=-1), "fill"),
]


@pytest.mark.parametrize("call,msg", REFUSED, ids=[f"{c[0]}-{i}" for i, (c, _) in enumerate(REFUSED)])
def test_argument_errors_refused_before_any_launch(call, msg):
    from unetseg_hip import lib

    raw = _raw()
    name, args = call
    assert getattr(raw, "unetseg_" + name)(*args) == 1
    err = raw.unetseg_last_error().decode()
    assert name in err and msg in err, err
    with pytest.raises(RuntimeError, match=f"unetseg_{name} failed"):
        getattr(lib.lib, name)(*args)


def test_tile_count_argument_errors():
    from unetseg_hip import lib

    raw = _raw()
    nx, ny = ctypes.c_int(7), ctypes.c_int(7)
    assert raw.unetseg_tile_count(37, 53, 16, 4, None, ctypes.byref(ny)) == 1
    assert b"tile_count" in raw.unetseg_last_error()
    for H, W, t, o in ((37, 53, 0, 0), (37, 53, 16, 9), (37, 53, 16, -1), (0, 53, 16, 4), (BIG, BIG, 1, 0)):
        assert raw.unetseg_tile_count(H, W, t, o, ctypes.byref(nx), ctypes.byref(ny)) == 1
        assert b"tile_count" in raw.unetseg_last_error()
        assert (nx.value, ny.value) == (7, 7)  # outputs untouched
    with pytest.raises(RuntimeError, match="overlap"):
        lib.tile_count(37, 53, 16, 9)
