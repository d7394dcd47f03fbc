"""CPU: the host side of the test-time augmentation (csrc/tta.hip, unetseg_hip/tta.py).

* both entry points refuse every bad argument set before any launch, with status 1 and a message;
* the named modes are the four masks of the view numbering;
* tests/tta_ref.py (the reference the GPU tests hold the kernels to) inverts each of its own views, and
  its view 2 is one counter-clockwise quarter turn: this pins the turn direction.
"""
import os

import pytest
import torch

import tta_ref

PTR = 4096  # a non-null pointer value; every call below is refused before it is used
BIG = 2 ** 31 - 1


def _raw():
    from unetseg_hip import lib

    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    return lib.load()


# (x, B, C, H, W, views, out), the text the message must contain
BAD_BOTH = [
    ((None, 1, 3, 8, 8, 1, PTR), "null"),
    ((PTR, 1, 3, 8, 8, 1, None), "null"),
    ((PTR, 0, 3, 8, 8, 1, PTR), "bad shape"),
    ((PTR, 1, 0, 8, 8, 1, PTR), "bad shape"),
    ((PTR, 1, 3, -1, 8, 1, PTR), "bad shape"),
    ((PTR, 1, 3, 8, 0, 1, PTR), "bad shape"),
    ((PTR, 1, 3, 8, 8, 0, PTR), "views mask"),
    ((PTR, 1, 3, 8, 8, 256, PTR), "views mask"),
    ((PTR, 1, 3, 8, 8, -1, PTR), "views mask"),
    ((PTR, 1, 3, 8, 9, 0x04, PTR), "H == W"),
    ((PTR, 1, 3, 8, 9, 0x08, PTR), "H == W"),
    ((PTR, 1, 3, 9, 8, 0x40, PTR), "H == W"),
    ((PTR, 1, 3, 9, 8, 0xFF, PTR), "H == W"),
    ((PTR, BIG, 3, BIG, BIG, 0x33, PTR), "64-bit"),
]


@pytest.mark.parametrize("name", ["tta_views", "tta_merge"])
@pytest.mark.parametrize("args,msg", BAD_BOTH)
def test_argument_errors_reported_without_device(name, args, msg):
    from unetseg_hip import lib

    raw = _raw()
    fn = getattr(raw, "unetseg_" + name)
    assert fn(*args, None) == 1
    err = raw.unetseg_last_error().decode()
    assert name in err and msg in err, err
    with pytest.raises(RuntimeError, match=msg):
        getattr(lib.lib, name)(*args, None)


def test_merge_refuses_more_classes_than_it_holds():
    raw = _raw()
    assert raw.unetseg_tta_merge(PTR, 1, 33, 8, 8, 0xFF, PTR, None) == 1
    assert "C=33" in raw.unetseg_last_error().decode()
    # the views kernel has no class limit: the same shape fails there only for its offsets
    assert raw.unetseg_tta_views(PTR, BIG, 33, BIG, BIG, 0xFF, PTR, None) == 1
    assert "64-bit" in raw.unetseg_last_error().decode()


def test_flips_are_valid_on_any_rectangle():
    """the even-r views need no square input: a rectangular call gets past the geometry check of a
    quarter turn and is refused only for its offsets"""
    raw = _raw()
    for mask in (0x01, 0x02, 0x10, 0x20, 0x03, 0x33):
        assert raw.unetseg_tta_views(PTR, BIG, BIG, BIG, 7, mask, PTR, None) == 1
        assert "64-bit" in raw.unetseg_last_error().decode()


def test_modes_are_the_four_masks():
    from unetseg_hip import tta

    assert tta.MODES == {"none": 0x01, "hflip": 0x03, "flips": 0x33, "d4": 0xFF}
    assert tta_ref.ks(tta.MODES["flips"]) == [0, 1, 4, 5]  # identity, mirror, rot180, rot180 of the mirror
    with pytest.raises(ValueError, match="unknown TTA mode"):
        tta.TTA(lambda x: x, "rot")


def test_reference_views_invert_and_turn_counter_clockwise():
    x = torch.arange(1, 10).view(3, 3)  # a ramp: no symmetry of the square maps it to itself
    seen = []
    for k in range(8):
        v = tta_ref.view(x, k)
        assert torch.equal(tta_ref.inverse(v, k), x), k
        assert all(not torch.equal(v, s) for s in seen), k  # eight different views
        seen.append(v)
    assert torch.equal(tta_ref.view(x, 2), torch.rot90(x, 1, (-2, -1)))
    assert torch.equal(tta_ref.view(x, 2), torch.tensor([[3, 6, 9], [2, 5, 8], [1, 4, 7]]))  # right column on top
    assert torch.equal(tta_ref.view(x, 1), torch.tensor([[3, 2, 1], [6, 5, 4], [9, 8, 7]]))
    # view-major order, ascending k
    xb = x[None, None]
    got = tta_ref.views_ref(xb, 0x0A)
    assert torch.equal(got[0, 0], tta_ref.view(x, 1)) and torch.equal(got[1, 0], tta_ref.view(x, 3))


def test_reference_merge_of_one_view_is_log_softmax():
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 4, 5, 5, generator=g, dtype=torch.float64)
    for k in range(8):
        got = tta_ref.merge_ref(tta_ref.view(z, k), 1 << k)
        assert torch.allclose(got, torch.log_softmax(z, 1), atol=1e-12), k
    z1 = z[:, :1]
    assert torch.allclose(tta_ref.merge_ref(tta_ref.view(z1, 3), 0x08), z1, atol=1e-12)
