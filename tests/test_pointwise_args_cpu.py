"""CPU: the argument checks of the narrow 1x1 head, attention-gate, GAP and input-packing entry points
(csrc/pointwise.hip, the strided half of csrc/cls_head.hip; the contract is stated in include/unetseg_hip.h).

Nothing is launched: an empty problem (M == 0, an empty image, an empty batch) returns 0 before any pointer is
looked at, and every refusal happens before the first HIP call, so these run without a device.  The pointers
are the address of a host buffer that no call reads."""
import ctypes
import os

import pytest

_BUF = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_BUF)
BF16, F32 = 1, 0

# entry point -> (ordered (name, value) arguments of a well-formed bf16 call with c = 64 channels, the field that
# makes the problem empty, the required pointers, the strides of operands accessed in 16-B vectors, the strides
# of operands accessed by element)
CALLS = {
    "pw_small_fwd": ([("dtype", BF16), ("x", PTR), ("ldx", 80), ("M", 100), ("hw", 50), ("c", 64), ("k", 2), ("w", PTR),
                      ("b", None), ("y", PTR), ("stats", None), ("stream", None)], "M", ["x", "w", "y"], ["ldx"], []),
    "pw_small_bwd": ([("dtype", BF16), ("dy", PTR), ("x", PTR), ("ldx", 80), ("M", 100), ("hw", 50), ("c", 64), ("k", 2),
                      ("w", PTR), ("dx", PTR), ("lddx", 96), ("dx_acc", 0), ("part_w", PTR), ("part_b", PTR),
                      ("stream", None)], "M", ["dy", "x", "w", "part_w", "part_b"], ["ldx", "lddx"], []),
    "pw_small_bwd_relu": ([("dtype", BF16), ("dy", PTR), ("x", PTR), ("ldx", 80), ("M", 100), ("hw", 50), ("c", 64),
                           ("k", 2), ("w", PTR), ("dx", PTR), ("lddx", 96), ("part_w", PTR), ("part_b", PTR),
                           ("part_d", PTR), ("stream", None)], "M",
                          ["dy", "x", "w", "dx", "part_w", "part_b", "part_d"], ["ldx", "lddx"], []),
    "pw_head_fwd": ([("dtype", BF16), ("x", PTR), ("ldx", 80), ("M", 100), ("hw", 50), ("c", 64), ("k", 5), ("w", PTR),
                     ("b", None), ("y", PTR), ("stream", None)], "M", ["x", "w", "y"], ["ldx"], []),
    "pw_head_bwd": ([("dtype", BF16), ("dy", PTR), ("x", PTR), ("ldx", 80), ("M", 100), ("hw", 50), ("c", 64), ("k", 5),
                     ("w", PTR), ("dx", PTR), ("lddx", 96), ("dx_acc", 0), ("part_w", PTR), ("part_b", PTR),
                     ("stream", None)], "M", ["dy", "x", "w", "part_w", "part_b"], [], ["ldx", "lddx"]),
    "attn_apply": ([("dtype", BF16), ("skip", PTR), ("lds", 80), ("psi", PTR), ("sc", PTR), ("sh", PTR), ("alpha", PTR),
                    ("gated", PTR), ("ldg", 96), ("M", 100), ("c", 64), ("stream", None)], "M",
                   ["skip", "psi", "sc", "sh", "alpha", "gated"], ["lds", "ldg"], []),
    "attn_bwd1": ([("dtype", BF16), ("dg", PTR), ("ldg", 80), ("skip", PTR), ("lds", 96), ("alpha", PTR), ("psi", PTR),
                   ("mean", PTR), ("inv", PTR), ("dskip", PTR), ("ldds", 112), ("ds_acc", 0), ("dpsibn", PTR), ("M", 100),
                   ("c", 64), ("part", PTR), ("stream", None)], "M",
                  ["dg", "skip", "alpha", "psi", "mean", "inv", "dskip", "dpsibn", "part"], ["ldg", "lds", "ldds"], []),
    "attn_bwd2": ([("dtype", BF16), ("dpsibn", PTR), ("psi", PTR), ("mean", PTR), ("inv", PTR), ("coef", PTR), ("f", PTR),
                   ("ldf", 80), ("wpsi", PTR), ("dzf", PTR), ("lddz", 96), ("M", 100), ("c", 64), ("part_w", PTR),
                   ("part_b", PTR), ("stream", None)], "M",
                  ["dpsibn", "psi", "mean", "inv", "coef", "f", "wpsi", "dzf", "part_w", "part_b"], ["ldf", "lddz"], []),
    "gap_fwd": ([("dtype", BF16), ("x", PTR), ("ldx", 80), ("B", 2), ("HW", 9), ("c", 64), ("g", PTR), ("stream", None)],
                "B", ["x", "g"], [], ["ldx"]),
    "gap_bwd": ([("dtype", BF16), ("dg", PTR), ("B", 2), ("HW", 9), ("c", 64), ("dx", PTR), ("ldx", 80), ("accumulate", 0),
                 ("stream", None)], "B", ["dg", "dx"], [], ["ldx"]),
    "pack_input": ([("dtype", BF16), ("x", PTR), ("n", 2), ("c", 3), ("h", 4), ("w", 5), ("cpad", 8), ("y", PTR),
                    ("stream", None)], "n", ["x", "y"], [], []),
    "pack_input_stem": ([("x", PTR), ("n", 2), ("c", 3), ("h", 4), ("w", 5), ("y", PTR), ("stream", None)], "n",
                        ["x", "y"], [], []),
}


@pytest.fixture(scope="module")
def raw():
    from unetseg_hip import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libunetseg_hip.so not built")
    return lib.load()


def _call(raw, name, **change):
    args = dict(CALLS[name][0])
    assert set(change) <= set(args), (name, change)
    args.update(change)
    return getattr(raw, "unetseg_" + name)(*(args[k] for k, _ in CALLS[name][0]))


def _refused(raw, name, *words, **change):
    assert _call(raw, name, **change) != 0, (name, change)
    err = raw.unetseg_last_error().decode()
    assert name in err and all(w in err for w in words), (name, change, err)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_empty_problem_returns_zero_without_a_launch(raw, name):
    """M == 0 (an empty batch for GAP, an empty image for the packers): 0, whatever the pointers -- an empty torch
    tensor's pointer is null"""
    args, empty, ptrs, _, _ = CALLS[name]
    assert _call(raw, name, **{empty: 0}) == 0
    assert _call(raw, name, **{empty: 0}, **{p: None for p in ptrs}) == 0
    if name in ("pack_input", "pack_input_stem"):
        for dim in ("h", "w"):
            assert _call(raw, name, **{dim: 0, "x": None, "y": None}) == 0
    if name == "gap_bwd":
        assert _call(raw, name, HW=0, dg=None, dx=None) == 0
    if name == "gap_fwd":  # a mean over no pixels is no empty problem
        _refused(raw, name, "HW=0", HW=0)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_null_pointers_are_refused(raw, name):
    for p in CALLS[name][2]:
        _refused(raw, name, **{p: None})


@pytest.mark.parametrize("name", sorted(CALLS))
def test_strides_are_checked(raw, name):
    """ld is in elements and at least c; where the kernel moves 16-byte vectors, a multiple of 8 (bf16) / 4 (fp32)"""
    _, _, _, vec, elem = CALLS[name]
    for ld in vec + elem:
        _refused(raw, name, "at least", **{ld: 56})
        _refused(raw, name, "at least", **{ld: 0})
    for ld in vec:
        _refused(raw, name, "multiple of the 16-B vector", **{ld: 68})   # a multiple of 4, not of 8
        if name != "pw_small_bwd_relu":  # bf16 only
            _refused(raw, name, "multiple of the 16-B vector", **{ld: 66, "dtype": F32})
    if name in ("pw_small_bwd", "pw_head_bwd"):
        # dx == NULL: lddx is not looked at (the op layer passes 0).  Shown through the check that follows it.
        _refused(raw, name, "bad pixel counts", dx=None, lddx=0, M=-1)


def test_small_head_output_counts(raw):
    """pw_small_bwd ran its two-output kernel for any k != 1"""
    for name in ("pw_small_fwd", "pw_small_bwd", "pw_small_bwd_relu"):
        for k in (0, 3, -1):
            _refused(raw, name, "k must be 1 or 2", k=k)
    for name in ("pw_head_fwd", "pw_head_bwd"):
        for k in (0, 33):
            _refused(raw, name, "k=", k=k)


def test_sizes_the_kernels_cannot_take(raw):
    _refused(raw, "pw_small_fwd", "power of two", c=8 * 128, ldx=8 * 128)   # C/V > 64
    _refused(raw, "pw_small_fwd", "power of two", c=8 * 3, ldx=80)
    _refused(raw, "pw_small_bwd", "bad C", c=8 * 3)
    _refused(raw, "pw_small_bwd", "bad C", c=8 * 512, ldx=8 * 512, lddx=8 * 512)
    _refused(raw, "pw_small_bwd_relu", "bf16 only", dtype=F32)
    _refused(raw, "pw_head_bwd", "divide 256", c=48)
    _refused(raw, "pw_head_fwd", "multiple of the 16-B vector", c=12)
    _refused(raw, "attn_bwd1", "power of two", c=48)
    _refused(raw, "attn_bwd2", "bad C", c=8 * 3)
    for name in ("pw_small_fwd", "pw_small_bwd", "pw_small_bwd_relu", "pw_head_fwd", "pw_head_bwd"):
        _refused(raw, name, "bad pixel counts", M=-1)
        _refused(raw, name, "bad pixel counts", hw=0)
    for name in ("attn_apply", "attn_bwd1", "attn_bwd2"):
        _refused(raw, name, "bad pixel counts", M=-1)
        _refused(raw, name, "dtype", dtype=2)
    _refused(raw, "pack_input", "cpad", cpad=2)
    _refused(raw, "pack_input_stem", "c=9", c=9)
    _refused(raw, "pack_input_stem", "c=0", c=0)
    _refused(raw, "pack_input_stem", "h=-1", h=-1)
    _refused(raw, "gap_fwd", "B=-1", B=-1)
    _refused(raw, "gap_bwd", "C=0", c=0)
