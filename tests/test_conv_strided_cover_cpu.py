"""CPU: the strided conv cases (tests/test_gpu_conv_strided.py) reach every kernel configuration the packed
cases of tests/test_gpu_configs.py reach.

Both sets come from the host-only configuration queries of the C ABI, so no device is needed: a configuration
added to CASES / HALO_CASES / POST3_SHAPES / RELU_BITS_SHAPES / the stem cases there without a strided case here
fails on the CPU.  The strided side is asked with the padded pixel strides its cases run with.
"""
import os

import pytest


def _packed_keys():
    import test_gpu_configs as tgc
    from unetseg_hip import introspect
    keys = tgc.covered_keys()
    (mark,) = [m for m in tgc.test_stem_bench_size.pytestmark if m.name == "parametrize"]
    for N, H, tn, _ in mark.args[1]:
        saved = os.environ.get("UNETSEG_STEM_TN")
        if tn:
            os.environ["UNETSEG_STEM_TN"] = "1"
        try:
            desc = (N, H, H, 3, 0, 64, 7, 7, 2, 3, 8, 0)
            keys.update(introspect.call_configs(("stem_fwd",) + desc))
            keys.add(introspect.call_configs(("stem_wgrad",) + desc)[0])
        finally:
            if saved is None:
                os.environ.pop("UNETSEG_STEM_TN", None)
            else:
                os.environ["UNETSEG_STEM_TN"] = saved
    keys.discard("reduce")  # the split-K reduce follows every weight gradient; it takes no activation operand
    return keys


#: configurations the strided cases reach that no case of test_gpu_configs.py does
BEYOND = {"wgrad:wgrad64x256_row"}


def test_strided_cases_cover_every_configuration():
    from unetseg_hip import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    import test_gpu_conv_strided as tcs
    want, got = _packed_keys(), tcs.strided_keys()
    assert not (tcs.PACKED_ONLY & got), f"PACKED_ONLY lists configurations a strided case reaches: {tcs.PACKED_ONLY & got}"
    missing = sorted(want - got - tcs.PACKED_ONLY)
    assert not missing, f"configurations without a strided case (add one, or list it in PACKED_ONLY with the reason): {missing}"
    assert got | tcs.PACKED_ONLY == want | BEYOND, sorted((got | tcs.PACKED_ONLY) ^ (want | BEYOND))


def test_strided_cases_select_what_they_list():
    """every case's padded strides select the configuration it lists, the same as the packed strides; each
    tensor of a call has its own ld and its own non-zero c0, multiples of 8; every direction has a tail case"""
    from unetseg_hip import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    import test_gpu_conv_strided as tcs
    tails = set()
    for cid, (direction, shape, expect, env, tail) in tcs.STRIDED_CASES.items():
        chs = tcs.operand_channels(direction, shape)
        lay = tcs.layout(chs, tail)
        assert len({ld for ld, _ in lay}) == len(lay) and len({c0 for _, c0 in lay}) == len(lay), (cid, lay)
        for C, (ld, c0) in zip(chs, lay):
            assert c0 > 0 and c0 % 8 == 0 and ld % 8 == 0 and c0 + C <= ld and (c0 + C == ld) == tail, (cid, lay)
        with tcs._environ(env):
            assert tcs.case_keys(direction, shape, lay) == expect, cid
            assert tcs.case_keys(direction, shape, tcs.packed_layout(chs)) == expect, cid
        if tail:
            tails.add(tcs._QUERY[direction][0].split("_post")[0])
    assert tails >= {"fwd", "dgrad", "wgrad", "fwd_bnrelu_in", "wgrad_bnrelu_in"}, tails
