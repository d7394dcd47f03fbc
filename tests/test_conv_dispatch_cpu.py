"""CPU: the conv dispatch rules of csrc/conv.hip, pinned through the host-only queries of the C ABI.

tools/record_conv_dispatch.py asks every dispatch query (kernel configuration, row tile, split-K slabs,
workspace, partial rows of the fused data gradients, the stem's) over a fixed shape list -- the shapes of
tests/test_gpu_configs.py's cases, a thinned grid of channel counts / sizes / filter geometries in both dtypes
with and without a second source and padded pixel strides, and a few shapes past the 2^31-byte extent -- and
tests/golden/conv_dispatch.json holds its answers.  The queries need no device (the CU count then falls
back to 256, the MI355X's), so any change of the host code that moves a shape to another kernel, tile
or split count fails here, entry by entry, before a GPU is involved.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_dispatch_matches_golden(golden_dir):
    import torch

    from unetseg_hip import LIB_PATH
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built")
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != 256:
            pytest.skip(f"device reports {cus} CUs; the recording assumes 256 (the persistent kernels' tile "
                        "counts depend on it)")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "record_conv_dispatch.py")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout)
    with open(os.path.join(golden_dir, "conv_dispatch.json")) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for sec in want:
        assert list(got[sec]) == list(want[sec]), f"{sec}: the shape list changed"
        bad = [(k, want[sec][k], got[sec][k]) for k in want[sec] if got[sec][k] != want[sec][k]]
        assert not bad, f"{sec}: {len(bad)} of {len(want[sec])} entries differ (key, golden, now), first 10: {bad[:10]}"
