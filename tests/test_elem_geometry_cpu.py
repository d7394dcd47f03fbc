"""CPU: the launch geometry of the memory-bound op families, pinned through the host-only queries of the C ABI.

tools/record_elem_geometry.py asks every size query of csrc/elem.hip, upsample.hip, pointwise.hip, resize.hip and
the loss files (reduction tiles, the upsample backward's partial rows, the pointwise pixel tiles, the loss
workspaces) over a fixed shape list -- every model's activation shapes at the bench sizes in both dtypes and the
edges each rule turns on -- once per knob setting, each in a process of its own.  tests/golden/
elem_geometry.json holds the answers.  The launches read the same decisions as the queries, so a change of
the host code that moves a shape to another block count fails here, entry by entry, before a GPU is involved.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recording():
    """a fresh recording from the built library (a missing library fails: this gate never skips)"""
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "record_elem_geometry.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


def test_elem_geometry_matches_golden(recording, golden_dir):
    got = recording
    with open(os.path.join(golden_dir, "elem_geometry.json")) as f:
        want = json.load(f)
    assert list(got) == list(want), "the knob settings changed"
    for setting in want:
        assert list(got[setting]) == list(want[setting]), f"{setting}: the queries changed"
        for q, entries in want[setting].items():
            assert list(got[setting][q]) == list(entries), f"{setting} / {q}: the shape list changed"
            bad = [(k, v, got[setting][q][k]) for k, v in entries.items() if got[setting][q][k] != v]
            assert not bad, (f"{setting} / {q}: {len(bad)} of {len(entries)} entries differ (key, golden, now), "
                             f"first 10: {bad[:10]}")


def test_knobs_reach_the_queries(recording):
    """the two per-call knobs are read by the library as built: each changes some answer of its query"""
    base = recording["unset"]
    for setting, family in (("UNETSEG_RED_TARGET=2048", "reduce_tiles"), ("UNETSEG_UP_STREAM=0", "up_bwd_tiles")):
        assert list(recording[setting]) == [family]
        assert list(recording[setting][family]) == list(base[family])
        assert recording[setting][family] != base[family]
