"""The resident (device) transcript set, CPU tier: the ABI surface of ald_tset_dev_*, no CPU fallback, and the larger reference
fixture tests/golden/ref_tset_resident.json.gz (made by tests/golden/make_golden_dev_tset.py from oracle/_ref/ref_tset, the reference's
own transcript_set.cc) validated against the host sink, itself pinned to the reference by tests/test_tset_cpu.py."""
import json
import os
import re
import subprocess
import sys

import pytest

import aletsch_amd as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_dev_tset as mk  # noqa: E402
ENTRY_POINTS = ["ald_tset_dev_create", "ald_tset_dev_destroy", "ald_tset_dev_add_batch", "ald_tset_dev_add_stream", "ald_tset_dev_merge",
                "ald_tset_dev_size", "ald_tset_dev_export", "ald_tset_dev_snapshot", "ald_tset_dev_stats"]


def as_groups(groups):
    return [(sid, [(st, cov, conf, abd, c1, tid, [tuple(e) for e in ex]) for st, cov, conf, abd, c1, tid, ex in ts]) for sid, ts in groups]


def check(items, want):
    assert len(items) == len(want)
    for a, b in zip(items, want):
        for k in ("hash", "count", "coverage", "cov2", "conf", "abd", "count1", "count2", "tid"):
            assert a[k] == b[k], (k, a, b)
        assert [list(e) for e in a["exons"]] == b["exons"]
        assert len(a["samples"]) == len(b["samples"]) == a["count2"]
        for x, y in zip(a["samples"], b["samples"]):
            for k in ("sid", "cov2", "conf", "abd", "count1"):
                assert x[k] == y[k], (k, x, y)
            assert y["coverage"] == a["coverage"] and y["count2"] == a["count2"]


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "aletsch_decomp.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", A.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ald_\w+)", syms))
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(A.DecompError) as e:
        A.DeviceTranscriptSet(0)
    assert e.value.code == -2                                        # ALD_ERR_NO_DEVICE
    import ctypes as C
    h = C.c_void_p()
    assert A.load_library().ald_tset_dev_create(0, C.c_double(0.8), C.byref(h)) == -2 and not h.value


def test_host_sink_reproduces_the_resident_fixture():
    """validates the fixture: the host sink fed the same groups gives the reference's items; the cases are large and keep hitting old items"""
    cases = mk.load()
    assert [len(g) for g, _ in cases] == [2000, 10000]
    for groups, items in cases:
        s = A.TranscriptSink(0.8); s.add_groups(as_groups(groups))
        check(s.items(), items)
        assert max(x["count"] for x in items) >= 100 and max(len(x["samples"]) for x in items) == 8
        assert any(len(x["exons"]) == 1 for x in items) and any(len(x["exons"]) >= 6 for x in items)


def test_resident_fixture_matches_live_reference_build():
    """where build() could make oracle/_ref/ref_tset, the reference asked again gives the stored sets (a live pin); elsewhere the stored
    cases stand in"""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_tset")
    cases = mk.load()
    if os.path.exists(exe):
        assert [mk.mg.tset_parse(o) for o in mk.reference_outputs(exe)] == [items for _, items in cases]
    assert len(cases) == 2
