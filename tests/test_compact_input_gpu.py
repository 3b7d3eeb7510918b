"""GPU tier: compact input (ald_params.reserved & ALD_PARAM_COMPACT_INPUT) -- columns of a batch that follow from its other columns are
derived on the device (aletsch_amd/csrc/input_expand.h) instead of copied to it.

1. tests/compact_input_gpu_main.hip runs every case of tests/compact_input_cases.h (the list of the CPU tier) through the expand kernels
   and compares every section of the device buffer with the host's staging, byte for byte.
2. The seeded mix of tests/class_cases.py, the hub batch of tests/shapes.py and a raw batch give the same answer with the bit set and
   with it clear: status, path and iteration counts, every record the result index names (all of its words) and the index's shape, op
   traces, every field of the features_all tables bit for bit, ald_batch_algorithmic_bytes.  WHERE a record lies in the pool is decided by which
   wave bumps the pool pointer first and differs between two runs of the same build, so the records are compared through the index:
   record (g, p) of one run against record (g, p) of the other, word for word, and the totals of both.
3. One batch object reused: compact upload, run, download, clear, other graphs, upload, run == a fresh batch.
4. ALD_COMPACT_INPUT=1 switches the mode on without the bit, ALD_COMPACT_INPUT_LOG=1 shows what was elided; ALD_COMPACT_INPUT=0 wins
   over the bit.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aletsch_amd as A
from aletsch_amd.distributed import REC_HDR_WORDS
import class_cases as CC
import common
import shapes

pytestmark = pytest.mark.gpu
ROOT = common.ROOT


def _params(compact, base=None):
    p = base if base is not None else A.default_params()
    q = A.AldParams.from_buffer_copy(p)
    q.reserved = A.PARAM_COMPACT_INPUT if compact else 0
    return q


# ---- 1: the kernels against the host's staging ----
def test_expand_kernels_fill_every_section_as_the_host_does():
    bld = os.path.join(ROOT, "tests", "_build"); os.makedirs(bld, exist_ok=True)
    exe = os.path.join(bld, "compact_input_gpu_main")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "compact_input_gpu_main.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-6000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "0 failures" and len(lines) > 25 and all(ln.startswith("ok ") for ln in lines[:-1]), r.stdout[-6000:]


# ---- 2: parity through the C ABI ----
def _records_by_index(b, npaths):
    """record (g, p) for every path, through the index the kernel wrote -> (list of word arrays in (graph, path) order, pool words in use)"""
    raw = b.raw_records(); idx, gf = b.result_index()
    out = []
    for g in range(b.n):
        for p in range(int(npaths[g])):
            o = int(idx[int(gf[g]) + p]); nv, nx = int(raw[o + 2]), int(raw[o + 14])
            out.append(raw[o:o + ((REC_HDR_WORDS + nv + nx + 1) & ~1)])
    return out, int(raw.size), int(idx.size)


def _features_of(b, g):
    try:
        fs, c, rc = b.features(g)
    except A.DecompError as e:
        return ("error", e.code)
    return (b"".join(bytes(x) for x in fs), c.tobytes(), rc)


def _answer(stage, params, n_trace=0, raw_features_on_device=False):
    with A.DecompBatch(0, params, trace_events=CC.TRACE_CAP if n_trace else 0) as b:
        stage(b)
        b.upload(); b.run(); b.download()
        st, npth, nit = b.status_arrays()
        recs, words, entries = _records_by_index(b, np.where((st == 0) | (st == 1), npth, 0))
        ans = dict(status=st.copy(), npaths=npth.copy(), iters=nit.copy(), iterations=b.iterations().copy(), recs=recs, words=words, entries=entries,
                   traces=[b.trace(g) for g in range(0, min(b.n, n_trace), CC.TRACE_STRIDE)], bytes=b.algorithmic_bytes())
        f = b.features_all(raw_on_device=raw_features_on_device)
        ans["feat"] = {k: f[k].tobytes() for k in ("complete", "graph_rc", "row_begin")}
        # every FIELD of every row bit for bit.  Not the 4-byte holes between the fields: the kernel stores end_cnt with a dwordx2 whose upper
        # half is the old content of a register, so two runs of the SAME build differed there (seen with the parent commit's library too)
        ans["feat"]["rows"] = {name: np.ascontiguousarray(f["rows"][name]).tobytes() for name in f["rows"].dtype.names}
        ans["feat_one"] = [_features_of(b, g) for g in range(0, b.n, max(1, b.n // 7))]      # the per-graph host routine reads the in-CSR, which a compact batch builds on demand
    return ans


def _same(a, b, what):
    for k in ("status", "npaths", "iters", "iterations"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["words"] == b["words"] and a["entries"] == b["entries"] and len(a["recs"]) == len(b["recs"]), what
    for i, (x, y) in enumerate(zip(a["recs"], b["recs"])):
        assert np.array_equal(x, y), (what, "record", i)
    assert a["traces"] == b["traces"], (what, "op trace")
    assert a["feat"] == b["feat"], (what, "features_all")
    assert a["feat_one"] == b["feat_one"], (what, "ald_batch_features")
    assert a["bytes"] == b["bytes"], (what, "algorithmic bytes")


def _add_raw_items(items):
    def stage(b):
        for pg, phases, dist in items:
            assert b.add_raw(pg, phases, dist) == 0
    return stage


@pytest.mark.parametrize("part", ["staged", "second", "hub", "raw", "raw_features_on_device", "raw_and_staged", "uniform_defaults"])
def test_same_answer_with_the_bit_set_and_clear(part):
    base = CC.second_params() if part == "second" else None
    dev = part == "raw_features_on_device"
    if part == "staged":
        stage = lambda b: b.add(CC.staged_batch())
    elif part == "second":
        stage = lambda b: b.add(CC.second_batch())
    elif part == "hub":
        stage = lambda b: b.add(shapes.hub_batch()[0])
    elif part == "uniform_defaults":                      # every derivable column derived: the sample lists and the four defaults as well
        stage = lambda b: b.add(uniform_of(CC.staged_batch()), omit=("edge_abd", "vertex_type", "edge_strand"))
    elif part == "raw_and_staged":
        def stage(b):
            _add_raw_items(CC.raw_part()["items"][:10])(b); b.add(CC.staged_batch().select(np.arange(0, 20))); _add_raw_items(CC.raw_part()["items"][10:16])(b)
    else:
        stage = _add_raw_items(CC.raw_part()["items"])
    n_trace = 64 if part in ("staged", "second", "raw", "uniform_defaults") else 0
    full = _answer(stage, _params(False, base), n_trace, dev)
    compact = _answer(stage, _params(True, base), n_trace, dev)
    assert (full["status"] == 0).sum() > 0.5 * full["status"].size, part          # the comparison is about graphs that ran
    _same(full, compact, part)


# ---- 3: reuse of one batch object ----
def uniform_of(pg):
    """the same graphs as assembler::assemble(bundle&) hands them over: one sample per edge, the same one per graph, its abundance the weight"""
    import dataclasses
    E = pg.g_ne.astype(np.int64)
    esoff = np.concatenate([np.arange(e + 1, dtype=np.int32) for e in E])
    return dataclasses.replace(pg, edge_sample_offset=esoff, sample_id=np.repeat(np.arange(pg.n, dtype=np.int32) % 3, E), sample_abd=pg.edge_weight.copy(), edge_count=None, edge_rank=None)


def _result_key(r):
    return (r.status.tobytes(), r.path_offset.tobytes(), r.weight.tobytes(), r.abd.tobytes(), r.conf.tobytes(), r.reads.tobytes(), r.length.tobytes(), r.count.tobytes(), r.path_vertices.tobytes())


def test_one_batch_object_reused():
    first = uniform_of(A.synth(seed=71, n_graphs=300, v_min=6, v_max=50, edges_per_vertex=3))
    second = A.synth(seed=72, n_graphs=200, v_min=6, v_max=40, edges_per_vertex=3, n_samples=3, phasing_per_graph=4)
    prm = _params(True)
    with A.DecompBatch(0, prm) as b:
        b.add(first, omit=("edge_abd", "vertex_type", "edge_strand")); b.upload(); b.run(); b.download(); r1 = _result_key(b.result())
        b.clear()
        b.add(second); b.upload(); b.run(); b.download(); r2 = _result_key(b.result())
    with A.DecompBatch(0, prm) as f:
        f.add(second); f.upload(); f.run(); f.download(); assert _result_key(f.result()) == r2
    with A.DecompBatch(0, _params(False)) as f:
        f.add(first, omit=("edge_abd", "vertex_type", "edge_strand")); f.upload(); f.run(); f.download(); assert _result_key(f.result()) == r1


# ---- 4: the mode is visible, and the environment decides ----
_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import aletsch_amd as A
from test_compact_input_gpu import uniform_of
bit = int(sys.argv[1])
p = A.default_params(); p.reserved = A.PARAM_COMPACT_INPUT if bit else 0
any_batch = A.synth(seed=81, n_graphs=50, v_min=6, v_max=40, edges_per_vertex=3, n_samples=3)
with A.DecompBatch(0, p) as b:
    b.add(any_batch); b.upload(); b.run(); b.download(); print("paths", int(b.result().path_offset[-1]))
    b.clear()
    b.add(uniform_of(any_batch), omit=("edge_abd",)); b.upload(); b.run(); b.download(); print("paths", int(b.result().path_offset[-1]))
"""


def _run_script(bit, env_value):
    env = dict(os.environ, ALD_COMPACT_INPUT=env_value, ALD_COMPACT_INPUT_LOG="1")
    r = subprocess.run([sys.executable, "-c", _SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests")), str(bit)], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout, [ln for ln in r.stderr.splitlines() if "compact upload" in ln]


def test_the_environment_switches_the_mode_and_the_log_line_shows_it():
    out_on, lines = _run_script(0, "1")
    assert len(lines) == 2, lines
    m = [re.search(r"elided((?: [A-Z]+)*) sent (\d+) full (\d+)", ln) for ln in lines]
    assert all(m), lines
    e0, e1 = m[0].group(1).split(), m[1].group(1).split()
    assert e0[:2] == ["INOFF", "INEDGE"] and not set(e0) & {"ESOFF", "SID", "SABD", "EABD"}, lines[0]      # three samples an edge, and A.synth supplies edge_abd (not edge_count)
    assert e1[:7] == ["INOFF", "INEDGE", "ESOFF", "SID", "SABD", "EABD", "ECOUNT"], lines[1]
    for x in m:
        assert 0 < int(x.group(2)) < int(x.group(3)), lines
    out_off, lines = _run_script(1, "0")
    assert lines == []
    assert out_on == out_off and out_on.count("paths") == 2
