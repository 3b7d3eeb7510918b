"""GPU tier of the hub shapes (tests/shapes.py): the batch whose census (tests/test_hub_shapes_cpu.py, taken in the oracle) reaches every star
and router form of the kernel, through the product library against the oracle.  Here the wave-parallel forms run that the single-lane
emulation cannot: star_reg (fans of up to STAR_MAX edges in registers), the lane-parallel parts of star_fixed, router_prepare.
Bit-exact as every parity test: identical paths in identical order, weight / abd / reads bit-identical, conf within 1e-9 relative."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aletsch_amd as A
import common
import device_run as DR
import shapes
from test_batch_features_gpu import assert_tables_equal, host_table

pytestmark = pytest.mark.gpu

K = shapes.kernel_constants()
_MEMO = {}


def oracle(pg, params=None):
    if id(pg) not in _MEMO:
        _MEMO[id(pg)] = shapes.census_of(pg, threads=DR.THREADS, params=params)
    return _MEMO[id(pg)]


def batches():
    """(name, batch, parameters): the hub batch under the default parameters, the wide routers without phasing lists under theirs"""
    pg, _ = shapes.hub_batch(); wpg, _, wp = shapes.wide_router_batch()
    return (("hubs", pg, None), ("wide routers", wpg, wp))


def test_hub_batches_match_oracle():
    """records, statuses (all 0) and iteration counts of both batches"""
    for name, pg, prm in batches():
        want, st, _ = oracle(pg, prm)
        r = DR.run(pg, prm)
        bad = DR.oracle_mismatches(name, r, want, st[:, 3])
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
        assert int((r.result.status != 0).sum()) == 0, name


def test_hubs_with_a_zero_count_edge_on_gpu():
    """edge_info.count == 0 on a hub edge that a route covers: router_prepare's iso == 2 branch, then one of the reference's asserts.  Every
    graph of this batch ends on such an assert and has no records: the status word is compared, and the op trace up to the assert -- the
    router that fired on the hub before it, with its vertex, type and leftover ratio."""
    pg, _ = shapes.zero_count_batch()
    want, _, _ = oracle(pg)
    traces = common.oracle_run(pg, threads=DR.THREADS, trace=True)[3]
    r = DR.run(pg, trace_cap=4096)
    bad = DR.oracle_mismatches("zero counts", r, want, None, traces)
    assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
    assert (r.result.status >= 100).all()
    assert sum(1 for t in traces if any(ev[0] in (7, 8) for ev in t)) >= 10            # a router did fire before the assert (OP_UNSPLIT_NOW / _BEST)


def trace_subset(pg, per_graph, traces_len, cap):
    """graphs that cover every fan-size bucket in both directions and every router bucket at least once, plus every 9th graph"""
    pick = set(range(0, pg.n, 9)); have = set()
    for g, cen in enumerate(per_graph):
        for key in cen:
            names = [("fan", shapes.fan_bucket(key[2], K), key[1])] if key[0] == 0 else [("router", b) for b in shapes.router_buckets(key, K)]
            for nm in names:
                if nm not in have and traces_len[g] <= cap:
                    have.add(nm); pick.add(g)
    return np.array(sorted(g for g in pick if traces_len[g] <= cap)), have


def test_op_trace_of_the_hubs_on_gpu():
    """rule id / vertex or edge id / ratio of every firing, in order, on a subset that holds every census bucket at least once"""
    cap = 8192; seen = set()
    for name, pg, prm in batches():
        _, st, per_graph = oracle(pg, prm)
        idx, have = trace_subset(pg, per_graph, st[:, 3], cap - 64)
        seen |= have
        sub = pg.select(idx)
        want, st, _, traces = common.oracle_run(sub, threads=DR.THREADS, trace=True, params=prm)
        bad = DR.oracle_mismatches(name, DR.run(sub, prm, trace_cap=cap), want, st[:, 3], dict(zip(idx.tolist(), traces)), traced=idx)
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
    fans = {(fb, d) for fb in shapes.fan_buckets(K) for d in (0, 1)} - {("1", 1)}
    assert fans <= {(x[1], x[2]) for x in seen if x[0] == "fan"}
    # every router bucket of the census; the zero-count one lives in the batch test_hubs_with_a_zero_count_edge_on_gpu traces whole
    want_routers = set(shapes.Census([], [], [], K).router_names()) - {"routes, count 0"}
    assert want_routers <= {x[1] for x in seen if x[0] == "router"}, want_routers - {x[1] for x in seen if x[0] == "router"}


def test_graphs_of_twin_size_on_the_twins_and_off(monkeypatch):
    """the graphs whose class has a slab-resident twin, forced onto the twins and kept off them"""
    pg, _ = shapes.hub_batch()
    _, _, cl = common.emu_run(pg)
    idx = np.nonzero(np.isin(cl, list(K["TWINS"])))[0]
    assert idx.size >= 20
    sub = pg.select(idx); want = common.oracle_run(sub, threads=DR.THREADS)[0]
    for force in ("1", "0"):
        monkeypatch.setenv("ALD_DEBUG_TWIN", force)
        r = DR.run(sub)
        assert not DR.oracle_mismatches("twins " + force, r, want, want_classes=(set(K["TWINS"].values()) if force == "1" else set(K["TWINS"])) | {9})
        assert (r.result.status == 0).all()


def test_hub_batches_started_one_class_too_low():
    """ALD_DEBUG_UNDERCLASS=1: the wide hubs outgrow the class they start in and are re-queued one class up"""
    for name, pg, prm in batches():
        want, _, _ = oracle(pg, prm)
        plain = DR.run(pg, prm).classes
        r = DR.run(pg, prm, env={"ALD_DEBUG_UNDERCLASS": "1"}); used = r.classes
        assert not DR.oracle_mismatches(name, r, want), name
        assert (r.result.status == 0).all(), name
        lowered = {}
        for c, k in plain.items(): lowered[max(c - 1, 0)] = lowered.get(max(c - 1, 0), 0) + k
        print(name, "classes: plain", plain, "started one lower", lowered, "ended in", used)
        assert sum(used.values()) == pg.n and used != lowered, (name, used)                  # some graphs had to climb back up


def test_hub_batches_through_the_variant_builds():
    """the STARREG build (fans of 2..4 through star_reg instead of star_fixed), the WSYNC build (full drain at every hand-over, kept sweep
    records in every class) and the ROWS build (adjacency rows): tools/hub_parity.py, one child process per library, as
    test_gpu_parity.py runs its fuzz slices through them"""
    libs = [os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_%s.so" % n) for n in ("starreg", "wsync", "rows")]
    for lib in libs:
        assert os.path.exists(lib), "build it with python __graft_entry__.py"
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "hub_parity.py"), *libs], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    totals = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("TOTAL graphs")]
    assert len(totals) == 3 and all(ln.strip().endswith("mismatches 0") for ln in totals), r.stdout[-2500:]


def test_raw_hub_graphs_through_the_device_pre_steps():
    """hub graphs handed over raw (add_raw, phases as exon-coordinate lists): the wave that loads a graph folds the boundary edges at the source
    and the sink -- where hubs live -- before it decomposes it; against the oracle's pre-steps + decomposition"""
    import test_hub_shapes_cpu as T
    from aletsch_amd.packed import PackedGraphs
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    items, staged, ok = T.raw_items(O, stride=3)
    ok = np.array(ok)
    got = DR.run(items, raw=True).result
    assert len(items) > 300 and ok.sum() >= 0.9 * len(ok)
    want = common.oracle_run(PackedGraphs.concat(staged), threads=DR.THREADS)[0]
    assert not common.compare_results(want, common.select_results(got, np.nonzero(ok)[0]), len(staged), conf_tol=1e-9)
    assert (got.status[~ok] >= 100).all()
    emu, _ = common.emu_run_raw(items)
    assert not common.compare_results(emu, got, len(items), conf_tol=1e-9)


def test_feature_block_of_the_hubs_at_three_lds_budgets(monkeypatch):
    """features_all against the per-graph host routine.  Hub graphs have more paths than the wave has lanes (65..300 and more), so the
    lane-stride loops of features_graph go round more than once; the junction lists go to LDS or to the scratch by 2 np + 2 sum(max(nv - 3, 0))
    against the budget: the full budget, none, and one in between under which one launch holds graphs of both kinds."""
    pg, _ = shapes.hub_batch()
    want_o, _, _ = oracle(pg)
    npaths = np.diff(want_o.path_offset); nv = np.diff(want_o.pv_offset)
    need = np.array([2 * int(npaths[g]) + 2 * int(np.maximum(nv[want_o.path_offset[g]:want_o.path_offset[g + 1]] - 3, 0).sum()) for g in range(pg.n)])
    assert int(npaths.max()) > 64
    lo, hi = int(need[need > 0].min()), int(need.max())
    mid = int(np.median(need[need > 0]))
    assert 0 < mid < K["FT_LDS_WORDS"] and hi > 0                                          # (the knob is ignored outside 0 .. FT_LDS_WORDS - 1)
    assert lo <= mid < hi and (need <= mid).any() and (need > mid).any()                 # graphs of both kinds within the one launch
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        want = host_table(b, pg.n)
        assert want[0].size == int(npaths.sum())
        for budget in (None, "0", str(mid)):
            if budget is None: monkeypatch.delenv("ALD_DEBUG_FEAT_LDS", raising=False)
            else: monkeypatch.setenv("ALD_DEBUG_FEAT_LDS", budget)
            got = b.features_all(None, g_nv=pg.g_nv)
            assert_tables_equal(got, want)
            assert got["stats"]["device_graphs"] == pg.n, budget
        monkeypatch.delenv("ALD_DEBUG_FEAT_LDS", raising=False)


def test_hub_transcripts_into_the_device_set():
    """star graphs give many transcripts that share the first and the last exon and differ in one exon in between (the compare1 walk inside
    one bucket): the device-resident set against the host sink after the add"""
    pg, _ = shapes.hub_batch()
    rng = np.random.default_rng(5)
    sid = rng.integers(-1, 8, pg.n).astype(np.int32)
    for skip in (False, True):
        host = A.TranscriptSink(0.8)
        with A.DeviceTranscriptSet(0, 0.8) as ds, A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            host.add_batch(b, sid, tid_base=0, skip_single_exon=skip)
            ds.add_batch(b, sid, tid_base=0, skip_single_exon=skip)
            got, want = ds.items(), host.items()
        assert len(got) == len(want) and len(want) > 3000
        for x, y in zip(got, want):
            assert x == y, (skip, x, y)
