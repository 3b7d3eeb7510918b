"""GPU tier of the size-class matrix: each of the 28 decomposition kernels (14 size classes, plain and raw build) against the oracle on the
mix of tests/class_cases.py.

ALD_DEBUG_FIRST_CLASS=c (decomp_common.h: debug_first_class) gives pick_class() its first class, so the small graphs of the mix run in the
kernel of class c; the twins 11 / 12 are reached as 7 / 8 with ALD_DEBUG_TWIN=1.  Every run is a fresh DecompBatch: all of its graphs must
have run in the expected class and in no other (a graph of more than 32 vertices runs in class 1 when class 0 comes first), records equal
to the oracle's (conf within 1e-9, as everywhere in this tier), statuses, iteration counts, and the op trace on every fourth graph.  tests/test_class_matrix_cpu.py runs the same mix through the emulation and
asserts the census of what it exercises."""
import time

import numpy as np
import pytest

import aletsch_amd as A
import class_cases as CC
import common
import device_run as DR

pytestmark = pytest.mark.gpu

# (first class, ALD_DEBUG_TWIN, the class the graphs must end in)
KERNELS, IDS = DR.forced_kernels(CC.CLASSES, twins=(11, 12))


def _expected(part, first, cls):
    """class_cases.expected_classes, with the twin in the place of its LDS class"""
    want = CC.expected_classes(part, first).copy()
    want[want == first] = cls
    assert (want == cls).sum() >= 20
    return want


def test_census_of_the_mix_on_this_machine():
    """the census both tiers assert: counted by the oracle, at least 10 events a line"""
    print("\ncensus of the class mix (events per line, from the oracle):\n" + CC.census_table())
    short = {k: v for k, v in CC.census().items() if v < CC.MIN_EVENTS}
    assert not short, short


@pytest.mark.parametrize("part", ["staged", "second"])
@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_plain_kernel_matches_oracle(first, twin, cls, part):
    o = CC.oracle_of(part); pg = o["pg"]; prm = o["params"]
    assert max(len(t) for t in o["traces"]) <= CC.TRACE_CAP
    exp = _expected(part, first, cls)
    traced = np.arange(0, pg.n, CC.TRACE_STRIDE)
    assert len(traced) <= DR.HUGE_BATCH
    for idx, cap in [(idx, 0) for idx in DR.in_chunks(pg.n, cls)] + [(traced, CC.TRACE_CAP)]:
        r = DR.run(pg.select(idx), prm, first=first, twin=twin, trace_cap=cap)
        bad = DR.oracle_mismatches(f"class {cls}, {part}", r, common.select_results(o["res"], idx), o["iters"][idx], o["traces"] if cap else None,
                                   traced=idx, want_classes=DR.class_counts(exp[idx]))
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
    print(f"class {cls:2d} plain, {part}: {pg.n} graphs, 0 mismatches")


@pytest.mark.parametrize("part", ["raw", "raw2"])
@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_raw_kernel_matches_oracle(first, twin, cls, part):
    """the raw build of class `cls`: pre_assemble_device in the load phase, then the decomposition, against the oracle's pre-steps +
    decomposition under both parameter sets; an item on which the oracle's pre-steps assert ends with a status >= 100"""
    raw = CC.raw_part(); o = CC.oracle_of(part); prm = o["params"]; ok = raw["ok"]; items = raw["items"]
    staged_index = np.cumsum(ok) - 1                      # item -> index among the oracle's staged graphs (where ok)
    exp = _expected(part, first, cls)
    traced = np.nonzero(ok)[0][::CC.TRACE_STRIDE]
    for idx, cap in [(idx, 0) for idx in DR.in_chunks(len(items), cls)] + [(traced, CC.TRACE_CAP)]:
        r = DR.run([items[int(i)][:3] for i in idx], prm, first=first, twin=twin, raw=True, trace_cap=cap)
        okc = ok[idx]; sidx = staged_index[idx][okc]
        assert (r.result.status[~okc] >= 100).all(), (cls, r.result.status[~okc])
        mine = r._replace(result=common.select_results(r.result, np.nonzero(okc)[0]), iterations=r.iterations[okc], traces=[t for t, k in zip(r.traces, okc) if k])
        want = common.select_results(o["res"], sidx)
        want_it = np.where(want.status == 0, o["iters"][sidx], mine.iterations)       # (iteration counts: of the graphs that end with status 0)
        bad = DR.oracle_mismatches(f"raw class {cls}, {part}", mine, want, want_it, o["traces"] if cap else None, traced=sidx, want_classes=DR.class_counts(exp[idx]))
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
    print(f"class {cls:2d} raw, {part}: {len(items)} graphs, 0 mismatches")


def test_natural_size_of_the_large_classes_with_the_features_on():
    """two graphs each at the natural size of classes 9, 10 and 13 with phasing paths, three samples, strands and touching exons"""
    pg = CC.natural_size_batch()
    want, st, _, _ = common.oracle_run(pg, threads=CC.THREADS)
    r = DR.run(pg)
    assert [r.classes.get(c) for c in (9, 10, 13)] == [2, 2, 2]
    assert not DR.oracle_mismatches("natural size", r, want, st[:, 3])


def test_large_raw_graphs_match_oracle():
    """raw graphs of class-10 size through the device pre-steps and the decomposition, against the oracle's"""
    items, staged = CC.large_raw_items()
    want, st, _, _ = common.oracle_run(staged, threads=CC.THREADS)
    r = DR.run(items, raw=True)
    assert not DR.oracle_mismatches("large raw", r, want, st[:, 3], want_classes={10: len(items)})


def test_creation_ids_on_both_sides_of_16_bits():
    """the id-width pair of class 13 (creation ids that end above and just below 65 535) on the device, against the EMULATION: the oracle
    needs half a minute for each of the two, and tests/test_class_matrix_cpu.py pins the emulation to it on the same graphs"""
    pg = CC.id_width_batch()
    want, wit, cl = common.emu_run(pg)
    assert (cl == 13).all()
    t0 = time.perf_counter()
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.result(); it = b.iterations(); ms = b.kernel_ms()
        assert b.class_info(13)["n_graphs"] == 2
    print(f"\nid-width pair on the device: kernel {ms:.0f} ms, whole batch {time.perf_counter() - t0:.2f} s")
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert np.array_equal(got.status, want.status) and np.array_equal(it, wit)
