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
from test_pre_steps_cpu import common_select_results

pytestmark = pytest.mark.gpu

# (first class, ALD_DEBUG_TWIN, the class the graphs must end in)
KERNELS = [(c, None, c) for c in CC.CLASSES] + [(7, "1", 11), (8, "1", 12)]
IDS = ["class%d" % k[2] for k in KERNELS]
HUGE_BATCH = 32                             # class 13: ~105 MB of slab per wave, so no batch of it holds more than 32 graphs


def _env(monkeypatch, first, twin):
    monkeypatch.setenv("ALD_DEBUG_FIRST_CLASS", str(first))
    monkeypatch.setenv("ALD_DEBUG_TWIN", twin or "0")         # (the LDS form of classes 7 / 8 where their twins are not asked for)


def _chunks(n, cls):
    step = HUGE_BATCH if cls == 13 else n
    return [np.arange(a, min(a + step, n)) for a in range(0, n, step)]


def _classes_are(b, want):
    """every graph of the batch ran in the class it was sent to, and no graph in any other"""
    used = {c: b.class_info(c)["n_graphs"] for c in range(14)}
    exp = {c: int((want == c).sum()) for c in range(14)}
    assert used == exp, ({c: k for c, k in used.items() if k}, {c: k for c, k in exp.items() if k})


def _expected(part, first, cls):
    """class_cases.expected_classes, with the twin in the place of its LDS class"""
    want = CC.expected_classes(part, first).copy()
    want[want == first] = cls
    assert (want == cls).sum() >= 20
    return want


def _traces_equal(b, want_traces, idx, what):
    for k, g in enumerate(idx):
        mine = [(c, a, bb, v) for c, a, bb, v in b.trace(k)]; ref = want_traces[int(g)]
        assert mine == ref, f"{what}, graph {int(g)}: first divergence at {next((i for i, (x, y) in enumerate(zip(mine, ref)) if x != y), min(len(mine), len(ref)))}"


def test_census_of_the_mix_on_this_machine():
    """the census both tiers assert: counted by the oracle, at least 10 events a line"""
    print("\ncensus of the class mix (events per line, from the oracle):\n" + CC.census_table())
    short = {k: v for k, v in CC.census().items() if v < CC.MIN_EVENTS}
    assert not short, short


@pytest.mark.parametrize("part", ["staged", "second"])
@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_plain_kernel_matches_oracle(monkeypatch, first, twin, cls, part):
    o = CC.oracle_of(part); pg = o["pg"]; prm = o["params"]
    assert max(len(t) for t in o["traces"]) <= CC.TRACE_CAP
    _env(monkeypatch, first, twin); exp = _expected(part, first, cls)
    for idx in _chunks(pg.n, cls):
        sub = pg.select(idx)
        with A.DecompBatch(0, prm) as b:
            b.add(sub); b.upload(); b.run(); b.download()
            got = b.result(); it = b.iterations()
            _classes_are(b, exp[idx])
        want = common_select_results(o["res"], idx)
        assert np.array_equal(got.status, want.status), (cls, part)
        bad = common.compare_results(want, got, sub.n, conf_tol=1e-9)
        assert not bad, f"class {cls}, {part}: {len(bad)} mismatches, first {bad[:3]}"
        assert np.array_equal(it, o["iters"][idx]), (cls, part, np.nonzero(it != o["iters"][idx])[0][:10])
    idx = np.arange(0, pg.n, CC.TRACE_STRIDE)
    assert len(idx) <= HUGE_BATCH
    with A.DecompBatch(0, prm, trace_events=CC.TRACE_CAP) as b:
        b.add(pg.select(idx)); b.upload(); b.run(); b.download()
        _classes_are(b, exp[idx])
        _traces_equal(b, o["traces"], idx, f"class {cls}, {part}")
    print(f"class {cls:2d} plain, {part}: {pg.n} graphs, 0 mismatches")


@pytest.mark.parametrize("part", ["raw", "raw2"])
@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_raw_kernel_matches_oracle(monkeypatch, first, twin, cls, part):
    """the raw build of class `cls`: pre_assemble_device in the load phase, then the decomposition, against the oracle's pre-steps +
    decomposition under both parameter sets; an item on which the oracle's pre-steps assert ends with a status >= 100"""
    raw = CC.raw_part(); o = CC.oracle_of(part); prm = o["params"]; ok = raw["ok"]; items = raw["items"]
    staged_index = np.cumsum(ok) - 1                      # item -> index among the oracle's staged graphs (where ok)
    _env(monkeypatch, first, twin); exp = _expected(part, first, cls)
    for idx in _chunks(len(items), cls):
        with A.DecompBatch(0, prm) as b:
            for i in idx:
                assert b.add_raw(*items[int(i)][:2], items[int(i)][2]) == 0
            b.upload(); b.run(); b.download()
            got = b.result(); it = b.iterations()
            _classes_are(b, exp[idx])
        okc = ok[idx]
        assert (got.status[~okc] >= 100).all(), (cls, got.status[~okc])
        sidx = staged_index[idx][okc]
        want = common_select_results(o["res"], sidx); mine = common_select_results(got, np.nonzero(okc)[0])
        assert np.array_equal(mine.status, want.status), (cls, part)
        bad = common.compare_results(want, mine, len(sidx), conf_tol=1e-9)
        assert not bad, f"raw class {cls}, {part}: {len(bad)} mismatches, first {bad[:3]}"
        good = want.status == 0
        assert np.array_equal(it[okc][good], o["iters"][sidx][good]), (cls, part)
    keep = np.nonzero(ok)[0][::CC.TRACE_STRIDE]
    with A.DecompBatch(0, prm, trace_events=CC.TRACE_CAP) as b:
        for i in keep:
            assert b.add_raw(*items[int(i)][:2], items[int(i)][2]) == 0
        b.upload(); b.run(); b.download()
        _classes_are(b, exp[keep])
        _traces_equal(b, o["traces"], staged_index[keep], f"raw class {cls}, {part}")
    print(f"class {cls:2d} raw, {part}: {len(items)} graphs, 0 mismatches")


def test_natural_size_of_the_large_classes_with_the_features_on():
    """two graphs each at the natural size of classes 9, 10 and 13 with phasing paths, three samples, strands and touching exons"""
    pg = CC.natural_size_batch()
    want, st, _, _ = common.oracle_run(pg, threads=CC.THREADS)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.result(); it = b.iterations()
        assert [b.class_info(c)["n_graphs"] for c in (9, 10, 13)] == [2, 2, 2]
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert np.array_equal(got.status, want.status) and np.array_equal(it, st[:, 3])


def test_large_raw_graphs_match_oracle():
    """raw graphs of class-10 size through the device pre-steps and the decomposition, against the oracle's"""
    items, staged = CC.large_raw_items()
    want, st, _, _ = common.oracle_run(staged, threads=CC.THREADS)
    with A.DecompBatch(0) as b:
        for pg, phases, dist in items:
            assert b.add_raw(pg, phases, dist) == 0
        b.upload(); b.run(); b.download()
        got = b.result(); it = b.iterations()
        assert b.class_info(10)["n_graphs"] == len(items)
    assert not common.compare_results(want, got, len(items), conf_tol=1e-9)
    assert np.array_equal(got.status, want.status) and np.array_equal(it, st[:, 3])


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
