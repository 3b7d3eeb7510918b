"""CPU tier of the size-class matrix: every class of the engine, plain and raw, against the oracle on ONE mix of small graphs.

The engine is compiled once per size class and the source differs by class: 32-bit creation ids in class 13, sweep records kept in the slab
in classes 10..13, the merged in / out list walks of eval_smallest and compute_balance_ratio in classes 10..13 (ALD_MERGED_WALKS: compiled
by the emulation of classes 10 and 13 as well), ALD_STARFIX_MAX 2 or 4, the register form of sweep_smallest wherever NC <= 16.  The
suite's big batches only ever reach the class a graph's size asks for; here pick_class() is given a FIRST class (force_class), so the mix of
tests/class_cases.py -- 6..60 vertices, every feature on -- runs in each of them.  What the mix exercised is counted in the oracle alone
(class_cases.census) and asserted at 10 events a line.  tests/test_class_matrix_gpu.py repeats the matrix on the device kernels."""
import numpy as np
import pytest

import class_cases as CC
import common
import device_run as DR
import shapes


def test_census_of_the_mix():
    """every op code 1..10, router builds with and without phasing lists / with one and with several samples, fans of 2, 3, 4 and 5-8 in
    both directions, raw graphs with a folded boundary and with a dropped phase: at least 10 events each, counted by the oracle"""
    cen = CC.census()
    print("\ncensus of the class mix (events per line, from the oracle):\n" + CC.census_table())
    short = {k: v for k, v in cen.items() if v < CC.MIN_EVENTS}
    assert not short, short
    raw = CC.raw_part()
    assert (~raw["ok"]).sum() * 5 <= len(raw["ok"]), "more than a fifth of the raw part ends on an assert of the pre-steps"
    assert raw["n_hubs"] == 12


def test_forced_hubs_fill_the_group_of_classes_10_and_13():
    """shapes.class_group's fourth group (classes 10 / 13: ALD_STARFIX_MAX = 2 like classes 0 / 1, everything else unlike them) is filled
    by the hubs of this mix, which the matrix runs in those classes -- not by a larger hub batch"""
    K = shapes.kernel_constants()
    assert shapes.class_group(10, 40, K) == shapes.class_group(13, 40, K) == "10,13"
    assert K["STARFIX_MAX"][10] == K["STARFIX_MAX"][13] == K["STARFIX_MAX"][0]
    req = CC.forced_hub_census(K).required_of_group("10,13")
    print("\nfans of the mix as classes 10 / 13 see them:\n" + "\n".join("%-40s %6d" % kv for kv in req.items()))
    assert len(req) == 8
    short = {k: v for k, v in req.items() if v < CC.MIN_EVENTS}
    assert not short, short


def _check_traces(o, mine, idx, what):
    for k, g in enumerate(idx):
        a, b = mine[k], o["traces"][int(g)]
        assert a == b, f"{what}, graph {int(g)}: first divergence at {DR.first_divergence(a, b)}"


@pytest.mark.parametrize("part", ["staged", "second"])
@pytest.mark.parametrize("cls", CC.CLASSES)
def test_plain_class_matches_oracle(cls, part):
    """the staged part under the default parameters, the second sub-batch under its own: every graph runs in class `cls` (in
    class 1 under a first class of 0 when it has more than 32 vertices: class_cases.expected_classes); records bit for
    bit, iteration counts, the op trace on every fourth graph"""
    o = CC.oracle_of(part); pg = o["pg"]
    got, it, cl = common.emu_run(pg, force_class=cls, params=o["params"])
    assert np.array_equal(cl, CC.expected_classes(part, cls)), (cls, np.unique(cl))
    bad = common.compare_results(o["res"], got, pg.n)
    assert not bad, (cls, part, bad[:3])
    assert np.array_equal(it, o["iters"]), (cls, part)
    idx = np.arange(0, pg.n, CC.TRACE_STRIDE)
    _check_traces(o, common.emu_traces(pg.select(idx), CC.TRACE_CAP, cls, o["params"]), idx, f"class {cls}, {part}")


@pytest.mark.parametrize("part", ["staged", "second"])
@pytest.mark.parametrize("cls", range(2, 10))
def test_kept_records_build_of_the_lds_classes_matches_oracle(cls, part):
    """the emulation with the sweep records kept in EVERY class (and its stale-record checker): classes 7 / 8 of it are the source of the
    twins 11 / 12 minus the slab walks"""
    o = CC.oracle_of(part); pg = o["pg"]
    got, it, cl = common.emu_run(pg, force_class=cls, params=o["params"], keep=True)
    assert np.array_equal(cl, CC.expected_classes(part, cls)), (cls, np.unique(cl))
    bad = common.compare_results(o["res"], got, pg.n)
    assert not bad, (cls, part, bad[:3])
    assert np.array_equal(it, o["iters"]), (cls, part)
    idx = np.arange(0, pg.n, CC.TRACE_STRIDE)
    _check_traces(o, common.emu_traces(pg.select(idx), CC.TRACE_CAP, cls, o["params"], keep=True), idx, f"kept records, class {cls}, {part}")


@pytest.mark.parametrize("part", ["raw", "raw2"])
@pytest.mark.parametrize("cls", CC.CLASSES)
def test_raw_class_matches_oracle(cls, part):
    """the raw part through the load phase (pre_assemble_device) of class `cls`, under both parameter sets, against the oracle's pre-steps +
    decomposition; an item on which the oracle's pre-steps assert ends with a status >= 100"""
    raw = CC.raw_part(); o = CC.oracle_of(part); ok = raw["ok"]
    got, it, cl, traces = common.emu_run_raw(raw["items"], params=o["params"], force_class=cls, trace_cap=CC.TRACE_CAP, full=True)
    assert np.array_equal(cl, CC.expected_classes(part, cls)), (cls, np.unique(cl))
    assert (got.status[~ok] >= 100).all(), (cls, got.status[~ok])
    keep = np.nonzero(ok)[0]
    bad = common.compare_results(o["res"], common.select_results(got, keep), len(keep))
    assert not bad, (cls, part, bad[:3])
    good = o["res"].status == 0
    assert np.array_equal(it[keep][good], o["iters"][good]), (cls, part)
    idx = np.arange(0, len(keep), CC.TRACE_STRIDE)
    _check_traces(o, [traces[int(keep[k])] for k in idx], idx, f"raw class {cls}, {part}")


def test_natural_size_of_the_large_classes_with_the_features_on():
    """two graphs each at the natural size of classes 9, 10 and 13 with phasing paths, three samples, strands and touching exons (the
    suite's other graphs of these classes are bare): more than 16 chunks a sweep and long lists"""
    pg = CC.natural_size_batch()
    want, st, _, _ = common.oracle_run(pg, threads=CC.THREADS)
    got, it, cl = common.emu_run(pg)
    assert tuple(cl) == CC.NATURAL_CLASSES, cl
    assert not common.compare_results(want, got, pg.n)
    assert np.array_equal(it, st[:, 3])


def test_large_raw_graphs_match_oracle():
    """raw graphs of class-10 size: pre-steps + decomposition against the oracle's (the feature tests compare their feature table only)"""
    items, staged = CC.large_raw_items()
    want, st, _, _ = common.oracle_run(staged, threads=CC.THREADS)
    got, it, cl, _ = common.emu_run_raw(items, full=True)
    assert (cl == 10).all(), cl
    assert not common.compare_results(want, got, len(items))
    good = want.status == 0
    assert good.all() and np.array_equal(it, st[:, 3])


def test_creation_ids_on_both_sides_of_16_bits():
    """Class 13 keeps its creation ids in 32 bits; every other graph of the suite ends below 65 536 ids.  Two graphs of class-13 size, one
    whose ids end above 65 535 and one just below (the oracle's total_edge_ids), emulation against oracle.  The oracle needs about half a
    minute for each (they run side by side): the one long test of this file."""
    pg = CC.id_width_batch()
    want, st, _, _ = common.oracle_run(pg, threads=2)
    print("\ntotal_edge_ids of the id-width pair:", st[:, 2].tolist())
    assert st[0, 2] > 65535 and st[1, 2] < 65535, st[:, 2]
    got, it, cl = common.emu_run(pg)
    assert (cl == 13).all(), cl
    assert not common.compare_results(want, got, pg.n)
    assert np.array_equal(it, st[:, 3])
