"""CPU tier of the assert exits (tests/assert_cases.py): every graph of it ends on one of the reference's asserts, and which one is counted --
per site of the ORACLE (a name: scope + function + tag, with the vertex of the rule in flight and its degrees), per fan bucket and direction
for the sites of the trivial decomposition, per router form for the router's, and per fail() LINE of decomp_device.h as the emulation reports
it.  A line of the kernel is either reached by MIN_EVENTS graphs or listed in assert_cases.UNREACHED with its reason; a listed line that IS
reached fails the test as well.

Compared, in the list build, the row build and the kept-records build of the emulation: status word, no path from a failed graph, the op trace
(which ends where the oracle's ends: tolerance 0), the records of every graph that ends well.  The emulated wave runs a class's work list in
order, so the graph behind a failed one is chosen: every (exit group, witness kind) pair occurs MIN_EVENTS times as `failed graph directly
followed by witness in the same class`, the witness's records are the oracle's, and the same batch reversed gives every graph the same result."""
import ctypes as C
import os

import numpy as np
import pytest

import aletsch_amd as A
import assert_cases as AC
import common
import device_run as DR
import shapes

MIN_EVENTS = AC.MIN_EVENTS
K = AC.K
BUILDS = {"lists": dict(), "rows": dict(rows=True), "keep": dict(keep=True)}


def test_site_names_are_names():
    """scope + function + tag, never a line number; the same condition twice in one function has tags of its own (balance_vertex)"""
    c = AC.census()
    for site in c.sites:
        assert ": " in site and not any(ch.isdigit() for ch in site.split(": ")[0]), site
    assert {"Scallop::balance_vertex: in-edge weight", "Scallop::balance_vertex: out-edge weight"} <= set(c.sites)


@pytest.mark.parametrize("build", list(BUILDS))
def test_emulation_matches_oracle_on_every_failing_graph(build):
    """status, zero paths, the whole op trace -- it must end where the oracle's ends --, per parameter set"""
    n = 0
    for ps, (labels, pg, graphs, prm) in AC.site_batches().items():
        want, traces, sites = AC.oracle_of(ps)
        got, it, cl, mine, ln = common.emu_run_full(pg, params=prm, **BUILDS[build])
        ended_well = {labels[g] for g in np.nonzero(want.status < 100)[0]}
        assert ended_well <= {"star remainder"}, (ps, ended_well)               # (a `remainder` star whose rounding stays within SMIN ends with status 0: compared all the same)
        bad = common.compare_results(want, got, pg.n)
        assert not bad, (ps, build, bad[:3])
        failed = np.nonzero(want.status != 0)[0]
        assert (np.diff(got.path_offset)[failed] == 0).all(), (ps, build)
        assert ((ln != 0) == (got.status != 0)).all(), (ps, build)              # every status has the line that raised it, and only those
        for g in range(pg.n):
            assert mine[g] == traces[g], f"{ps}, {build}, graph {g} ({labels[g]}): first divergence at {DR.first_divergence(mine[g], traces[g])} of {len(traces[g])}"
        n += pg.n
    print(f"\n{build}: {n} graphs that end on an assert, 0 mismatches")


def test_raw_graphs_whose_pre_steps_assert():
    """the two asserts of the pre-steps (boundaries that do not ascend, a phase listed backwards): the raw build of the emulation ends with the
    oracle's status class"""
    rc, sites, status, ln = AC.raw_results()
    assert all(r >= 100 for r in rc) and [int(s) for s in status] == rc, (rc, status.tolist())


def test_census_of_the_assert_exits():
    """>= MIN_EVENTS graphs per oracle site; per site of the trivial decomposition again per fan bucket and direction, per router site per form;
    per fail() line of decomp_device.h that the emulation compiles -- reached, or listed in UNREACHED with its reason, never both"""
    c = AC.census()
    print("\ncensus of the assert exits (graphs per line, sites and degrees from the oracle, lines from the emulation):\n" + c.table())
    short = {k: v for k, v in c.required().items() if v < MIN_EVENTS}
    assert not short, short
    lines = AC.kernel_fail_lines()
    listed = AC.unreached_lines()
    neither = [ln for ln in lines if c.lines.get(ln, 0) < MIN_EVENTS and ln not in listed]
    assert not neither, {ln: (lines[ln], c.lines.get(ln, 0)) for ln in neither}
    stale = [ln for ln in listed if c.lines.get(ln, 0) > 0]
    assert not stale, stale
    assert set(c.lines) - {0} <= set(lines), sorted(set(c.lines) - {0} - set(lines))          # the parser found every line the emulation reports
    assert set(listed) <= set(lines)


def test_conditions_on_the_unreached_list():
    """the eight sites a crude random probe reaches are not on it; no weight or count exit of a star form is; ALD_INV_MERGE_EQUAL only with its
    argument written down; every entry has a sentence"""
    lines = AC.kernel_fail_lines(); src = open(os.path.join(shapes.CSRC, "decomp_device.h")).read().split("\n")
    lo, hi = AC.star_form_lines(src)
    for key, reason in AC.UNREACHED.items():
        assert reason.startswith("cannot happen") and len(reason.split()) >= 12, key      # an argument, stated as one
        assert "not covered" not in reason and "no generator" not in reason, key           # "nobody built it" is no reason: build the generator
    for ln in AC.unreached_lines():
        what = lines[ln]
        if lo <= ln <= hi: assert "ALD_INV_WEIGHT" not in what and "ALD_INV_COUNT" not in what, (ln, what)
        if "ALD_INV_MERGE_EQUAL" in what:
            # only the general merge of the greedy phase may be listed, with the argument of its two premises: the cut weight is finite, the pieces lie within SMIN
            why = AC.unreached_lines()[ln]
            assert not (lo <= ln <= hi) and "greedy" in why and "DBL_MAX" in why and "SMIN" in why, (ln, why)
    assert c_sites().get(AC.MERGE_EQUAL_SITE, 0) >= MIN_EVENTS                             # where the pair weight CAN be infinite -- the stars -- the exit is reached
    c = AC.census()
    for site in AC.PROBE_SITES:
        assert c.sites.get(site, 0) >= MIN_EVENTS, site
    for ln in c.site_lines_of(AC.PROBE_SITES): assert ln not in AC.unreached_lines(), ln


def test_census_notices_a_missing_generator():
    """without the stars whose centre is used up early, the line of that exit in the sequential star is neither reached nor listed"""
    c = AC.census(without=("star consumed",))
    lines = AC.kernel_fail_lines(); listed = AC.unreached_lines()
    neither = [ln for ln in lines if c.lines.get(ln, 0) < MIN_EVENTS and ln not in listed]
    assert neither, "the census did not notice"
    full = AC.census()
    assert all(full.lines.get(ln, 0) >= MIN_EVENTS for ln in neither)          # (the site itself stays filled by the stars that keep a remainder: it is the LINE census that notices)


def test_witnesses_need_what_they_claim():
    """(a) grows past its own V, (b) holds more live edges than it was staged with, (c) phasing lists, (d) several samples on an edge,
    (e) at most 6 vertices, (f) two router builds or more in a sweep that ends on `best`: from the oracle's statistics and trace"""
    w = AC.witnesses(); pg = AC.pack([g for _, g in w]); prm = AC.params(**AC.PARAM_SETS["wide"])
    want, st, _, tr = common.oracle_run(pg, threads=DR.THREADS, trace=True, params=prm)
    assert (want.status == 0).all()
    for j, (kind, g) in enumerate(w):
        V, E = g["V"], len(g["edges"])
        if kind == "a": assert st[j, 1] > V, (j, st[j])
        if kind == "b": assert st[j, 0] > E and st[j, 2] > 2 * E, (j, st[j])
        if kind == "c": assert pg.g_np[j] >= 2
        if kind == "d": assert max(len(e[4]) for e in g["edges"]) >= 2
        if kind == "e": assert V <= 6
        if kind == "f": assert st[j, 4] >= 2 and any(ev[0] == 8 for ev in tr[j]), (j, st[j])


@pytest.mark.parametrize("build", list(BUILDS))
def test_the_graph_behind_a_failed_one(build):
    """the interleaved batch (failed graph, witness, failed graph, witness ...) in one class, in its order and reversed: every graph the oracle's
    status, trace and records both times"""
    o = AC.successor_batch(); pg = o["pg"]; prm = o["params"]
    want, traces = o["want"], o["traces"]
    fwd = common.emu_run_full(pg, params=prm, force_class=AC.SUCCESSOR_CLASS, **BUILDS[build])
    pairs = AC.successor_pairs(o, fwd[2])
    print("\n(exit group, witness kind): failed graph directly followed by the witness in the same class\n" + "\n".join("%-22s %s  %4d" % (k + (v,)) for k, v in sorted(pairs.items())))
    short = {k: v for k, v in pairs.items() if v < MIN_EVENTS}
    assert not short and len(pairs) == len(AC.SUCCESSOR_GROUPS) * len(AC.WITNESS_KINDS), short
    rev = np.arange(pg.n)[::-1]
    back = common.emu_run_full(pg.select(rev), params=prm, force_class=AC.SUCCESSOR_CLASS, **BUILDS[build])
    for name, (got, it, cl, mine, ln), order in (("given", fwd, np.arange(pg.n)), ("reversed", back, rev)):
        sel = common_select(want, order)
        bad = common.compare_results(sel, got, pg.n)
        assert not bad, (build, name, bad[:3])
        for k, g in enumerate(order):
            assert mine[k] == traces[int(g)], (build, name, int(g), o["labels"][int(g)])
        assert (np.diff(got.path_offset)[sel.status != 0] == 0).all()


def common_select(res, idx):
    return common.select_results(res, idx)


def c_sites():
    return AC.census().sites


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("which", ["grown", "climb"])
def test_the_graph_behind_one_that_grew_or_climbed(which, build, monkeypatch):
    """two more exit groups, a batch each: hubs that grow past max_num_exons mid-run (ALD_ST_SKIPPED_LARGE, asserted from the oracle's vertex
    statistics), and hubs started one class too low (ALD_DEBUG_UNDERCLASS=1) that meet ALD_ST_CAPACITY where the decomposition behind the router
    asks for 400 edge slots and really climb (asserted from the emulation's classes: the hubs end one class above the witnesses).  Every witness
    kind 10 times directly behind one, in the same work list; records and traces the oracle's, in the given order and reversed"""
    o = AC.extra_successor_batch(which); pg = o["pg"]; prm = o["params"]; want = o["want"]; kinds = o["kinds"]
    hubs = np.array([k == o["group"] for k in kinds])
    if which == "grown":
        assert (want.status[hubs] == 1).all()                                      # ALD_ST_SKIPPED_LARGE (include/aletsch_decomp.h)
        assert (pg.g_nv[hubs] <= AC.GROWN_MAX_EXONS).all() and (o["stats"][hubs, 1] > AC.GROWN_MAX_EXONS).all()      # not refused at the start: grown past the limit
    else:
        monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
        assert (want.status == 0).all()
    rev = np.arange(pg.n)[::-1]
    for name, order in (("given", np.arange(pg.n)), ("reversed", rev)):
        got, it, cl, mine, ln = common.emu_run_full(pg.select(order) if name == "reversed" else pg, params=prm, force_class=AC.SUCCESSOR_CLASS, cap=1 << 10, **BUILDS[build])
        sel = common.select_results(want, order)
        assert not common.compare_results(sel, got, pg.n), (which, build, name)
        assert all(mine[k] == o["traces"][int(g)] for k, g in enumerate(order)), (which, build, name)
        if name == "given":
            start = int(cl[~hubs].min())
            if which == "climb":
                assert (cl[~hubs] == start).all() and (cl[hubs] == start + 1).all(), np.unique(cl)      # every graph began in one work list; the hubs had to climb
            else:
                assert (cl == start).all(), np.unique(cl)
            pairs = {}
            for x in range(pg.n - 1):
                if hubs[x] and not hubs[x + 1] and want.status[x + 1] == 0: pairs[kinds[x + 1]] = pairs.get(kinds[x + 1], 0) + 1
            print("\n%s: witness kind directly behind  %s" % (o["group"], sorted(pairs.items())))
            assert set(pairs) == set(AC.WITNESS_KINDS) and min(pairs.values()) >= MIN_EVENTS, pairs
