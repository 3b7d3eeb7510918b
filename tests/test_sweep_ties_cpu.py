"""CPU tier of the sweeps' ties, thresholds and lane order: the cases of tests/sweep_cases.py through the single-lane emulation against the
oracle, and the census of what they put in front of the selections.

The emulation does not run wave_argmin (an empty stub where ALD_WAVE == 1) nor the interplay of the lanes -- `lim`, a stop lane in front of a
now lane, the per-lane fold over the chunks, the dense-lane refresh of the kept records -- so this tier pins what ONE lane can pin: the
comparisons against the thresholds, the ties inside a vertex, which parameter a pass reads; and it keeps the cases honest where there is no
GPU (a case whose oracle trace the emulation does not reproduce is a wrong case or a wrong engine, found here).  The lane order itself is
pinned by tests/test_sweep_ties_gpu.py on the same cases."""
import numpy as np
import pytest

import common
import device_run as DR
import sweep_cases as SC

# the emulation legs: (force_class, kept-records build)
LEGS = {"natural": (0, False), "class2": (2, False), "class9": (9, False), "class10": (10, False), "class13": (13, False), "keep": (0, True)}


def test_census_of_the_cases():
    """every bullet of the families (a)-(i), every varied parameter and every trace-derived kind: at least 10 events, counted by the oracle;
    (a): at least 120 distinct (chunk, lane) winner positions, the lanes on both sides of every DPP row and of the chunk edge among them"""
    print("\ncensus of the sweep cases (events per line, from the oracle):\n" + SC.census_table())
    assert not SC.census_short(), SC.census_short()


def test_unread_parameters_change_nothing_in_the_oracle():
    """max_decompose_error_ratio[1], [2], [3] and [6] are read by nothing: the oracle's results under a set that moves only them are the default's"""
    R = SC.runs(); a, b = R["param/default"], R["param/unread"]
    assert not common.compare_results(a["res"], b["res"], a["pg"].n)
    assert np.array_equal(a["iters"], b["iters"]) and a["traces"] == b["traces"]


def test_the_invariant_statuses_are_there():
    """min_guaranteed_edge_weight = 2.0 ends some graphs of the random batch on an invariant status in the oracle, and not all of them"""
    st = SC.runs()["param/minw20"]["res"].status
    assert (st >= 100).sum() >= SC.MIN_EVENTS and (st == 0).sum() >= SC.MIN_EVENTS, np.unique(st, return_counts=True)


@pytest.mark.parametrize("leg", list(LEGS))
def test_emulation_matches_oracle(leg):
    """records bit for bit, statuses, and -- for every graph that does not end on an invariant status -- the iteration count and the whole op
    trace, on every run of sweep_cases.runs()"""
    force, keep = LEGS[leg]; n = 0
    for name, o in SC.runs().items():
        pg = o["pg"]
        got, it, cl, traces = SC.emu_full(pg, o["params"], force, keep)
        assert np.array_equal(cl, SC.expected_classes(name, force)), (leg, name, np.unique(cl))
        assert np.array_equal(got.status, o["res"].status), (leg, name)
        bad = common.compare_results(o["res"], got, pg.n)
        assert not bad, (leg, name, bad[:3])
        good = o["res"].status < 100                        # (a graph that ends on an invariant status has no iteration count in the oracle)
        assert np.array_equal(it[good], o["iters"][good]), (leg, name, np.nonzero(it != o["iters"])[0][:10])
        for g in np.nonzero(good)[0]:
            a, b = traces[g], o["traces"][g]
            assert a == b, f"{leg}, {name}, graph {g} ({o['labels'][g] if o['labels'] else ''}): first divergence at {DR.first_divergence(a, b)}"
        n += pg.n
    print(f"{leg}: {n} graphs, 0 mismatches")
