"""CPU tier of the subset-sum pin: reference object code -> tests/golden/ref_subsetsum_wide.json.gz -> oracle/subsetsum_oracle.hpp.
The fixture (tests/golden/make_golden_subsetsum.py) holds 1500 instances of the families of tests/subsetsum_cases.py -- 1..32 items a side,
bumped items up to the largest table bound, scale-up, dense lists, ties far apart, sort order, refused instances -- with the answers of the
reference's own scallop/subsetsum.cc.  The GPU tier (tests/test_subsetsum_gpu.py) takes the kernel from there."""
import os
import sys

import common
import subsetsum_cases as K

sys.path.insert(0, os.path.join(common.ROOT, "tests", "golden"))
import make_golden_subsetsum as mk  # noqa: E402


def test_oracle_matches_the_wide_reference_fixture():
    """the oracle equals every stored answer of the reference: e with ==, label lists in order, refused -> None"""
    stored = mk.load()
    assert len(stored) >= 1400
    bad = [i for i, (_, s, t, a) in enumerate(stored) if K.oracle_answer(s, t) != K.stored_answer(a)]
    assert not bad, (len(bad), bad[:5], [stored[i][0] for i in bad[:5]])


def test_wide_fixture_is_what_the_generator_draws():
    """the stored instances are fixture_selection() of today's families: a drifting generator fails here, not silently in the census"""
    assert [(f, s, t) for f, s, t, _ in mk.load()] == K.fixture_selection()


def test_wide_fixture_matches_live_reference_build():
    """where build() could make oracle/_ref/ref_subsetsum, the reference asked again gives the stored answers (a live pin); elsewhere the
    stored answers stand in"""
    exe = os.path.join(common.ROOT, "oracle", "_ref", "ref_subsetsum")
    stored = mk.load()
    if os.path.exists(exe):
        bad = [i for i, (_, s, t, a) in enumerate(stored) if mk.reference_answer(exe, s, t) != a]
        assert not bad, (len(bad), bad[:5])
    assert len(stored) == sum(K.FIXTURE_COUNTS.values())


def test_census_conditions_hold_on_the_fixture():
    """every bucket of the census holds at least MIN_PER_BUCKET stored instances; refused ones are at most a tenth; what the census calls
    refused is what the reference aborted on"""
    stored = mk.load()
    cs = K.census([(s, t) for _, s, t, _ in stored])
    b = K.buckets(cs)
    print(b)
    short = {k: v for k, v in b.items() if v < K.MIN_PER_BUCKET}
    assert not short, short
    assert b["refused"] * 10 <= len(stored)
    assert [c["refused"] for c in cs] == [a is None for _, _, _, a in stored]
    assert max(max(c["ub1"], c["ub2"]) for c in cs) == 1029 and max(max(c["bumps1"], c["bumps2"]) for c in cs) == 31      # the largest the domain allows
    assert not any(c["out_of_range"] for c in cs)


def test_instances_stay_inside_the_reference_domain():
    for counts, seed in ((K.FIXTURE_COUNTS, K.FIXTURE_SEED), (K.LIVE_COUNTS, 20261018)):
        for f, s, t in K.draw(counts, seed):
            for side in (s, t):
                assert all(1 <= v <= K.MAX_VALUE for v, _ in side) and sum(v for v, _ in side) < 2 ** 31, f
                assert all(-2 ** 31 <= l < 2 ** 31 for _, l in side), f
            assert K.in_range(s, t) == (f != "out_of_range"), f


def test_census_notices_a_missing_family():
    """the selection without the bump family leaves the bucket of 9..31 bumped items empty, without the tie family the instances whose
    equal minima lie at a distance d > 0 and 64 entries apart are gone, and an empty selection fills nothing"""
    w = K.buckets(K.census([(s, t) for _, s, t in K.fixture_selection(without=("bumps",))]))
    assert w["bumped 9..31"] < K.MIN_PER_BUCKET, w
    far = lambda cs: sum(1 for c in cs if c["minima"] > 8 and c["spread"] >= 64 and c["d"] == 1)      # noqa: E731
    every = K.census([(s, t) for _, s, t in K.fixture_selection()])
    no_ties = K.census([(s, t) for _, s, t in K.fixture_selection(without=("ties",))])
    assert far(every) >= K.MIN_PER_BUCKET > far(no_ties), (far(every), far(no_ties))
    assert not any(K.buckets([]).values())


def test_reuse_batch_layout():
    """the batch of the GPU tier's block-reuse test: 3 * 2048 instances, every adverse order at least MIN_PER_ORDER times between the
    instances one block runs in turn, every census bucket filled"""
    inst, cs, names = K.reuse_batch()
    assert len(inst) == 3 * K.GRID and set(names) == set(K.FAMILIES)
    n = K.order_counts(cs)
    assert min(n.values()) >= K.MIN_PER_ORDER, n
    short = {k: v for k, v in K.buckets(cs).items() if v < K.MIN_PER_BUCKET}
    assert not short, short
