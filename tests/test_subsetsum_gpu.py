"""GPU tier of the subset-sum pin: aletsch_amd/csrc/subsetsum_kernel.hip against the reference's stored answers over the whole domain of
the kernel (tests/golden/ref_subsetsum_wide.json.gz) and against the oracle, which the CPU tier (tests/test_subsetsum_cpu.py) pins to the
same answers.  Everything compares bit for bit: e with ==, label lists in order, None where the reference or the oracle refuses and for
0 or 33 items on a side.  The instance families, the census and the layout against the grid-stride loop are tests/subsetsum_cases.py.

One thing no answer can show: which of the two list entries of a sum that both sides reach is written first.  Such a pair has distance 0, so
the minimum is 0 and only such pairs compete; they occupy the same two positions in either order, and the two back-traces fill separate
outputs.  A kernel with that order swapped passes this file, as it would pass any comparison of answers."""
import os
import random
import sys

import pytest

import aletsch_amd as A
import common
import subsetsum_cases as K

sys.path.insert(0, os.path.join(common.ROOT, "tests", "golden"))
import make_golden_subsetsum as mk  # noqa: E402

pytestmark = pytest.mark.gpu


def expected(inst):
    """the oracle's answers; None for the out-of-range instances, which never reach the oracle"""
    return [K.oracle_answer(s, t) if K.in_range(s, t) else None for s, t in inst]


def differing(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def dirty_the_lds():
    """a decomposition batch first: its kernels leave their own working state in the LDS the subset-sum tables are laid over"""
    pg = A.synth(**dict(common.PARITY_CONFIGS["cfg1_32v96e"], n_graphs=4096))
    A.decompose(pg, device=0)


def test_wide_fixture_through_the_kernel():
    """every stored instance in one call equals the reference's stored answer"""
    stored = mk.load()
    got = A.subsetsum_batch([(s, t) for _, s, t, _ in stored], 0)
    want = [K.stored_answer(a) for _, _, _, a in stored]
    assert len(got) == len(want) >= 1400
    bad = differing(got, want)
    assert not bad, (len(bad), [(i, stored[i][0], got[i], want[i]) for i in bad[:3]])
    # the fixture fits into one grid: once more behind a copy of itself, so that the first 952 blocks run a second instance over used rows
    twice = A.subsetsum_batch([(s, t) for _, s, t, _ in stored] * 2, 0)
    assert not differing(twice, want * 2)


def test_block_reuse_with_adverse_neighbours():
    """3 * 2048 live instances of all families in one call: block b runs b, b + 2048 and b + 4096, laid out so that a large table is followed
    by a small one and the reverse, a dense list by a sparse one, a refused or out-of-range instance by a valid one and the reverse (each
    order at least MIN_PER_ORDER times, counted from the layout).  All answers equal the oracle's; 64 of them also equal the same
    instance run alone."""
    inst, cs, names = K.reuse_batch()
    assert len(inst) >= 3 * K.GRID
    n = K.order_counts(cs)
    print(n)
    assert min(n.values()) >= K.MIN_PER_ORDER, n
    want = expected(inst)
    assert [w is None for w in want] == [c["out_of_range"] or c["refused"] for c in cs]
    dirty_the_lds()
    got = A.subsetsum_batch(inst, 0)
    bad = differing(got, want)
    assert not bad, (len(bad), [(i, names[i], got[i], want[i]) for i in bad[:3]])
    rng = random.Random(5)
    for i in rng.sample(range(K.GRID, len(inst)), 64):               # second and third instances of their blocks
        assert A.subsetsum_batch([inst[i]], 0) == [got[i]], (i, names[i])


def test_batch_shape_invariance():
    """the same 500 instances as one batch, as batches of one and reversed give the same answer per instance"""
    inst, _, _ = K.reuse_batch()
    sub = [inst[i] for i in random.Random(6).sample(range(len(inst)), 500)]
    whole = A.subsetsum_batch(sub, 0)
    assert whole == expected(sub)
    assert [A.subsetsum_batch([x], 0)[0] for x in sub] == whole
    assert A.subsetsum_batch(sub[::-1], 0)[::-1] == whole


def test_out_of_range_neighbours_and_empty_batch():
    """0 or 33 items on a side return None, and the instances before and after them in the arrays are untouched by it: the offsets of
    ald_subsetsum_batch count a side of 33 items and skip a side of none.  An empty batch is legal."""
    rng = random.Random(7)
    valid = [x for x in K.random_instances(rng, 400) + K.sizes(rng, 98)]
    oor = K.out_of_range(rng, 120)
    inst = []
    for k, x in enumerate(valid):
        inst.append(x)
        if k % 4 == 0:
            inst.append(oor[(k // 4) % len(oor)])
        if k % 40 == 0:
            inst.append(oor[(k // 4 + 1) % len(oor)])              # two in a row
    inst = [oor[0]] + inst + [oor[1]]                              # first and last of the arrays
    want = expected(inst)
    got = A.subsetsum_batch(inst, 0)
    assert sum(not K.in_range(s, t) for s, t in inst) >= 100
    assert all(got[i] is None for i, (s, t) in enumerate(inst) if not K.in_range(s, t))
    assert got == want
    assert A.subsetsum_batch([oor[0]], 0) == [None] and A.subsetsum_batch(oor, 0) == [None] * len(oor)
    assert A.subsetsum_batch([], 0) == []


def test_census_conditions_hold_on_the_live_batch():
    """the live batch fills every bucket the fixture fills (the CPU tier asserts the same of the fixture)"""
    _, cs, _ = K.reuse_batch()
    b = K.buckets(cs)
    print(b)
    short = {k: v for k, v in b.items() if v < K.MIN_PER_BUCKET}
    assert not short, short
