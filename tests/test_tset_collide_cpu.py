"""Transcripts that share hash buckets, CPU tier: the cases of tests/collide_cases.py against the answers of the reference's own
transcript_set.cc stored in tests/golden/ref_tset_collide.json.gz (tests/golden/make_golden_tset_collide.py).  Checked here: the census
(every situation of collide_cases.census at least CENSUS_MIN times, in both cases), the host sink against the reference fed in one call and
group by group, with and without the single-exon filter, ald_tset_merge of sinks built from segments of the groups against
transcript_set::add(transcript_set&) of the reference's sets, the stored hash of every item against the hash written out in numpy, and,
where oracle/_ref/ref_tset exists, the reference asked again.  Every comparison is bit for bit."""
import functools
import os
import sys

import pytest

import aletsch_amd as A
import collide_cases as cc
from test_dev_tset_cpu import as_groups, check
from test_owner_split_cpu import bucket_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_tset_collide as mkc  # noqa: E402

N_CASES = len(cc.CASES)


@functools.lru_cache(maxsize=None)
def golden():
    """[(groups in as_groups form, {seq, merge2, merge3, seq_multi: the reference's items})]"""
    return [(as_groups(g), want) for g, want in mkc.load()]


def sink_of(groups, skip=False, one_by_one=False):
    s = A.TranscriptSink(0.8)
    if one_by_one:
        for g in groups:
            s.add_groups([g], skip_single_exon=skip)
    else:
        s.add_groups(groups, skip_single_exon=skip)
    return s


def cut(groups, parts):
    out = []; a = 0
    for k in cc.segments(len(groups), parts):
        out.append(groups[a:a + k]); a += k
    assert a == len(groups)
    return out


@pytest.mark.parametrize("i", range(N_CASES))
def test_census(i):
    groups, want = golden()[i]
    assert len(groups) == cc.CASES[i][0]
    c = cc.census(groups, want["seq"])
    print(c)
    assert len(c) == 18
    for line, n in c.items():
        assert n >= cc.CENSUS_MIN, (line, n)
    # every chain of every cluster was drawn under all three strands
    seen = {(t[0], tuple(t[6][0]) if len(t[6]) == 1 else tuple(cc.flat(t[6])[1:-1])) for _, ts in groups for t in ts}
    for cl in cc.case(i)[1]:
        for ch in cl["chains"]:
            if len(ch) > 1:
                assert all((st, tuple(cc.flat(ch)[1:-1])) in seen for st in cc.STRANDS), (cl["kind"], ch)
    kinds = [cl["kind"] for cl in cc.case(i)[1]]
    assert {k: kinds.count(k) for k in set(kinds)} == {"visible": len(cc.VISIBLE_NE) * cc.CASES[i][1], "hidden": len(cc.HIDDEN_NE) * cc.CASES[i][2],
                                                        "mixed": cc.CASES[i][3], "cross": cc.CASES[i][4], "host/device": cc.CASES[i][5]}
    assert any(len(ch) == 9 for cl in cc.case(i)[1] if cl["kind"] == "visible" for ch in cl["chains"])


@pytest.mark.parametrize("i", range(N_CASES))
def test_host_sink_equals_the_reference(i):
    groups, want = golden()[i]
    for one_by_one in (False, True):
        check(sink_of(groups, False, one_by_one).items(), want["seq"])
        check(sink_of(groups, True, one_by_one).items(), want["seq_multi"])
    assert all(len(x["exons"]) > 1 for x in want["seq_multi"]) and any(len(x["exons"]) == 1 for x in want["seq"])


@pytest.mark.parametrize("parts", mkc.PARTS)
@pytest.mark.parametrize("i", range(N_CASES))
def test_merge_of_segment_sinks_equals_the_reference_merge(i, parts):
    """ald_tset_merge against transcript_set::add(transcript_set&) on sets that both hold items: the sets of the segments folded left to right"""
    groups, want = golden()[i]
    sinks = [sink_of(seg) for seg in cut(groups, parts)]
    assert all(len(s.items()) > 100 for s in sinks)
    for s in sinks[1:]:
        sinks[0].merge(s)
        assert s.items() == []
    check(sinks[0].items(), want["merge%d" % parts])
    # the merged sets hold the chains of the sequential answer in its order (sums may differ in their last bits: another nesting)
    assert [(x["hash"], x["count"], x["tid"], x["exons"]) for x in want["merge%d" % parts]] == [(x["hash"], x["count"], x["tid"], x["exons"]) for x in want["seq"]]


def test_stored_hashes_equal_the_hash_written_out():
    n = 0
    for _, want in golden():
        for items in want.values():
            for x in items:
                w = [v for e in x["exons"] for v in e]
                assert x["hash"] == bucket_of(w) == cc.bucket_of(x["exons"]), x
                n += 1
    assert n > 3000
    for i in range(N_CASES):                                          # the generator's own bookkeeping: a cluster is one bucket
        for cl in cc.case(i)[1]:
            assert all(bucket_of(cc.flat(ch)) == cl["bucket"] for ch in cl["chains"])


def test_fixture_matches_live_reference_build():
    """where build() could make oracle/_ref/ref_tset, the reference asked again repeats the stored file; elsewhere the stored answers stand in.
    A ref_tset that was built from the driver as it was before it took `merge` (it ignores the arguments: mkc.knows_merge) is asked for the
    sequential answers only, which that driver replays in the same way"""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_tset")
    d = mkc.stored()
    if os.path.exists(exe):
        merges = mkc.knows_merge(exe)
        live = mkc.reference_outputs(exe, merges)
        for got, want in zip(live, d["out"]):
            for k in got:
                assert got[k] == want[k], (k, "merge is known" if merges else "a driver without merge")
        assert len(live) == len(d["out"]) and all(len(got) == (4 if merges else 2) for got in live)
    assert len(d["out"]) == N_CASES and all(sorted(o) == sorted(mkc.KEYS) for o in d["out"])


def test_a_restatement_wrong_by_one_word_would_show():
    """the words compare1 skips are exactly those of the exon before the last: filing the transcripts under a key that skips one word less
    (either of the two) or one word more (the word after them, nw-2, or the word before them, nw-5) gives another number of multi-exon items than the reference has"""
    for groups, want in golden():
        multi = [t for _, ts in groups for t in ts if len(t[6]) > 1]
        n_ref = sum(len(x["exons"]) > 1 for x in want["seq"])
        assert len({cc.chain_key(t[0], t[6]) for t in multi}) == n_ref
        wrong = {"word nw-4 compared": lambda t: (cc.chain_key(t[0], t[6]), t[6][-2][0] if len(t[6]) >= 3 else 0),
                 "word nw-3 compared": lambda t: (cc.chain_key(t[0], t[6]), t[6][-2][1] if len(t[6]) >= 3 else 0),
                 "word nw-2 skipped": lambda t: cc.chain_key(t[0], t[6])[:3] + (cc.chain_key(t[0], t[6])[3][:-1] if len(t[6]) >= 3 else cc.chain_key(t[0], t[6])[3],)}
        wrong["word nw-5 skipped"] = lambda t: cc.chain_key(t[0], t[6])[:3] + (cc.chain_key(t[0], t[6])[3][:-2] + cc.chain_key(t[0], t[6])[3][-1:] if len(t[6]) >= 4 else cc.chain_key(t[0], t[6])[3],)
        for name, key in wrong.items():
            n = len({key(t) for t in multi})
            assert abs(n - n_ref) >= cc.CENSUS_MIN, (name, n, n_ref)
