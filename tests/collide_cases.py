"""Transcript groups whose chains SHARE hash buckets, and the census of what they exercise.

transcript::get_intron_chain_hashing is a 31-bit hash_combine and a weak one: let two words of a chain range over a window of a few
hundred bases (an alternative donor or acceptor) and tens of thousands of bucket values hold several chains.  Real loci therefore put
different chains into one bucket routinely; make_golden.tset_case (unrelated chains) almost never does.  This module searches such
chains with the hash written out in numpy (bucket_grid; nothing of the library is used) and draws groups from them as tset_case draws
its groups.  A *cluster* is a set of chains with one bucket value:

  visible     3..7 chains of one exon count that transcript::compare1 tells apart (scan of the last two chain words)
  hidden      2..4 chains that differ only in the exon before the last one, which intron_chain_compare (gtf/transcript.cc:218-238)
              never looks at: one item to the reference, which keeps the exons of whichever came first
  mixed       two compare1 classes in one bucket, at least one of them with two hidden variants; the classes differ in the word after
              the skipped exon or in the word before it
  cross       chains of different exon counts in one bucket
  host/device a multi-exon chain whose bucket is below 2^16 plus three single-exon transcripts with (l + r) / 10000 + 1 equal to it:
              two that overlap by the 0.8 rule and one that overlaps neither

Every chain is drawn under '+', '-' and '.'; a few unrelated chains put unshared buckets between the shared ones.  census() counts, from
the groups and the reference's items alone, how often each situation the kernels must get right occurs; both tiers assert CENSUS_MIN of
every line.  tests/golden/make_golden_tset_collide.py stores the reference's answers for CASES."""
import bisect
import functools
import itertools
import random

import numpy as np

SEED = 9157
# (groups, visible clusters per exon count, hidden clusters per exon count, mixed, cross, host/device, unrelated chains)
CASES = ((600, 2, 3, 8, 10, 4, 40), (2500, 3, 4, 8, 12, 5, 90))
VISIBLE_NE = (2, 3, 4, 6, 9)                     # 9 exons: beyond the sink's eight inline exons
HIDDEN_NE = (3, 4, 7)
MIXED_NE = (4, 5)
CROSS_NE = ((2, 3), (3, 4), (4, 6), (2, 9), (6, 9), (3, 6))
WINDOW = 1200
CENSUS_MIN = 10
CHUNKS = (1, 7)
STRANDS = "+-."
_C = np.uint64(0x9e3779b9)


def bucket_grid(base, scan=None):
    """transcript::get_intron_chain_hashing of the flat exon words `base` (l0 r0 l1 r1 ...), with the words named in `scan` = {index:
    array of values} replaced by every combination of those values -> uint64 array with one axis per scanned word, in index order
    (no scan: a 0-d array).  One exon: (l + r) / 10000 + 1 with C's truncating division; more: vector_hash (util/util.cc:38-46) over
    the inner words, seeded with their number, 31 bits, + 1.  Scanned words must be inner words."""
    scan = dict(scan or {})
    nw = len(base)
    assert nw % 2 == 0 and all(0 < i < nw - 1 for i in scan)
    if nw == 0:
        return np.zeros((), np.uint64)
    if nw == 2:
        s = int(base[0]) + int(base[1])
        assert -(1 << 31) <= s < (1 << 31)
        q = abs(s) // 10000 * (1 if s >= 0 else -1)
        return np.array((q + 1) & ((1 << 64) - 1), np.uint64)
    axes = sorted(scan)
    h = np.full((1,) * len(axes), nw - 2, np.uint64)
    for i in range(1, nw - 1):
        if i in scan:
            shape = [1] * len(axes); shape[axes.index(i)] = -1
            v = np.asarray(scan[i], np.int64).astype(np.uint64).reshape(shape)
        else:
            v = np.array(int(base[i]), np.int64).astype(np.uint64)
        with np.errstate(over="ignore"):
            h = h ^ (v + _C + (h << np.uint64(6)) + (h >> np.uint64(2)))
    h = (h & np.uint64(0x7FFFFFFF)) + np.uint64(1)
    return h.reshape([len(scan[i]) for i in axes]) if axes else h.reshape(())


def flat(exons):
    return [v for e in exons for v in e]


def bucket_of(exons):
    return int(bucket_grid(flat(exons)))


def chain_key(strand, exons):
    """what transcript_set files a multi-exon transcript under: bucket, exon count, strand and the words compare1 reads (all inner words
    but, from three exons on, those of the exon before the last)"""
    w = flat(exons); nw = len(w)
    assert nw >= 4
    vis = w[1:nw - 4] + w[nw - 2:nw - 1] if nw >= 6 else w[1:3]
    return (bucket_of(exons), nw // 2, strand, tuple(vis))


def hidden_words(exons):
    return tuple(exons[-2]) if len(exons) >= 3 else ()


def _base_chain(rng, ne):
    """exons and introns of 1500..4000 bases: any inner word may move up by a WINDOW without reaching its neighbour"""
    x = rng.randrange(1000, 2000000); ex = []
    for _ in range(ne):
        l = x + rng.randrange(1500, 4000); r = l + rng.randrange(1500, 4000); ex.append((l, r)); x = r
    return ex


def _with(base, idx, vals):
    w = flat(base)
    for i, v in zip(idx, vals):
        w[i] = int(v)
    assert all(a < b for a, b in zip(w[:-1], w[1:]))
    return tuple((w[2 * k], w[2 * k + 1]) for k in range(len(w) // 2))


def _scan(base, idx, window):
    w = flat(base)
    h = bucket_grid(w, {i: w[i] + np.arange(window) for i in idx})
    return h


def _shared(h, least, limit=256):
    """[(bucket, [grid coordinates])] of the bucket values that at least `least` points of the scan share, by bucket value (at most `limit`
    of them, evenly spaced)"""
    f = h.reshape(-1)
    order = np.argsort(f, kind="stable"); s = f[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]])); size = np.diff(np.concatenate([start, [len(s)]]))
    start, size = start[size >= least], size[size >= least]
    if len(start) > limit:
        pick = np.arange(limit) * len(start) // limit; start, size = start[pick], size[pick]
    out = []
    for a, n in zip(start, size):
        out.append((int(s[a]), [tuple(int(c) for c in np.unravel_index(k, h.shape)) for k in order[a:a + n]]))
    return out


def _chains(base, idx, coords):
    w = flat(base)
    return [_with(base, idx, [w[i] + c for i, c in zip(idx, co)]) for co in coords]


def visible_cluster(rng, ne):
    k = rng.randint(3, 7)
    while True:
        base = _base_chain(rng, ne); nw = 2 * ne; idx = (nw - 3, nw - 2)
        cand = []
        for b, co in _shared(_scan(base, idx, WINDOW), k):
            if ne >= 3:                                             # word nw - 3 is one compare1 skips: keep one chain per value of word nw - 2
                seen = {}
                for c in co:
                    seen.setdefault(c[1], c)
                co = sorted(seen.values())
            if len(co) >= k:
                cand.append((b, co))
        if cand:
            b, co = cand[rng.randrange(len(cand))]
            return dict(kind="visible", bucket=b, chains=_chains(base, idx, rng.sample(co, k)))


def hidden_cluster(rng, ne):
    k = rng.randint(2, 4)
    while True:
        base = _base_chain(rng, ne); nw = 2 * ne; idx = (nw - 4, nw - 3)
        cand = _shared(_scan(base, idx, WINDOW), k)
        if cand:
            b, co = cand[rng.randrange(len(cand))]
            return dict(kind="hidden", bucket=b, chains=_chains(base, idx, rng.sample(co, k)))


def mixed_cluster(rng, ne, first=False, window=130):
    """two compare1 classes in one bucket, the larger with two or three hidden variants.  The classes differ in the last chain word
    (nw - 2, the word after the skipped exon) or, with `first`, in word nw - 5 (the word before it)"""
    while True:
        base = _base_chain(rng, ne); nw = 2 * ne
        idx = (nw - 5, nw - 4, nw - 3) if first else (nw - 4, nw - 3, nw - 2); axis = 0 if first else 2
        cand = []
        for b, co in _shared(_scan(base, idx, window), 3):
            cls = {}
            for c in co:
                cls.setdefault(c[axis], []).append(c)
            if len(cls) >= 2 and max(len(v) for v in cls.values()) >= 2:
                two = sorted(cls.values(), key=lambda v: (-len(v), v))[:2]
                cand.append((b, two[0][:3] + two[1][:2]))
        if cand:
            b, co = cand[rng.randrange(len(cand))]
            return dict(kind="mixed", bucket=b, chains=_chains(base, idx, co))


def cross_cluster(rng, ne_a, ne_b):
    """the shorter chain's scan (its last two chain words) reaches a narrow range of bucket values; the longer chain's scan reaches wide
    (see host_device_cluster) and is repeated with other chains until it meets that range"""
    ba = _base_chain(rng, ne_a); ia = (2 * ne_a - 3, 2 * ne_a - 2)
    ha = _scan(ba, ia, WINDOW); ua = np.unique(ha)
    for _try in range(400):
        bb = _base_chain(rng, ne_b); ib = (1, 2 * ne_b - 2)
        hb = _scan(bb, ib, WINDOW)
        near = hb[(hb >= ua[0]) & (hb <= ua[-1])]
        both = np.intersect1d(near, ua)
        if len(both):
            b = both[rng.randrange(len(both))]
            ca = [tuple(int(v) for v in c) for c in np.argwhere(ha == b)][:1]
            cb = [tuple(int(v) for v in c) for c in np.argwhere(hb == b)][:1]
            return dict(kind="cross", bucket=int(b), chains=_chains(ba, ia, ca) + _chains(bb, ib, cb))
    raise AssertionError("no bucket shared by chains of %d and %d exons in 400 scans" % (ne_a, ne_b))


def host_device_cluster(rng, ne, taken):
    """a multi-exon chain in a bucket below 2^16 and three single-exon transcripts of that bucket: two that overlap by the 0.8 rule, one
    that overlaps neither.  A scan of the LAST two chain words does not get there: every step of the hash moves a word's influence up
    by six bits only, so those two words reach some 2^19 values around what the words before them fixed.  The scan takes the FIRST two
    chain words of a chain with four or more exons, whose influence has reached all 31 bits by the last step: some dozens of the chains
    of a WINDOW x WINDOW scan lie below 2^16"""
    assert ne >= 4
    hits = []
    for _try in range(50):
        base = _base_chain(rng, ne); idx = (1, 2)
        h = _scan(base, idx, WINDOW)
        hits = [tuple(int(v) for v in c) for c in np.argwhere((h < (1 << 16)) & (h >= 3))]
        hits = [c for c in hits if int(h[c]) not in taken]
        if hits:
            break
    assert hits, "no multi-exon chain below 2^16 in 50 scans of %d x %d" % (WINDOW, WINDOW)
    c = hits[rng.randrange(len(hits))]; b = int(h[c])
    mid = (b - 1) * 5000 + 2500                                     # l + r of the three: (b - 1) * 10000 + 5000, + 5040, + 1200
    singles = [((mid - 500, mid + 500),), ((mid - 480, mid + 520),), ((mid - 2400, mid - 1400),)]
    assert all(bucket_of(s) == b for s in singles)
    return dict(kind="host/device", bucket=b, chains=_chains(base, idx, [c]) + singles)


def build_clusters(rng, shape):
    _, n_vis, n_hid, n_mix, n_cross, n_hd, n_unrel = shape
    cl = []
    for ne in VISIBLE_NE:
        cl += [visible_cluster(rng, ne) for _ in range(n_vis)]
    for ne in HIDDEN_NE:
        cl += [hidden_cluster(rng, ne) for _ in range(n_hid)]
    cl += [mixed_cluster(rng, MIXED_NE[k % len(MIXED_NE)], first=k % 4 >= 2) for k in range(n_mix)]
    cl += [cross_cluster(rng, *CROSS_NE[k % len(CROSS_NE)]) for k in range(n_cross)]
    taken = set()
    for k in range(n_hd):
        cl.append(host_device_cluster(rng, (4, 5)[k % 2], taken)); taken.add(cl[-1]["bucket"])
    unrelated = []
    for _ in range(n_unrel):
        ne = rng.choice([1, 2, 2, 3, 4, 6, 9]); x = rng.randrange(1000, 2000000); ex = []
        for _k in range(ne):
            l = x + rng.randrange(20, 400); r = l + rng.randrange(30, 900); ex.append((l, r)); x = r
        w = [0.8, 0.15, 0.05]; rng.shuffle(w)
        unrelated.append((tuple(ex), w))
    for c in cl:
        assert len(set(c["chains"])) == len(c["chains"]) and all(bucket_of(x) == c["bucket"] for x in c["chains"]), c
    assert len({c["bucket"] for c in cl}) == len(cl)
    return cl, unrelated


def draw_groups(rng, n_groups, clusters, unrelated):
    """as make_golden.tset_case: 0..6 transcripts a group, outer bounds jittered, 6..8 samples.  A group has a home cluster (a graph is
    one locus) from which most of its transcripts come, so that one group brings several chains of one bucket"""
    n_samples = rng.randint(6, 8)
    groups = []; drawn = set(); tids = itertools.count()

    def transcript(chain, st):
        drawn.add((chain, st)); ex = list(chain)
        if len(ex) == 1:
            d = rng.choice([0, 0, 5, 40]); ex[0] = (ex[0][0] + d, ex[0][1] + rng.choice([d, d + 3]))
        else:
            ex[0] = (ex[0][0] - rng.choice([0, 0, 7, 90]), ex[0][1]); ex[-1] = (ex[-1][0], ex[-1][1] + rng.choice([0, 0, 11, 250]))
        return (st, round(rng.uniform(0.1, 30), 3), round(rng.random(), 4), round(rng.uniform(0, 50), 2), rng.randint(1, 9), next(tids), ex)
    for _g in range(n_groups):
        sid = rng.randrange(n_samples); ts = []
        home = clusters[rng.randrange(len(clusters))]
        for _ in range(rng.randint(0, 6)):
            u = rng.random()
            if u < 0.65:
                ex = rng.choice(home["chains"]); st = rng.choice(STRANDS)
            elif u < 0.88:
                ex = rng.choice(rng.choice(clusters)["chains"]); st = rng.choice(STRANDS)
            else:
                ex, w = rng.choice(unrelated); st = rng.choices(STRANDS, w)[0]
            ts.append(transcript(ex, st))
        groups.append((sid, ts))
    for cl in clusters:                                             # a (chain, strand) the draw left out joins a group that has room
        for ch in cl["chains"]:
            for st in STRANDS:
                if (ch, st) not in drawn:
                    ts = groups[rng.randrange(n_groups)][1]
                    while len(ts) >= 6:
                        ts = groups[rng.randrange(n_groups)][1]
                    ts.append(transcript(ch, st))
    return groups


@functools.lru_cache(maxsize=None)
def case(i):
    """(groups, clusters) of case i, drawn from the seed"""
    rng = random.Random(SEED + i)
    clusters, unrelated = build_clusters(rng, CASES[i])
    return draw_groups(rng, CASES[i][0], clusters, unrelated), clusters


def groups_of(i):
    return case(i)[0]


def multi_exon_only(groups):
    """what skip_single_exon must leave: every group keeps its place and sample id, single-exon transcripts are gone"""
    return [(sid, [t for t in ts if len(t[6]) > 1]) for sid, ts in groups]


def segments(n, parts):
    """n groups cut into `parts` consecutive segments -> their sizes"""
    cuts = [n * k // parts for k in range(parts + 1)]
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def census(groups, items):
    """counted from the groups and the reference's items (tset_parse form) alone"""
    by_tid = {t[5]: t for _, ts in groups for t in ts}
    c = {}
    # ---- runs of one bucket among the reference's items ----
    runs = []
    for k, x in enumerate(items):
        if runs and items[runs[-1][0]]["hash"] == x["hash"]:
            runs[-1].append(k)
        else:
            runs.append([k])
    size = [len(r) for r in runs]
    c["run of 2"] = sum(n == 2 for n in size); c["run of 3"] = sum(n == 3 for n in size)
    c["run of 4..7"] = sum(4 <= n <= 7 for n in size); c["run of more than 7"] = sum(n > 7 for n in size)
    ne_of = lambda r: {len(items[k]["exons"]) for k in r}
    c["run with several exon counts, all above one"] = sum(len(ne_of(r) - {1}) > 1 for r in runs)
    shared = [r for r in runs if 1 in ne_of(r) and len(ne_of(r)) > 1]
    c["host/device run: single-exon items"] = sum(len(items[k]["exons"]) == 1 for r in shared for k in r)
    c["host/device run: multi-exon items"] = sum(len(items[k]["exons"]) > 1 for r in shared for k in r)
    # ---- the multi-exon items by the key the reference files them under; their place in the reference's order ----
    pos = {}
    for k, x in enumerate(items):
        if len(x["exons"]) > 1:
            key = chain_key(by_tid[x["tid"]][0], x["exons"])
            assert key not in pos and key[0] == x["hash"]
            pos[key] = k
    variants = {}
    for _, ts in groups:
        for t in ts:
            if len(t[6]) > 1:
                variants.setdefault(chain_key(t[0], t[6]), set()).add(hidden_words(t[6]))
    assert set(variants) == set(pos)
    several = [key for key in pos if len(variants[key]) >= 2]
    c["item of two or more hidden variants"] = len(several)
    c["such an item that kept a variant other than the smallest"] = sum(hidden_words([tuple(e) for e in items[pos[key]]["exons"]]) != min(variants[key]) for key in several)
    c["group whose transcripts share a bucket"] = 0
    for _, ts in groups:
        b = {}
        for t in ts:
            b.setdefault(bucket_of(t[6]), set()).add(tuple(flat(t[6])[1:-1]) if len(t[6]) > 1 else tuple(t[6][0]))
        c["group whose transcripts share a bucket"] += any(len(v) > 1 for v in b.values())
    # ---- what a chunk brings to a run that already has resident (multi-exon) items ----
    for chunk in CHUNKS:
        resident = {}                                               # bucket -> sorted places of the resident items
        n_same = n_front = n_between = n_behind = 0
        for a in range(0, len(groups), chunk):
            new = {}
            for _, ts in groups[a:a + chunk]:
                for t in ts:
                    if len(t[6]) > 1:
                        key = chain_key(t[0], t[6]); r = resident.get(key[0], [])
                        p = pos[key]; j = bisect.bisect_left(r, p)
                        if j == len(r) or r[j] != p:
                            new.setdefault(key[0], set()).add(p)
            for b, ps in new.items():
                r = resident.setdefault(b, [])
                if r:
                    ins = [bisect.bisect_left(r, p) for p in ps]
                    n_same += len(set(ins)) < len(ins)
                    n_front += 0 in ins; n_behind += len(r) in ins; n_between += any(0 < j < len(r) for j in ins)
                for p in ps:
                    bisect.insort(r, p)
        c["chunk of %d: two or more new items at one insertion point of a run with resident items" % chunk] = n_same
        c["chunk of %d: new item in front of the resident items of its run" % chunk] = n_front
        c["chunk of %d: new item between the resident items of its run" % chunk] = n_between
        c["chunk of %d: new item behind the resident items of its run" % chunk] = n_behind
    return c
