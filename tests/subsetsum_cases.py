"""Instance families for the two-sided subset-sum DP (aletsch_amd/csrc/subsetsum_kernel.hip, oracle/subsetsum_oracle.hpp; reference
scallop/subsetsum.cc:20-206), and a census that says what a list of instances actually exercises.

An instance is (source, target), each a list of (value, label).  Every family is deterministic from its seed.  The domain is the one the
reference defines: every value >= 1 and every side's sum below 2^31 (values <= MAX_VALUE with at most 32 items).  Zero or negative
values and overflowing sums are undefined behaviour in the reference (division by a zero sum, negative table indices, signed overflow)
and stay out of scope.  The kernel takes 1..32 items per side; the `out_of_range` family (0 or 33 items on a side) is the one family
that never goes to the reference or the oracle: the kernel refuses it before it reads anything, the expected answer is None.

What the rescaling can reach: the side with the larger sum s > 1000 is multiplied by 1000 / s and truncated, so its truncated values add
up to at most 999 unless nothing was cut; an item that truncates to 0 is bumped to 1.  Not every item of a side can be bumped (the products
add up to the common bound), so at most 31 are, and the largest table bound is ub = 999 + 31 - 1 = 1029 (SS_MAXS = 1040 in the kernel).

census() restates rescale() with Python integers and floats and runs the dynamic programme naively (a bit set of sums per side).  It is
test-side arithmetic for counting buckets and for laying out a batch; it is never the expected answer (that is the reference's stored
output, or the oracle).
"""
import random

MAX_VALUE = 60000000
MAX_ITEMS = 32
SIZE_GRID = (1, 2, 3, 12, 13, 31, 32)
RANDOM_HI = (3, 20, 100, 1000, 5000, 10 ** 6)
GRID = 2048                                   # ald_subsetsum_batch launches min(n, 2048) blocks; block b runs b, b + 2048, ...


def _plain(sv, tv):
    """labels as tests/golden/make_golden.py gives them: i / 100 + i in input order"""
    return [(v, i) for i, v in enumerate(sv)], [(v, 100 + i) for i, v in enumerate(tv)]


def _shuffled_labels(rng, sv, tv):
    ls = list(range(len(sv))); lt = list(range(100, 100 + len(tv))); rng.shuffle(ls); rng.shuffle(lt)
    return list(zip(sv, ls)), list(zip(tv, lt))


def sizes(rng, n):
    """every (n1, n2) of SIZE_GRID x SIZE_GRID in turn, value scales 3 / 40 / 1000 / 10^6 in turn"""
    out = []
    grid = [(a, b) for a in SIZE_GRID for b in SIZE_GRID]
    scales = (3, 40, 1000, 10 ** 6)
    for k in range(n):
        n1, n2 = grid[k % len(grid)]; hi = scales[(k // len(grid)) % len(scales)]
        out.append(_plain([rng.randint(1, hi) for _ in range(n1)], [rng.randint(1, hi) for _ in range(n2)]))
    return out


def _bump_side(rng, k, n_big, small_hi):
    big = [rng.randint(10 ** 6, MAX_VALUE if n_big == 1 else 10 ** 7) for _ in range(n_big)]
    v = big + [rng.randint(1, small_hi) for _ in range(k)]
    rng.shuffle(v)
    return v


def bumps(rng, n):
    """scale-down with bumps: one or two values of 10^6..6*10^7 among k <= 31 small ones, which truncate to 0 and are bumped to 1.
    Every fourth instance is the maximum of the domain on one or both sides: one huge value and 31 small ones, ub = 1029."""
    out = []
    for k in range(n):
        if k % 4 == 0:
            sv = _bump_side(rng, 31, 1, rng.choice([1, 5, 200]))
            tv = _bump_side(rng, 31, 1, 3) if k % 8 == 0 else [rng.randint(1, 10 ** 6) for _ in range(rng.randint(2, 32))]
            if k % 16 == 4:
                sv, tv = tv, sv
        else:
            nb1, nb2 = rng.choice([1, 1, 2]), rng.choice([1, 1, 2])
            sv = _bump_side(rng, rng.randint(1, MAX_ITEMS - nb1), nb1, rng.choice([1, 20, 900]))
            tv = _bump_side(rng, rng.randint(1, MAX_ITEMS - nb2), nb2, rng.choice([1, 20, 900, 20000]))
        out.append(_shuffled_labels(rng, sv, tv) if k % 3 == 0 else _plain(sv, tv))
    return out


def _with_sum(rng, n, total):
    """n values >= 1 adding up to total"""
    cuts = sorted(rng.sample(range(1, total), n - 1)) if n > 1 else []
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def scale_up(rng, n):
    """both sums below 1000, so the smaller side is multiplied by a ratio > 1 and truncated: ratios next to 1 (sums one or a few apart),
    far from 1 (a sum of a few units against several hundred), and equal sums, where both ratios are exactly 1"""
    out = []
    for k in range(n):
        big = rng.randint(40, 999)
        kind = k % 4
        if kind == 0:
            small = big - rng.randint(1, 3)
        elif kind == 1:
            small = rng.randint(2, max(2, big // 20))
        elif kind == 2:
            small = big
        else:
            small = rng.randint(2, big - 1)
        n1 = rng.randint(1 if k % 16 == 15 else 2, min(MAX_ITEMS, big)); n2 = rng.randint(2, min(MAX_ITEMS, small))
        sv, tv = _with_sum(rng, n1, big), _with_sum(rng, n2, small)
        if k % 2:
            sv, tv = tv, sv
        out.append(_plain(sv, tv))
    return out


def _dense_side(rng, kind, total):
    """a side whose subsets reach every sum below its total"""
    if kind == 0:                                                   # all ones
        return [1] * min(MAX_ITEMS, total)
    v = [1, 2, 4, 8, 16, 32, 64, 128, 256] if kind == 1 else [1, 1, 2, 4, 8, 16, 32, 64, 128, 256]
    while sum(v) > total - 1:
        v.pop()
    rest = total - sum(v)
    while rest > 0:                                                 # each further item is at most one more than what is reachable so far
        x = min(rest, sum(v) + 1); v.append(x); rest -= x
    return v


def dense(rng, n):
    """all ones; powers of two; 1, 1, 2, 4, ...: every sum is achievable on both sides, so the list holds about 2 * ub entries, every lane
    of the compaction writes both of its slots and the distance 0 occurs at every sum.  Three in four have equal totals of 520..1000 (both
    ratios exactly 1); the others differ a little, carry a common factor (a true scale-down) or a few items that get bumped."""
    out = []
    for k in range(n):
        kind = (k // 2) % 3 if k % 8 else 0
        if kind == 0:
            sv, tv = _dense_side(rng, 0, rng.randint(20, 32)), _dense_side(rng, rng.choice([0, 1, 2]), rng.randint(20, 32))
        else:
            t1 = rng.randint(520, 1000); mode = k % 4
            t2 = t1 if mode != 3 else rng.randint(max(520, t1 - 30), t1)
            sv, tv = _dense_side(rng, kind, t1), _dense_side(rng, 3 - kind, t2)
            if mode == 2 and k % 16 == 2:
                f = rng.choice([1000, 59000])
                sv = [x * f for x in sv] + [rng.randint(1, 3) for _ in range(rng.randint(1, 8))]; tv = [x * f for x in tv]
        rng.shuffle(sv); rng.shuffle(tv)
        out.append(_shuffled_labels(rng, sv, tv) if k % 2 else _plain(sv, tv))
    return out


def _distinct_with_sum(rng, n, total):
    """n distinct integers >= 0 adding up to total"""
    c = list(range(n))
    assert sum(c) <= total, "no distinct split of %d into %d" % (total, n)
    for _ in range(total - sum(c)):
        while True:
            i = rng.randrange(n)
            if c[i] + 1 not in c:
                c[i] += 1
                break
    return c


def ties(rng, n):
    """the minimum distance at many list positions, far apart.  The source is m * (1, 2, 4, ...): its sums are the multiples of m.  The target
    has m items that are all 1 modulo m and the same total, so none of its listed sums is a multiple of m: a single item sits one above a
    multiple of m and a set of m - 1 items one below, which gives about 2m positions with d == 1 spread over a list of several hundred
    entries.  Every third instance instead has multiples of m on both sides (d == 0 at every common sum, first one late in the list
    when the target's smallest item is large)."""
    out = []
    for k in range(n):
        m = 3 + k % 7
        p = max(q for q in range(2, 10) if m * (2 ** q - 1) <= 1000)
        if k % 5 == 4 and m * (m - 1) // 2 <= 2 ** (p - 1) - 2:
            p -= 1
        sv = [m << i for i in range(p)]
        units = 2 ** p - 1
        if k % 3 == 2:
            nt = rng.randint(2, 6)
            tv = [m * x for x in _with_sum(rng, nt, units)]
        else:
            tv = [1 + m * c for c in _distinct_with_sum(rng, m, units - 1)]
        assert sum(sv) == sum(tv)
        rng.shuffle(sv); rng.shuffle(tv)
        if k % 2:
            sv, tv = tv, sv
        out.append(_plain(sv, tv))
    return out


def order(rng, n):
    """what the (value, label) sort has to get right: duplicate values with shuffled labels, labels descending, identical (value, label) pairs,
    labels that are large or negative int32 -- the reference sorts pairs with std::sort, the kernel with an insertion sort"""
    out = []
    for k in range(n):
        n1, n2 = rng.randint(2, MAX_ITEMS), rng.randint(2, MAX_ITEMS)
        hi = rng.choice([2, 4, 9, 30])                              # few distinct values: many duplicates
        f = rng.choice([1, 1, 7, 1000, 250000])
        sv = [f * rng.randint(1, hi) for _ in range(n1)]; tv = [f * rng.randint(1, hi) for _ in range(n2)]
        kind = k % 4
        if kind == 0:
            s, t = _shuffled_labels(rng, sv, tv)
        elif kind == 1:
            s = [(v, 1000 - i) for i, v in enumerate(sv)]; t = [(v, 2000 - i) for i, v in enumerate(tv)]
        elif kind == 2:                                             # labels from a pool of three: identical pairs
            s = [(v, rng.choice([7, 7, 8])) for v in sv]; t = [(v, rng.choice([-1, 0, 0])) for v in tv]
        else:
            pool = [2 ** 31 - 1, -2 ** 31, -1, 0, 1, 2 ** 31 - 2, -2 ** 31 + 1, 65536, -65536]
            s = [(v, rng.choice(pool) if rng.random() < 0.5 else rng.randint(-2 ** 31, 2 ** 31 - 1)) for v in sv]
            t = [(v, rng.choice(pool) if rng.random() < 0.5 else rng.randint(-2 ** 31, 2 ** 31 - 1)) for v in tv]
        out.append((s, t))
    return out


def refused(rng, n):
    """instances the reference aborts on: one item on both sides (an empty list), or one side whose only item leaves the list with the other
    side's tag alone"""
    out = []
    for k in range(n):
        hi = rng.choice([1, 50, 10 ** 6])
        kind = k % 4
        if kind == 0:
            sv, tv = [rng.randint(1, hi)], [rng.randint(1, hi)]
        elif kind == 1:
            sv, tv = [rng.randint(1, hi)], [rng.randint(1, hi) for _ in range(rng.randint(2, MAX_ITEMS))]
        elif kind == 2:
            sv, tv = [rng.randint(1, hi) for _ in range(rng.randint(2, MAX_ITEMS))], [rng.randint(1, hi)]
        else:
            sv, tv = [rng.randint(1, hi) for _ in range(MAX_ITEMS)], [MAX_VALUE]
        out.append(_plain(sv, tv))
    return out


def out_of_range(rng, n):
    """0 or 33 items on a side: refused by the kernel before it reads anything; never given to the reference or the oracle"""
    out = []
    for k in range(n):
        a = [0, MAX_ITEMS + 1, rng.randint(1, MAX_ITEMS), rng.randint(1, MAX_ITEMS), 0, MAX_ITEMS + 1][k % 6]
        b = [rng.randint(1, MAX_ITEMS), rng.randint(1, MAX_ITEMS), 0, MAX_ITEMS + 1, MAX_ITEMS + 1, 0][k % 6]
        out.append(_plain([rng.randint(1, 1000) for _ in range(a)], [rng.randint(1, 1000) for _ in range(b)]))
    return out


def random_instances(rng, n):
    """as tests/golden/make_golden.py draws them, with 1..32 items a side and a wider choice of value ranges"""
    out = []
    for _ in range(n):
        ns, nt = rng.randint(1, MAX_ITEMS), rng.randint(1, MAX_ITEMS)
        hi = rng.choice(RANDOM_HI)
        out.append(_plain([rng.randint(1, hi) for _ in range(ns)], [rng.randint(1, hi) for _ in range(nt)]))
    return out


FAMILIES = {"sizes": sizes, "bumps": bumps, "scale_up": scale_up, "dense": dense, "ties": ties, "order": order, "refused": refused,
            "out_of_range": out_of_range, "random": random_instances}
FIXTURE_SEED = 20261017
FIXTURE_COUNTS = {"sizes": 196, "bumps": 200, "scale_up": 160, "dense": 96, "ties": 140, "order": 160, "refused": 24, "random": 524}
LIVE_COUNTS = {"sizes": 588, "bumps": 900, "scale_up": 500, "dense": 700, "ties": 500, "order": 500, "refused": 300, "out_of_range": 420, "random": 1736}


def draw(counts, seed, without=()):
    """[(family name, source, target)]: counts[name] instances of every family, each family from its own stream of the seed"""
    out = []
    for name, n in counts.items():
        if name in without:
            continue
        rng = random.Random("%d/%s" % (seed, name))
        out += [(name, s, t) for s, t in FAMILIES[name](rng, n)]
    return out


def fixture_selection(without=()):
    """what tests/golden/make_golden_subsetsum.py hands to the reference: every family except out_of_range"""
    return draw(FIXTURE_COUNTS, FIXTURE_SEED, without)


def in_range(s, t):
    return 1 <= len(s) <= MAX_ITEMS and 1 <= len(t) <= MAX_ITEMS


# ---- census ----
def rescaled(s, t):
    """subsetsum.cc:31-71 in Python numbers -> (values of the source, values of the target, scale-up?) before sorting"""
    s1 = sum(v for v, _ in s); s2 = sum(v for v, _ in t)
    ubound = min(max(s1, s2), 1000)
    r1 = ubound * 1.0 / s1; r2 = ubound * 1.0 / s2
    a = [int(v * r1) for v, _ in s]; b = [int(v * r2) for v, _ in t]
    return a, b, (s1 < 1000 and s2 < 1000 and s1 != s2)


def _sums(vals, ub):
    reach = 1
    for v in vals:
        reach |= reach << v
    return [j for j in range(1, ub + 1) if (reach >> j) & 1]


def census_one(s, t):
    """what one instance exercises; an out-of-range instance only says so"""
    c = {"n1": len(s), "n2": len(t), "out_of_range": not in_range(s, t)}
    if c["out_of_range"]:
        return c
    a, b, up = rescaled(s, t)
    c["bumps1"] = sum(1 for v in a if v <= 0); c["bumps2"] = sum(1 for v in b if v <= 0)
    a = [max(v, 1) for v in a]; b = [max(v, 1) for v in b]
    c["ub1"] = sum(a) - 1; c["ub2"] = sum(b) - 1; c["scale_up"] = up
    c["duplicates"] = len(set(a)) < len(a) or len(set(b)) < len(b)
    lst = sorted([(j, 1) for j in _sums(a, c["ub1"])] + [(j, 2) for j in _sums(b, c["ub2"])])
    c["list"] = len(lst)
    cross = [(lst[i + 1][0] - lst[i][0], i) for i in range(len(lst) - 1) if lst[i][1] != lst[i + 1][1]]
    c["refused"] = not cross
    if cross:
        d = min(x for x, _ in cross); pos = [i for x, i in cross if x == d]
        c["d"] = d; c["minima"] = len(pos); c["spread"] = pos[-1] - pos[0]; c["first"] = pos[0]
    else:
        c["d"] = None; c["minima"] = 0; c["spread"] = 0; c["first"] = -1
    return c


def census(instances):
    """[(source, target)] -> one dict per instance (census_one)"""
    return [census_one(s, t) for s, t in instances]


def _items_bucket(n):
    return "1" if n == 1 else "2..12" if n <= 12 else "13..31" if n <= 31 else "32"


def buckets(cs):
    """the bucket counts of a census.  Per-side quantities (bumped items, ub) count an instance in a bucket when either side falls into it."""
    names = ["items %s %s" % (side, b) for side in ("source", "target") for b in ("1", "2..12", "13..31", "32")]
    names += ["bumped 0", "bumped 1..8", "bumped 9..31", "ub <= 100", "ub 101..999", "ub 1000..1031", "list <= 64", "list 65..1024", "list > 1024",
              "minima 1", "minima 2..8", "minima > 8", "minima >= 64 apart", "d == 0", "scale-up", "duplicate values", "refused"]
    b = dict.fromkeys(names, 0)
    for c in cs:
        if c["out_of_range"]:
            continue
        b["items source " + _items_bucket(c["n1"])] += 1; b["items target " + _items_bucket(c["n2"])] += 1
        bm = (c["bumps1"], c["bumps2"]); ub = (c["ub1"], c["ub2"])
        b["bumped 0"] += max(bm) == 0
        b["bumped 1..8"] += any(1 <= x <= 8 for x in bm); b["bumped 9..31"] += any(x >= 9 for x in bm)
        b["ub <= 100"] += any(x <= 100 for x in ub); b["ub 101..999"] += any(101 <= x <= 999 for x in ub); b["ub 1000..1031"] += any(x >= 1000 for x in ub)
        b["list <= 64"] += c["list"] <= 64; b["list 65..1024"] += 65 <= c["list"] <= 1024; b["list > 1024"] += c["list"] > 1024
        b["minima 1"] += c["minima"] == 1; b["minima 2..8"] += 2 <= c["minima"] <= 8; b["minima > 8"] += c["minima"] > 8
        b["minima >= 64 apart"] += c["spread"] >= 64
        b["d == 0"] += c["d"] == 0
        b["scale-up"] += bool(c["scale_up"]); b["duplicate values"] += bool(c["duplicates"]); b["refused"] += bool(c["refused"])
    return b


MIN_PER_BUCKET = 10


# ---- a batch laid out against the grid-stride loop ----
LARGE = lambda c: not c["out_of_range"] and not c["refused"] and max(c["ub1"], c["ub2"]) >= 1000      # noqa: E731
SMALL = lambda c: not c["out_of_range"] and not c["refused"] and max(c["ub1"], c["ub2"]) <= 100       # noqa: E731
DENSE = lambda c: not c["out_of_range"] and not c["refused"] and c["list"] > 1024                     # noqa: E731
SPARSE = lambda c: not c["out_of_range"] and not c["refused"] and c["list"] <= 64                     # noqa: E731
REFUSED = lambda c: not c["out_of_range"] and c["refused"]                                            # noqa: E731
OOR = lambda c: c["out_of_range"]                                                                     # noqa: E731
VALID = lambda c: not c["out_of_range"] and not c["refused"]                                          # noqa: E731
# what a block meets in its first, second and third instance; every pattern is laid on PATTERN_BLOCKS blocks
PATTERNS = ((LARGE, SMALL, LARGE), (SMALL, LARGE, SMALL), (DENSE, SPARSE, DENSE), (REFUSED, VALID, OOR), (OOR, VALID, REFUSED), (VALID, OOR, VALID))
PATTERN_BLOCKS = 64
ORDERS = {"large ub then small ub": (LARGE, SMALL), "small ub then large ub": (SMALL, LARGE), "dense list then sparse list": (DENSE, SPARSE),
          "refused then valid": (REFUSED, VALID), "out of range then valid": (OOR, VALID), "valid then out of range": (VALID, OOR)}
MIN_PER_ORDER = 50


def reuse_batch(seed=20261018):
    """3 * GRID instances of all families, ordered so that block b runs instances b, b + GRID and b + 2 * GRID with adverse neighbours:
    the first len(PATTERNS) * PATTERN_BLOCKS blocks follow PATTERNS, the others take what is left in a shuffled order.
    -> (instances, census, family names)"""
    pool = draw(LIVE_COUNTS, seed)
    assert len(pool) == 3 * GRID, len(pool)
    cs = census([(s, t) for _, s, t in pool])
    rng = random.Random(seed)
    idx = list(range(len(pool))); rng.shuffle(idx)
    used = set(); slots = [None] * len(pool)

    def take(pred):
        for i in idx:
            if i not in used and pred(cs[i]):
                used.add(i)
                return i
        raise AssertionError("the pool ran out of instances for a pattern")
    for b in range(len(PATTERNS) * PATTERN_BLOCKS):
        for tier, pred in enumerate(PATTERNS[b % len(PATTERNS)]):
            slots[b + tier * GRID] = take(pred)
    rest = iter([i for i in idx if i not in used])
    slots = [next(rest) if x is None else x for x in slots]
    assert sorted(slots) == list(range(len(pool)))
    return [(pool[i][1], pool[i][2]) for i in slots], [cs[i] for i in slots], [pool[i][0] for i in slots]


def order_counts(cs, grid=GRID):
    """how often each adverse order of ORDERS occurs between consecutive instances of one block"""
    n = dict.fromkeys(ORDERS, 0)
    for i in range(len(cs) - grid):
        for name, (first, then) in ORDERS.items():
            n[name] += bool(first(cs[i]) and then(cs[i + grid]))
    return n


# ---- the oracle's answer ----
def oracle_answer(s, t):
    """oracle/subsetsum_oracle.hpp on one instance -> (e, S labels, T labels), or None where it refuses; out-of-range instances never get here"""
    import ctypes as C
    import numpy as np
    import common
    assert in_range(s, t)
    O = common.oracle_lib()
    sv = np.array([v for v, _ in s], np.int32); sl = np.array([l for _, l in s], np.int32)
    tv = np.array([v for v, _ in t], np.int32); tl = np.array([l for _, l in t], np.int32)
    err = C.c_double(); ns = C.c_int32(); nt = C.c_int32(); os_ = np.zeros(64, np.int32); ot = np.zeros(64, np.int32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    if O.ora_subsetsum(len(s), len(t), p(sv), p(sl), p(tv), p(tl), C.byref(err), C.byref(ns), C.byref(nt), p(os_), p(ot)) != 0:
        return None
    return err.value, os_[:ns.value].tolist(), ot[:nt.value].tolist()


def stored_answer(a):
    """an answer of the fixture in the shape of oracle_answer / aletsch_amd.subsetsum_batch"""
    return None if a is None else (a["e"], a["s"], a["t"])
