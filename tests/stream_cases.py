"""Named transcript streams for the stream index (aletsch_amd/csrc/tset_index.hip), shared by the CPU and the GPU tier: chains whose length
sits around every round of the pointer doubling, long records among short ones, payloads whose words read as record headers (decoys), and
the streams the host walk refuses, each with the check of the walk that refuses it.  refusal() restates the walk's checks in Python."""
import numpy as np

from test_owner_split_cpu import HDR, walk
from test_owner_split_gpu import chain, one

CHAIN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097)


def zero_exon_records(n, first_graph=0):
    """n records without exons (12 words each: the longest chain a stream of that size can hold), three to a graph"""
    w = np.tile(one(0, 0, []), n).reshape(n, HDR)
    w[:, 0] = first_graph + np.arange(n) // 3; w[:, 1] = np.arange(n) % 3
    return np.ascontiguousarray(w.reshape(-1))


def two_exon(g, n=1):
    return [one(g + i, 0, chain(2, 5000 * (g + i))) for i in range(n)]


def filled(g, n_exons, value):
    """a record whose 2 * n_exons exon words all equal `value`: every even position of the payload reads as the header of a record of `value` exons"""
    return one(g, 0, [(value, value)] * n_exons)


def _mixed_counts():
    rng = np.random.default_rng(20260)
    return one(60, 0, rng.integers(0, 7, (90, 2)).tolist())


WELL_FORMED = {"chain of %d" % n: zero_exon_records(n) for n in CHAIN_LENGTHS}
WELL_FORMED.update({
    # a 16-lane group that loops 13 / 626 times beside groups that loop once; 10 012 words is longer than any LDS tile
    "200 exons among 2": np.concatenate(two_exon(0, 20) + [one(20, 0, chain(200, 77))] + two_exon(21, 20)),
    "5000 exons among 2": np.concatenate(two_exon(0, 20) + [one(20, 0, chain(5000, 77))] + two_exon(21, 20)),
    "5000 exons first": np.concatenate([one(0, 0, chain(5000, 77))] + two_exon(1, 20)),
    "200 exons last": np.concatenate(two_exon(0, 20) + [one(20, 0, chain(200, 77))]),
    # payload positions read as zero-exon records: their chains step by 12 words, every sixth of them onto the next real record (or the end)
    "decoy zeros": np.concatenate(two_exon(0, 5) + [filled(5, 60, 0)] + two_exon(6, 3) + [filled(9, 66, 0)] + two_exon(10, 5) + [filled(15, 60, 0)]),
    # payload words equal to small counts: chains that step by 14, 16, 18, 22 words and merge into the real chain, end exactly on n_words
    # (the last record), or run into a word that is no count (-1, 0x7FFFFFFF, the high half of a double in the next header)
    "decoy counts": np.concatenate(two_exon(0, 4) + [filled(4, 70, 1)] + two_exon(5, 2) + [filled(7, 64, 2)] + [filled(8, 63, 3)] + two_exon(9, 2) + [filled(11, 55, 5)]
                                   + [filled(12, 40, -1)] + [filled(13, 40, 0x7FFFFFFF)] + [_mixed_counts()] + two_exon(61, 3) + [filled(64, 70, 1)]),
    "equal and large graph ids": np.concatenate([one(5, 0, chain(3, 100)), one(5, 1, chain(2, 900)), one(0x80000000, 0, chain(3, 100)), one(0x80000000, 1, []),
                                                 one(0xFFFFFFFF, 0, chain(4, 40))]),
})
DECOYS = ("decoy zeros", "decoy counts")


def _count(rec, value):
    rec = rec.copy(); rec[5] = value
    return rec


# the last record (or pair) of a refused stream and the check of the host walk that refuses it
_BAD_TAILS = {
    "odd n_words": (np.append(one(7000, 0, chain(2, 10)), np.uint32(0)), "header"),
    "n_words = 10": (one(7000, 0, [])[:10], "header"),
    "count 0x80000000": (_count(one(7000, 0, chain(2, 10)), 0x80000000), "negative"),
    "count 0x7FFFFFFF": (_count(one(7000, 0, chain(2, 10)), 0x7FFFFFFF), "overrun"),       # 12 + 2 * 0x7FFFFFFF needs 64 bits
    "overrun by two words": (one(7000, 0, chain(3, 10))[:-2], "overrun"),
    "descending last pair": (np.concatenate([one(7001, 0, chain(2, 10)), one(7000, 0, chain(2, 10))]), "descending"),
}
MALFORMED = {}
for _name, (_tail, _why) in _BAD_TAILS.items():
    MALFORMED[_name + ", alone"] = (_tail, _why)
    MALFORMED[_name + ", behind 4096"] = (np.concatenate([zero_exon_records(4096), _tail]), _why)


def refusal(words):
    """the host walk's checks (tx_stream_records): None for a stream it accepts, else which check refuses it"""
    n = len(words); o = 0; last = -1
    while o < n:
        if o + HDR > n:
            return "header"
        c = int(words[o + 5])
        if c >= 1 << 31:
            return "negative"
        if o + HDR + 2 * c > n:
            return "overrun"
        if int(words[o]) < last:
            return "descending"
        last = int(words[o]); o += HDR + 2 * c
    return None


def successor(words, o):
    """the three conditions of the index for an even position o: the next position, or None"""
    n = len(words)
    if o + HDR > n or int(words[o + 5]) >= 1 << 31 or o + HDR + 2 * int(words[o + 5]) > n:
        return None
    return o + HDR + 2 * int(words[o + 5])


def runs(words):
    """number of runs of equal graph id"""
    g = [int(words[o]) for o, _ in walk(words)]
    return sum(1 for i in range(len(g)) if i == 0 or g[i] != g[i - 1])
