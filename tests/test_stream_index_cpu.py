"""The stream index, CPU tier: the two entry points are declared, exported and bound; no CPU fallback; and the named streams of
tests/stream_cases.py are what they claim to be -- the host walk accepts every well-formed one, refuses every malformed one for its stated
reason, and the decoy streams really hold off-chain positions that read as record headers, some of whose chains end exactly on n_words."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
from stream_cases import DECOYS, MALFORMED, WELL_FORMED, refusal, runs, successor
from test_dev_tset_cpu import as_groups
from test_dev_tset_gpu import stream_of
from test_owner_split_cpu import GOLDEN, ROOT, walk
from test_owner_split_gpu import EDGE_STREAMS

ENTRY_POINTS = ["ald_tset_index_stream", "ald_tset_dev_stream_stats"]


def test_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aletsch_decomp.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", A.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ald_\w+)", syms))
    lib = A.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(exported) == 89 and len(set(re.findall(r"\b(ald_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))) == 89
    assert callable(A.index_stream_into) and callable(A.DeviceTranscriptSet.add_stream_ptr) and callable(A.DeviceTranscriptSet.stream_stats)


def test_index_has_no_cpu_fallback():
    import torch
    w = WELL_FORMED["chain of 3"]
    nt = C.c_int64(-5); ng = C.c_int64(-5)
    rc = A.load_library().ald_tset_index_stream(0, C.c_void_p(w.ctypes.data), C.c_int64(w.size), None, C.c_int64(0), C.byref(nt), C.byref(ng))
    if torch.cuda.is_available():
        assert rc == 0 and (nt.value, ng.value) == (3, 1)
    else:
        assert rc == -2                                              # ALD_ERR_NO_DEVICE
        with pytest.raises(A.DecompError) as e:
            A.index_stream_into(w.ctypes.data, w.size, None, 0)
        assert e.value.code == -2


def test_the_walk_accepts_every_well_formed_stream():
    streams = dict(WELL_FORMED); streams.update(EDGE_STREAMS)
    streams.update({"golden %d" % i: stream_of(as_groups(GOLDEN[i][0]), 0)[0] for i in range(len(GOLDEN))})
    for name, w in streams.items():
        assert w.dtype == np.uint32 and refusal(w) is None, name
        recs = walk(w)
        assert sum(n for _, n in recs) == len(w) and 0 <= runs(w) <= len(recs), name
    assert len(walk(WELL_FORMED["chain of 4097"])) == 4097 and len(WELL_FORMED["chain of 4097"]) == 12 * 4097
    assert max(n for _, n in walk(WELL_FORMED["5000 exons among 2"])) == 10012


def test_every_malformed_stream_is_refused_for_its_stated_reason():
    assert len(MALFORMED) == 12
    for name, (w, why) in MALFORMED.items():
        assert refusal(w) == why, name
        if "behind 4096" in name:                                    # everything in front of the last record (pair) is good
            assert len(w) > 12 * 4096 and refusal(w[:12 * 4096]) is None, name
    assert len(MALFORMED["odd n_words, alone"][0]) % 2 == 1 and len(MALFORMED["n_words = 10, alone"][0]) == 10
    w = MALFORMED["overrun by two words, alone"][0]
    assert 12 + 2 * int(w[5]) == len(w) + 2


@pytest.mark.parametrize("name", DECOYS)
def test_decoys_are_not_vacuous(name):
    """at least 100 even positions off the real chain pass the three successor conditions, and the chains of at least 10 of them end
    exactly on n_words (merged into the real chain or on their own)"""
    w = WELL_FORMED[name]; n = len(w)
    real = {o for o, _ in walk(w)}
    ends = {}                                                       # position -> does its chain end on n_words?

    def chain_ends(o):
        path = []
        while o is not None and o != n and o not in ends:
            path.append(o); o = successor(w, o)
        res = o == n or (o is not None and ends[o])
        for p in path:
            ends[p] = res
        return res
    passing = [o for o in range(0, n, 2) if o not in real and successor(w, o) is not None]
    ending = [o for o in passing if chain_ends(o)]
    assert len(passing) >= 100 and len(ending) >= 10, (name, len(passing), len(ending))
    assert any(not chain_ends(o) for o in passing), name              # and some run into a position that is no header
