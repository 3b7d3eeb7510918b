"""CPU tier of the extend of a 2-in / 2-out unsplittable vertex (decomp_device.h: extend_22 beside the generic decompose_vertex_extend):
the single-lane emulation against the oracle on the batches of tests/extend22_cases.py, bit for bit -- records, op trace, iteration counts --
in classes 0, 1, 2 and 10 and in the KEEP=1 checker build; a counting build says which form a batch took; a build without the fixed form
(-DALD_NO_EXTEND22) must give the same outputs, down to the status word and the line of the fail() behind it."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import numpy as np
import pytest

import common
import device_run as DR
import extend22_cases as X

ROOT = common.ROOT
CASES = sorted(X.CASES)
EMU_FLAGS = "-O1 -std=c++17 -fPIC -ffp-contract=off -fno-strict-aliasing -DALD_EMU -DALD_RAW_VARIANT -Wno-unused-function -Wno-unused-variable -Wno-sign-compare"
CLIMB = ("i_63_vertices", "i_64_vertices")      # started one class too low these end on `nv + 2 > MAXV` of class 0 (64 vertices) and climb


def _check(name, want, st, traces, got, it, tr, what):
    bad = common.compare_results(want, got, len(traces))
    assert not bad, f"{name}, {what}: {len(bad)} mismatches, first {bad[:3]}"
    assert np.array_equal(it, st[:, 3]), (name, what, np.nonzero(it != st[:, 3])[0][:10])
    for g in range(len(traces)):
        assert tr[g] == traces[g], f"{name}, {what}, graph {g}: first divergence at {DR.first_divergence(tr[g], traces[g])}"


@pytest.mark.parametrize("name", CASES)
def test_emulation_matches_the_oracle(name):
    pg, prm, (want, st, traces), hits = X.batch(name)
    assert hits > 0
    for kw in (dict(force_class=0), dict(force_class=1), dict(force_class=2), dict(force_class=10), dict(keep=True)):
        got, it, cl, tr, ln = common.emu_run_full(pg, params=prm, **kw)
        assert (cl >= kw.get("force_class", 0)).all()
        _check(name, want, st, traces, got, it, tr, kw)
        assert not ln.any(), (name, kw, ln[ln != 0][:5])


@pytest.mark.parametrize("name", CLIMB)
def test_no_room_for_two_vertices_climbs_a_class(monkeypatch, name):
    """the capacity exit: a graph of 63 / 64 vertices started in class 0 has no room for the two new vertices.  The fixed form declines, the
    generic form reports it, the graph runs again one class up and ends with the oracle's records."""
    pg, prm, (want, st, traces), _ = X.batch(name)
    monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
    got, it, cl, tr, ln = common.emu_run_full(pg, params=prm)
    assert (cl == 1).all(), np.unique(cl)
    _check(name, want, st, traces, got, it, tr, "one class too low")


# ---------------------------------------------------------------------------------------------------------------------------------------
# other builds of the emulation, made here into directories of their own and run in child processes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    out = {}
    for tag, extra in (("count", "-DALD_EMU_COUNT"), ("generic", "-DALD_NO_EXTEND22")):
        d = str(tmp_path_factory.mktemp("emu_" + tag))
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "kernel_emu"), "-j8", "OUT=" + d, "CXXFLAGS=" + EMU_FLAGS + " " + extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out[tag] = os.path.join(d, "libkernel_emu.so")
    return out


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import common, extend22_cases as X
name, out = sys.argv[1], sys.argv[2]
pg, prm, _, _ = X.batch(name)
got, it, cl, tr, ln = common.emu_run_full(pg, params=prm)
np.savez(out, status=got.status, path_offset=got.path_offset, weight=got.weight, abd=got.abd, conf=got.conf, reads=got.reads, length=got.length, count=got.count,
         strand=got.strand, pv_offset=got.pv_offset, path_vertices=got.path_vertices, it=it, cl=cl, ln=ln,
         trace=np.array([x for t in tr for op in t for x in op] + [float(len(t)) for t in tr]))
""" % (ROOT, os.path.join(ROOT, "tests"))


def _child(lib, name, out, env=None):
    e = dict(os.environ, ALD_EMU_LIB=lib); e.update(env or {})
    r = subprocess.run([sys.executable, "-c", CHILD, name, out], env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _extends(stderr):
    """(all extends, through the fixed form, declined by it) summed over the classes of a counting run"""
    rows = re.findall(r"extends: (\d+) through the fixed 2x2 form: (\d+) declined: (\d+)", stderr)
    return tuple(sum(int(r[k]) for r in rows) for k in range(3))


@pytest.mark.parametrize("name", CASES)
def test_which_form_a_batch_takes(builds, tmp_path, name):
    """the counting build: every case but the last takes the fixed form at least once -- a pair of parallel edges included, whose two relinks
    the form does on lane 0 (the comment above extend_22) --; with jump_ratio > 1 it always declines"""
    total, taken, declined = _extends(_child(builds["count"], name, str(tmp_path / "o.npz")))
    assert total > 0, name
    if name == "l_jump_ratio":
        assert taken == 0 and declined > 0, (total, taken, declined)
    else:
        assert taken > 0, (total, taken, declined)
        if name == "j_wide_beside": assert total > taken + declined       # a 2 x 3 / 3 x 2 hub never reaches the fixed form


def _extends_by_class(stderr):
    """{class: (all extends, through the fixed form, declined by it)} of a counting run"""
    out = {}; cls = None
    for ln in stderr.splitlines():
        m = re.search(r"\[emu-count\] class (\d+):", ln)
        if m: cls = int(m.group(1))
        m = re.search(r"extends: (\d+) through the fixed 2x2 form: (\d+) declined: (\d+)", ln)
        if m: out[cls] = tuple(int(x) for x in m.groups())
    return out


def test_the_fixed_form_declines_without_room(builds, tmp_path, name="i_63_vertices"):
    """63 vertices in class 0 (MAXV 64): the graph loads, and the first extend has no room for its two vertices: the attempt in class 0
    declines every time and takes the fixed form never; the retry in class 1 takes it.  (A graph of 64 vertices leaves class 0 before
    any extend.)"""
    by = _extends_by_class(_child(builds["count"], name, str(tmp_path / "o.npz"), env=dict(ALD_DEBUG_UNDERCLASS="1")))
    assert by[0][2] > 0 and by[0][1] == 0, by
    assert by[1][1] > 0 and by[1][2] == 0, by


def _sub_cases(stderr):
    rows = re.findall(r"strand to i' from o\*: (\d+) to o' from i\*: (\d+) to z from i\*: (\d+) to z from o\*: (\d+) insert_between acted: (\d+)", stderr)
    return tuple(sum(int(r[k]) for r in rows) for k in range(5))


def test_the_three_borrow_orders_and_the_phasing_edit(builds, tmp_path):
    """What the oracle's op trace cannot say -- which of the four edges occurs twice -- the counting build says from inside the fixed form:
    in the stranded batch i' takes the strand of o*, o' the strand of i*, the new edge the strand of i* (o* has none) and the strand of o*
    over an unstranded i*, each at least once; in the phasing batch a path runs through (i*, o*) and hs_insert_between edits it"""
    to_ip, to_op, z_is, z_os, _ = _sub_cases(_child(builds["count"], "g_strands", str(tmp_path / "g.npz")))
    assert min(to_ip, to_op, z_is, z_os) > 0, (to_ip, to_op, z_is, z_os)
    assert _sub_cases(_child(builds["count"], "f_phasing", str(tmp_path / "f.npz")))[4] > 0


@pytest.mark.parametrize("name", X.RAW_CASES)
def test_raw_form_in_the_emulation(name):
    """the same hubs handed over raw (the build of every class that does the pre-steps in its load phase), against the oracle's pre-steps
    + decomposition: records, iteration counts, op trace"""
    items, spg, (want, st, traces) = X.raw_batch(name)
    cap = max(len(t) for t in traces) + 8
    for fc in (0, 1, 2):
        got, it, cl, mine = common.emu_run_raw(items, params=X.params_of(name), force_class=fc, trace_cap=cap, full=True)
        assert (cl >= fc).all()
        _check(name, want, st, traces, got, it, mine, "raw, class %d" % fc)


@pytest.mark.parametrize("name", CASES)
def test_same_outputs_without_the_fixed_form(builds, tmp_path, name):
    """-DALD_NO_EXTEND22 (the generic form everywhere) against the product emulation: every array equal, the status words and the lines of
    the fail() behind them included; the 63 / 64-vertex batches also started one class too low (the capacity exit)"""
    for env in ((None, dict(ALD_DEBUG_UNDERCLASS="1")) if name in CLIMB else (None,)):
        a = str(tmp_path / "a.npz"); b = str(tmp_path / "b.npz")
        _child(builds["generic"], name, a, env); _child(os.path.join(ROOT, "tests", "_build", "libkernel_emu.so"), name, b, env)
        A_, B_ = np.load(a), np.load(b)
        for k in A_.files:
            assert np.array_equal(A_[k], B_[k]), (name, env, k)
        if env: assert A_["ln"].any() or (A_["cl"] == 1).all()
