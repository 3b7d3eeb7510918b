"""CPU tier: the threaded HOST code every integrator calls, under ThreadSanitizer, without a GPU.

Two stand-alone programs (own main, g++ -fsanitize=thread, nothing preloaded):
  tests/host_adapter/queue_tsan_main.cc        aletsch::gpu_assembly_queue (aletsch_amd/host/gpu_dispatch.hpp): lanes, chunk hand-over with
                                               back-pressure, pack / device / merge threads, drain(), the destructor, and the ERROR path
                                               (a failing upload / run / download / merge cannot be had from a GPU on request)
  tests/host_adapter/host_passes_tsan_main.cc  the passes of host_pack.h and ald_sink.cpp that go multi-threaded only above a size threshold
Both link the product's own sink (aletsch_amd/csrc/ald_sink.cpp) and staging (host_pack.h) next to tests/host_adapter/stub_batch_abi.cc, a
stand-in for the batch entry points whose "device" is the engine's emulation (its class objects are NOT instrumented: single-threaded
per call).  NOT under the sanitizer: the real ald_batch_* with their HIP streams, comm_rccl.cpp, anything loaded into Python.

A case passes when the program exits 0, its own comparisons passed, stderr holds no ThreadSanitizer line, and the thread counts it
reports are the ones asked for.  A deadlock ends a case through the timeout."""
import functools
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aletsch_amd as A
import common

ROOT = common.ROOT
HA = os.path.join(ROOT, "tests", "host_adapter")
OUT = os.path.join(ROOT, "tests", "_build", "tsan")
TSAN = ["-fsanitize=thread", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-strict-aliasing", "-include", os.path.join(HA, "thread_probe.h")]
HOST = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]           # what aletsch_amd/csrc/Makefile gives the library's host units
ENV = dict(TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", ALD_SINK_THREADS="4")
EMU_CLASSES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13)


def _cxx(std, args, src, obj):
    r = subprocess.run(["g++", "-std=" + std, *TSAN, *args, "-c", src, "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return obj


@functools.lru_cache(maxsize=None)
def programs():
    """-> (queue program, host-passes program, control program), built once per session"""
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "kernel_emu"), "-j8"], capture_output=True, text=True)      # the emulation's objects, no sanitizer
    assert r.returncode == 0, r.stderr[-2000:]
    emu = [os.path.join(ROOT, "tests", "_build", "emu_c%d.o" % c) for c in EMU_CLASSES]
    o = lambda n: os.path.join(OUT, n)
    jobs = [("c++17", HOST + ["-DALD_EMU", "-DALD_RAW_VARIANT", "-w"], os.path.join(HA, "stub_batch_abi.cc"), o("stub.o")),
            # the product's sink as it is; only the name of ald_tset_add_batch changes, so that the stand-in can count and fail its calls
            ("c++17", HOST + ["-Dald_tset_add_batch=ald_real_tset_add_batch", "-w"], os.path.join(ROOT, "aletsch_amd", "csrc", "ald_sink.cpp"), o("sink.o")),
            ("c++11", ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")], os.path.join(HA, "queue_tsan_main.cc"), o("queue.o")),      # the adapter headers promise C++11
            ("c++17", HOST + ["-w"], os.path.join(HA, "host_passes_tsan_main.cc"), o("passes.o")),
            ("c++11", ["-Wall"], os.path.join(HA, "tsan_control_race.cc"), o("control.o"))]
    with ThreadPoolExecutor(len(jobs)) as ex:
        list(ex.map(lambda j: _cxx(*j), jobs))
    exes = []
    for exe, objs in (("queue_tsan", [o("queue.o"), o("stub.o"), o("sink.o")] + emu), ("host_passes_tsan", [o("passes.o"), o("stub.o"), o("sink.o")] + emu), ("tsan_control_race", [o("control.o")])):
        r = subprocess.run(["g++", "-fsanitize=thread", "-pthread", "-o", o(exe), *objs], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        exes.append(o(exe))
    return tuple(exes)


def run(exe, args=(), text=None, timeout=240):
    return subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **ENV))      # (the programs need nothing preloaded, and nothing is added)


def cases(r):
    """the CASE lines of a clean child: exit 0, nothing from the sanitizer, no failed comparison -> [(name, {key: value})]"""
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "FAILED" not in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = []
    for ln in r.stdout.splitlines():
        if ln.startswith("CASE "):
            f = ln.split()
            assert f[-1] == "OK", ln
            out.append((f[1], dict(x.split("=", 1) for x in f[2:-1])))
    return out


@functools.lru_cache(maxsize=None)
def queue_input():
    """1600 staged graphs of 6..24 vertices and 320 raw ones (gene-like, with phases) in the text form of tests/host_adapter/mock_types.h"""
    from test_gpu_adapter import graph_text
    n, r = 1600, 320
    pg = A.synth(seed=631, n_graphs=n, v_min=6, v_max=24, edges_per_vertex=3, phasing_per_graph=4, weight_mode=2, layout_mode=1)
    pg.sample_id[:] = 0; pg.sample_abd[:] = pg.edge_weight; pg.edge_abd[:] = pg.edge_weight      # what the mock edge_info carries
    text = ["%d %d\n" % (n, r)] + [graph_text(pg.select(np.array([g]))) for g in range(n)]
    rng = np.random.default_rng(12)
    for _ in range(r):
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 8)), strand=".")
        lines = ["%d %d %d" % (g["V"], len(g["edges"]), len(phases))]
        lines += ["%r %d %d" % (float(g["vw"][i]), g["lpos"][i], g["rpos"][i]) for i in range(g["V"])]
        lines += ["%d %d %r" % (s, t, w) for s, t, w, _st, _sp in g["edges"]]                  # listing order == creation order == gr.edges()
        lines += ["%d %d %s" % (len(co), c, " ".join(str(x) for x in co)) for co, c in phases]
        text.append("\n".join(lines) + "\n")
    return "".join(text)


def test_the_sanitizer_reports_a_race_it_is_shown():
    """the liveness control: without it an environment in which ThreadSanitizer silently does nothing would pass everything below"""
    r = run(programs()[2])
    assert r.returncode != 0 and "data race" in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("T,D,P,S", [(1, 1, 1, 1), (1, 3, 2, 4), (8, 3, 1, 1), (8, 1, 2, 4)])
def test_queue_under_tsan(T, D, P, S):
    """T submitting threads, D device slots (with the delay knob: later-cut batches finish first), P pack threads, S batch objects per
    device; submit / drain / submit from other threads / drain, then a second queue fed by threads that outlived the first; raw submits
    mixed in.  One submitter: the sink equals the serial per-graph loop bit for bit, whatever D, P and S are; eight: equal as
    test_dispatch_queue_matches_the_serial_merge compares.  (The comparisons are the program's; here the thread counts it ran with.)"""
    (name, f), = cases(run(programs()[0], [str(x) for x in (T, D, P, S)], queue_input()))
    assert name == "clean"
    assert int(f["submitters"]) == 2 * T                                  # T of the first and third round + T others of the second
    assert int(f["queue_threads"]) == P + D + 1                           # pack + device + merge threads the constructor started
    assert (int(f["pack"]), int(f["devices"]), int(f["slots"])) == (P, D, S)
    assert int(f["sink"]) == 4                                            # every merge under the queue ran ALD_SINK_THREADS wide
    assert int(f["staging"]) == 1                                         # chunks of 8 graphs are far below the staging thresholds (those: test_host_passes_under_tsan)
    assert int(f["batches"]) >= 30 and int(f["items"]) > 1000


@pytest.mark.parametrize("entry,kth", [("add_packed", 120), ("upload", 12), ("run", 12), ("download", 12), ("tset_add_batch", 12)])
def test_queue_error_path_under_tsan(entry, kth):
    """One call of `entry` fails in the middle of a run of eight submitters on two slow device slots with one batch object each (the
    ready cap holds submitters back): every submitter returns or throws gpu_error, drain() throws gpu_error with the injected code
    and text, the destructor returns, the sink holds nothing a clean run does not hold and no more items than it, the program exits."""
    (name, f), = cases(run(programs()[0], ["8", "2", "2", "1", entry, str(kth)], queue_input(), timeout=120))
    assert name == "error" and f["inject"] == entry and int(f["call"]) == kth
    assert int(f["submitters"]) == 8 and int(f["returned"]) + int(f["threw"]) == 8
    assert (int(f["pack"]), int(f["devices"]), int(f["slots"])) == (2, 2, 1)
    assert int(f["items"]) <= int(f["clean_items"])


def test_host_passes_under_tsan():
    """add_packed / add_packed_raw (clean, with a non-canonical row, with a raw graph that has parallel source edges), pack_range,
    HostResults::build, ald_batch_transcript_stream, ald_tset_add_stream and ald_tset_add_batch above their thresholds: 4 threads (the
    sink 1, 4 and 16) against 1, word for word, and the sink against one ald_tset_add per graph."""
    got = cases(run(programs()[1], timeout=600))
    by = {}
    for name, f in got:
        by.setdefault(name, []).append(f)
    for name in ("add_packed", "add_packed_raw", "add_packed_noncanonical_row", "add_packed_raw_parallel_source_edges", "pack_range", "results_build"):
        (f,) = by[name]
        assert int(f["staging"]) >= 4, (name, f)
    assert int(by["add_packed_raw"][0]["started"]) >= 6                   # the copy pass AND the verdict pass, three more threads each
    assert int(by["add_packed_raw_parallel_source_edges"][0]["rc"]) == -1 and int(by["add_packed_noncanonical_row"][0]["rc"]) == 0
    assert int(by["results_build"][0]["paths"]) >= 50000
    assert [int(f["sink"]) for f in by["sink"]] == [1, 4, 16]
    for f in by["sink"]:
        assert int(f["stream"]) == int(f["add_stream"]) == int(f["add_batch"]) == int(f["sink"]), f
