"""CPU tier: the host side of compact input (ald_params.reserved & ALD_PARAM_COMPACT_INPUT; HostBatch in aletsch_amd/csrc/host_pack.h).

tests/compact_input_main.cc is a stand-alone program over host_pack.h and the case list of tests/compact_input_cases.h (the list the GPU
tier runs through the expand kernels), built here with the address and undefined-behaviour sanitizers: a compact batch after
ensure_in_csr() equals an eager one in every section, layout() marks exactly the expected sections derived, a defective graph in the
middle of an add_packed call rolls back to equality (flags included), clear() and reuse work.
"""
import os
import subprocess

import aletsch_amd as A
import common


def test_compact_host_batch_equals_the_eager_one():
    out = os.path.join(common.ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "compact_input_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(common.ROOT, "tests", "compact_input_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("0 failures") and "FAIL" not in r.stdout, r.stdout[-4000:]
    assert r.stderr.strip() == "", r.stderr[-4000:]          # no sanitizer report


def test_the_bit_is_public_and_off_by_default():
    assert A.PARAM_COMPACT_INPUT == 1
    text = open(os.path.join(common.ROOT, "include", "aletsch_decomp.h")).read()
    assert "#define ALD_PARAM_COMPACT_INPUT 1" in text
    assert A.AldParams().reserved == 0


def test_adapter_configuration_sets_the_bit():
    """tests/compact_input_config_main.cc: stage_params (what gpu_scallop_batch and gpu_assembly_queue create their batches with) sets the
    bit from a configuration's `compact_input` member and leaves it clear for a configuration that has none; g++ -std=c++11 as the reference"""
    out = os.path.join(common.ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "compact_input_config_main")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I" + os.path.join(common.ROOT, "include"), "-I" + os.path.join(common.ROOT, "aletsch_amd", "host"),
                        os.path.join(common.ROOT, "tests", "compact_input_config_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0 failures", r.stdout


def test_omitted_columns_are_found_by_name():
    """DecompBatch.add(pg, omit=...) nulls an argument by its name in PackedGraphs.C_ARG_NAMES: the list must be c_args(), name by name"""
    import ctypes as C
    from aletsch_amd.packed import PackedGraphs
    pg = A.synth(seed=5, n_graphs=3, v_min=5, v_max=9, edges_per_vertex=2)
    pg.edge_count = pg.sample_counts(); pg.edge_rank = pg.identity_rank()
    args = pg.c_args(); names = PackedGraphs.C_ARG_NAMES
    assert len(args) == len(names) and names[0] == "n" and args[0].value == pg.n
    for k, a in zip(names[1:], args[1:]):
        got = C.cast(a, C.c_void_p).value; arr = getattr(pg, k)
        if k in ("edge_count", "edge_rank"):                  # passed through a contiguous copy: compare what the pointer reads
            assert (C.cast(a, C.POINTER(C.c_int32))[0:arr.size] == arr.tolist()), k
        else:
            assert got == arr.ctypes.data, k
    assert set(A.DecompBatch._OMITTABLE) <= set(names)
