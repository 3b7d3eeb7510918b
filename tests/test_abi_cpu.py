"""CPU tier: the C-ABI library loads, exports every symbol include/aletsch_decomp.h declares, and refuses to compute
without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

import aletsch_amd as A
import common


def _declared_symbols():
    txt = open(os.path.join(common.ROOT, "include", "aletsch_decomp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ald_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    lib = A.load_library()
    names = _declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/aletsch_decomp.h but not exported"


def test_library_exports_nothing_else():
    """the converse: built with -fvisibility=hidden, the library's dynamic symbol table holds no `ald_*` function the header does not
    declare (round 2 leaked the per-class launchers and occupancy helpers) and no C++ internals of the host code"""
    out = os.popen(f"nm -D --defined-only {A.library_path()}").read()
    exported = sorted(set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-2] in ("T", "W", "V", "B", "D")))
    declared = set(_declared_symbols())
    extra = [n for n in exported if n.startswith("ald_") and n not in declared]
    assert not extra, extra
    host_internals = [n for n in exported if n.startswith("_Z") and ("HostBatch" in n or "ald_batch" in n or "transcript_sink" in n)]
    assert not host_internals, host_internals[:5]


def test_version_and_defaults():
    lib = A.load_library()
    assert b"gfx950" in lib.ald_version()
    p = A.default_params()
    assert list(p.max_decompose_error_ratio) == [0.30, 0.0, 1.10, 1.10, 0.75, 0.30, 0.0, 1.00]      # util/parameters.cc:85-92
    assert p.min_guaranteed_edge_weight == 0.01 and p.min_transcript_coverage == 2.0 and p.max_num_exons == 10000


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    pg = A.synth(seed=1, n_graphs=2, v_min=8, v_max=8, fixed_edges=16)
    with pytest.raises(A.DecompError) as e:
        A.decompose(pg)
    assert e.value.code == -2                                        # ALD_ERR_NO_DEVICE
    assert A.load_library().ald_subsetsum_batch(0, 0, None, None, None, None, None, None, None, None, None, None, None) == -2


def test_product_package_never_touches_the_oracle():
    """the product path must not import / load anything under oracle/ or the emulation"""
    pkg = os.path.join(common.ROOT, "aletsch_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "liboracle" not in txt and "kernel_emu" not in txt.replace("tests/kernel_emu", "") or f in ("decomp_device.h", "decomp_device_rows.h", "decomp_common.h", "host_pack.h"), (dp, f)
                assert "scallop_oracle" not in txt, (dp, f)
    out = os.popen(f"nm -D {A.library_path()}").read()
    assert "ora_" not in out and "emu_run" not in out


def test_synth_is_deterministic_and_well_formed():
    import numpy as np
    a = A.synth(seed=1002, n_graphs=50, v_min=64, v_max=64, fixed_edges=256)
    b = A.synth(seed=1002, n_graphs=50, v_min=64, v_max=64, fixed_edges=256)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("edge_target", "edge_weight", "vertex_offset", "vertex_lpos"))
    assert (a.g_nv == 64).all() and (a.g_ne == 256).all()
    o = a.graph_slices()
    for g in range(a.n):
        vo = a.vertex_offset[o["vo"][g]:o["vo"][g] + 65]; t = a.edge_target[o["e"][g]:o["e"][g] + 256]
        src = np.repeat(np.arange(64), np.diff(vo))
        assert (t > src).all() and not ((src == 0) & (t == 63)).any()
        indeg = np.bincount(t, minlength=64); outdeg = np.diff(vo)
        assert (indeg[1:63] >= 1).all() and (outdeg[1:63] >= 1).all()


def test_host_adapters_compile_as_cxx11_against_the_header():
    """The reference builds with -std=c++11: both adapter programs (gpu_scallop.hpp, gpu_dispatch.hpp over include/aletsch_decomp.h,
    instantiated with mock types carrying the reference's member names) must compile and link against the in-tree library without a
    warning.  They are RUN by the GPU tier (tests/test_gpu_adapter.py); here only the build is checked."""
    import subprocess
    ROOT = common.ROOT
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    out = os.path.join(ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    for src in ("adapter_test.cc", "dispatch_test.cc"):
        r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host_adapter", src), "-o", os.path.join(out, src[:-3] + "_cpu_check"),
                            "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_dispatcher_conversion_matches_the_two_step_form():
    """aletsch::packed_chunk::append_graph (what a submitting thread of gpu_assembly_queue runs: one walk over gr.edges(), counting sort
    into CSR rows, the reference's heap objects asked for ahead of the walks) must fill a chunk exactly as stage_graph + append do --
    random DAGs in random creation order, parallel edges, 0 / 1 / several samples, abundances without their sample, phasing nodes.
    Host code only (no GPU); built with ASan + UBSan (tests/host_adapter/convert_test.cc)."""
    import subprocess
    ROOT = common.ROOT
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    out = os.path.join(ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "convert_test")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_adapter", "convert_test.cc"), "-o", exe,
                        "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "400"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_spill_audit_recognises_the_pattern():
    """tools/isa_spill_audit.py on a cut of the assembly that faulted in round 4 (four spills inside the mark-clearing region of narrowed EXEC,
    reloaded under full EXEC) and on the harmless shapes beside it (spills behind the widening s_or_b64, a spill / reload pair inside one region, a
    value defined inside the region)."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "isa_spill_audit.py"), os.path.join(common.ROOT, "tests", "golden", "isa_spill_in_narrowed_exec.s")], capture_output=True, text=True)
    assert r.returncode == 1, r.stdout
    flagged = [ln for ln in r.stdout.splitlines() if "is spilled at line" in ln or "are spilled at line" in ln]
    assert len(flagged) == 4 and all("ald_decomp_kernel_c12:" in ln for ln in flagged), r.stdout


def test_no_vgpr_spill_inside_a_region_of_narrowed_exec():
    """Round 4's memory fault was the compiler's: the register allocator had put VGPR spills inside a region of narrowed EXEC, so that the lanes
    inactive there lost their values at the reload (aletsch_amd/csrc/decomp_device.h: ev_clear_marks).  Nothing in the source forbids the next
    build from doing it elsewhere, so the device assembly of EVERY kernel of the product build (`make isa`, hipcc cross-compiles without a GPU) is
    searched for the pattern."""
    import glob, shutil, subprocess, sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    subprocess.run(["make", "-C", os.path.join(common.ROOT, "aletsch_amd", "csrc"), "-j8", "isa"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = sorted(glob.glob(os.path.join(common.ROOT, "build", "csrc", "isa", "*.s")))
    assert len(files) == 28, files
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "isa_spill_audit.py"), *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
