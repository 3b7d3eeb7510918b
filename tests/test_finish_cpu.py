"""CPU tier of ald_batch_finish: the Python surface is there and refuses to compute without a device like every other call, and the
C++ adapter test of gpu_scallop_batch::flush_on_device (tests/host_adapter/finish_test.cc) compiles as C++11 against the header and the
in-tree library without a warning.  (tests/test_abi_cpu.py checks that the new entry points are exported and nothing else is.)"""
import ctypes as C
import os
import subprocess

import pytest

import aletsch_amd as A
import common


def test_finish_surface_and_no_device():
    lib = A.load_library()
    for name in ("ald_batch_finish", "ald_batch_export_status", "ald_batch_last_finish_ms"):
        assert hasattr(lib, name), name
    assert lib.ald_batch_finish.argtypes == [C.c_void_p]
    assert len(lib.ald_batch_export_status.argtypes) == 4 and len(lib.ald_batch_last_finish_ms.argtypes) == 4
    for name in ("finish", "status_arrays", "last_finish_ms"):
        assert callable(getattr(A.DecompBatch, name)), name
    # a NULL batch is refused, not dereferenced
    assert lib.ald_batch_finish(None) == -1 and lib.ald_batch_export_status(None, None, None, None) == -1 and lib.ald_batch_last_finish_ms(None, None, None, None) == -1
    import torch
    if torch.cuda.is_available():
        return                                                       # the GPU tier covers the rest (tests/test_finish_gpu.py)
    with pytest.raises(A.DecompError) as e:                          # no device: no batch to finish -- ALD_ERR_NO_DEVICE at creation, as for every other call
        with A.DecompBatch(0) as b:
            b.finish()
    assert e.value.code == -2


def test_flush_on_device_adapter_compiles_as_cxx11():
    ROOT = common.ROOT
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    out = os.path.join(ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "host_adapter", "finish_test.cc"), "-o", os.path.join(out, "finish_test_cpu_check"),
                        "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
