"""SlowCaptureBatchRunner (include/pire_hip/batch_runner.hpp), compiled against the UNMODIFIED reference headers
(tests/cpp/slow_capture_shim_test.cpp) the way tests/test_combine_shim.py compiles its program, and run without a GPU: it checks
what is decided before a device is touched -- construction from a Pire::SlowCapturingScanner, refusals rethrown as Pire::Error,
empty batches and buffers, the accessors before Run() / RunLines().  (What the calls answer on a device is
tests/test_slow_capture.py's, through the same C entry points.)"""
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(REF_DIR, "bin", "slow_capture_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_slow_capture_shim_compiles_against_reference_headers_and_runs_without_a_device():
    """tests/cpp/slow_capture_shim_test.cpp with the flags oracle/Makefile gives tests/cpp/shim_test.cpp, next to it in oracle/_ref/bin"""
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("slow_capture_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(slow capture shim" in r.stdout
