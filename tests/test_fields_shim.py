"""BatchRunner::RunLinesField (include/pire_hip/batch_runner.hpp) against the host loop it replaces, compiled against the
UNMODIFIED reference headers (tests/cpp/fields_shim_test.cpp), the way tests/test_shim_cpp.py handles shim_test.cpp."""
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(REF_DIR, "bin", "fields_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present (GPU box): the prebuilt binary is used there")
def test_fields_shim_compiles_against_reference_headers():
    """tests/cpp/fields_shim_test.cpp with the flags oracle/Makefile gives tests/cpp/shim_test.cpp, next to it in oracle/_ref/bin"""
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("fields_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_fields_shim_agrees_with_the_host_loop_on_gpu():
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/bin/fields_shim_test was not built (needs the reference tree at build time)")
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(fields shim" in r.stdout
