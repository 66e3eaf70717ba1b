"""Which C calls include/pire_hip/batch_runner.hpp makes: tests/cpp/shim_calls_test.cpp walks every runner through its forms
against a recording stand-in for the library (tests/cpp/recording_hip.cpp; no library, no device), and the trace it writes is
byte for byte tests/cpp/shim_calls.expected.txt.  A change of the header that changes a call, its order or an argument shows
here as a diff of two text files; one that is meant re-records the file and says so.

The same build traces the header of another checkout: `make -B -C tests/cpp shim_calls_test SHIMINC=<its include directory>`."""
import difflib
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "shim_calls_test")
EXPECTED = os.path.join(ROOT, "tests", "cpp", "shim_calls.expected.txt")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "extra.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_the_shim_makes_the_recorded_c_calls(tmp_path):
    ob.build()
    r = H.make_shim_program("shim_calls_test")
    assert r.returncode == 0, r.stdout[-3000:]
    trace = tmp_path / "shim_calls.txt"
    r = subprocess.run([BIN, str(trace)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(shim calls" in r.stdout
    with open(EXPECTED) as f:
        want = f.read()
    got = trace.read_text()
    assert got == want, "".join(list(difflib.unified_diff(want.splitlines(True), got.splitlines(True), "expected", "traced"))[:80])
