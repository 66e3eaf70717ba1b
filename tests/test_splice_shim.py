"""Substitution (include/pire_hip/batch_runner.hpp), compiled against the UNMODIFIED reference headers
(tests/cpp/splice_shim_test.cpp) the way tests/test_search_all_shim.py compiles its program, and run without a GPU: what is
decided before a device is touched -- refusals rethrown as Pire::Error with pire_hip_search_lines_splice in them, empty buffers,
an accessor without a buffer throws, the pieces changed between two fetches.
(What the class answers on a device is tests/test_splice.py's, through the same C entry point.)"""
import os
import re
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "splice_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_splice_shim_compiles_against_reference_headers_and_runs_without_a_device():
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("splice_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(splice shim" in r.stdout


def _calls(body):
    return set(re.findall(r"\b(pire_hip_[a-z_]+)\s*\(", body))


def test_the_recorded_calls_are_untouched_by_construction():
    """Substitution is a class of its own behind MatchFinder: it names the one new entry point it calls and no other
    C call that the classes in front of it do not name already, and SearchBatchRunner -- whose calls
    tests/cpp/shim_calls.expected.txt records -- names neither of the new ones"""
    with open(os.path.join(ROOT, "include", "pire_hip", "batch_runner.hpp")) as f:
        src = f.read()
    at_runner, at_finder, at_sub = src.index("class SearchBatchRunner {"), src.index("class MatchFinder {"), src.index("class Substitution {")
    assert at_runner < at_finder < at_sub
    runner, finder = src[at_runner:at_finder], src[at_finder:at_sub]
    sub = src[at_sub:src.index("}  // namespace Hip")]
    assert "splice" not in runner and "Substitution" not in runner and "splice" not in finder.split("/*")[0]
    new = {"pire_hip_splice", "pire_hip_search_lines_splice"}
    assert _calls(sub) - _calls(src[:at_sub]) <= new and "pire_hip_search_lines_splice" in _calls(sub)
    assert not new & _calls(src[:at_sub])
    for name in ("With(", "Wrap(", "Delete()", "FirstOnly(", "RunLines(", "Text()", "Bytes()", "MatchCount()", "LineCount()", "GrowAndRetry("):
        assert name in sub, name
    assert "explicit Substitution(const MatchFinder& find)" in sub
