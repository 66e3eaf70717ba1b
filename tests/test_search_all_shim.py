"""SearchBatchRunner::All() and Rows() (include/pire_hip/batch_runner.hpp), compiled against the UNMODIFIED reference headers
(tests/cpp/search_all_shim_test.cpp) the way tests/test_search_shim.py compiles its program, and run without a GPU: what is
decided before a device is touched -- refusals rethrown as Pire::Error with the list form's entry point in them, empty batches,
Rows() behind RunLines() or without All() throws, Select() is the default of a new batch.
(What the runner answers on a device is tests/test_search_all.py's, through the same C entry points.)"""
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "search_all_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_search_all_shim_compiles_against_reference_headers_and_runs_without_a_device():
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("search_all_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(search_all shim" in r.stdout


def test_the_list_form_is_named_by_all_alone():
    """a program that never calls All() links neither of the list form's entry points: the calls that tests/test_shim_calls.py
    traces stay what they are"""
    with open(os.path.join(ROOT, "include", "pire_hip", "batch_runner.hpp")) as f:
        src = f.read()
    body = src[src.index("class SearchBatchRunner {"):src.index("class MatchFinder {")]
    assert body.count("pire_hip_search_all_lines_gather") == 1 and "All() { return SetAll(&SearchBatchRunner::FetchAll, pire_hip_search_all_lines_gather)" in body
    fetch_all = body[body.index("void FetchAll()"):body.index("void FetchHits()")]
    assert body.count("pire_hip_search_all(") == 1 and "pire_hip_search_all(" in fetch_all
