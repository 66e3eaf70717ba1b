"""SearchBatchRunner and MatchFinder (include/pire_hip/batch_runner.hpp), compiled against the UNMODIFIED reference headers
(tests/cpp/search_shim_test.cpp) the way tests/test_affix_shim.py compiles its program, and run without a GPU: MatchFinder's two
scanners, built from one Fsm, Save() byte for byte what the reference wrote into tests/golden/search for `re` (option n) and
`(re).*` (options nr); and what is decided before a device is touched -- refusals rethrown as Pire::Error, empty batches.
(What the runner answers on a device is tests/test_search.py's, through the same C entry points.)"""
import json
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(REF_DIR, "bin", "search_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_search_shim_compiles_against_reference_headers_and_runs_without_a_device(tmp_path):
    """tests/cpp/search_shim_test.cpp with the flags oracle/Makefile gives tests/cpp/shim_test.cpp, next to it in oracle/_ref/bin"""
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("search_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    with open(os.path.join(H.GOLDEN, "search", "cases.json")) as f:
        pairs = json.load(f)["pairs"]
    patterns = tmp_path / "patterns.txt"
    with open(patterns, "w") as f:
        for c in pairs:
            pattern = c["pattern"] if c["pattern"] is not None else "|".join(c["words"])
            assert "\t" not in pattern and "\n" not in pattern
            f.write("%s\t%s\n" % (c["name"], pattern))
    r = subprocess.run([BIN, str(patterns), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(search shim" in r.stdout
    assert {"num", "stamp", "alt", "blanks_star", "arrow", "gap", "eol", "bol", "words"} <= {c["name"] for c in pairs}
    for c in pairs:                       # Save() of both scanners, byte for byte what the reference wrote
        for form, key in (("n", "fwd"), ("nr", "rev")):
            with open(tmp_path / ("%s.%s.blob" % (c["name"], form)), "rb") as f:
                got = f.read()
            assert got == H.load_blob(os.path.join("search", c[key])), (c["name"], form, len(got))
