"""TokenFinder and LexBatchRunner (include/pire_hip/batch_runner.hpp), compiled against the UNMODIFIED reference headers
(tests/cpp/lex_shim_test.cpp) the way tests/test_search_all_shim.py compiles its program, and run without a GPU: TokenFinder's two
scanners, built from the regexps' Fsms, Save() byte for byte what the reference wrote into tests/golden/lex -- the Glue of the
regexps in order (option n) and `((re_0)|(re_1)|...).*` (options nr) --; and what is decided before a device is touched: refusals
rethrown as Pire::Error, empty batches, Labels() / Masks() / Rows() before a Run() throw.
(What the runner answers on a device is tests/test_lex.py's, through the same C entry points.)"""
import json
import os
import subprocess

import pytest

from oracle import binding as ob
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "lex_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))
SHIM_SETS = ("lexer3", "kw", "alt3", "ipnum", "r64")


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present: nothing to compile against")
def test_lex_shim_compiles_against_reference_headers_and_runs_without_a_device(tmp_path):
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("lex_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    with open(os.path.join(H.GOLDEN, "lex", "cases.json")) as f:
        sets = {c["name"]: c for c in json.load(f)["sets"]}
    listing = tmp_path / "sets.txt"
    with open(listing, "w") as f:
        for name in SHIM_SETS:
            assert not any("\t" in p or "\n" in p for p in sets[name]["patterns"])
            f.write("\t".join([name] + sets[name]["patterns"]) + "\n")
    r = subprocess.run([BIN, str(listing), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(lex shim" in r.stdout
    for name in SHIM_SETS:                # Save() of both scanners, byte for byte what the reference wrote
        for form, key in (("n", "fwd"), ("nr", "rev")):
            with open(tmp_path / ("%s.%s.blob" % (name, form)), "rb") as f:
                got = f.read()
            assert got == H.load_blob(os.path.join("lex", sets[name][key])), (name, form, len(got))


def test_the_runner_names_the_two_entry_points_and_grows_as_fetch_all_does():
    with open(os.path.join(ROOT, "include", "pire_hip", "batch_runner.hpp")) as f:
        src = f.read()
    body = src[src.index("class LexBatchRunner {"):src.index("class TokenFinder {")]
    assert body.count("pire_hip_lex(") == 1 and body.count("pire_hip_lex_lines_gather(") == 2
    assert body.count("GrowAndRetry(") == 2 and "m_form == kLines ? m_len / 64 + 1024 : m_n" in body
    finder = src[src.index("class TokenFinder {"):]
    assert "Pire::Scanner::Glue(" in finder and ".Reverse().Compile<Pire::Scanner>()" in finder and "glued.Empty()" in finder
