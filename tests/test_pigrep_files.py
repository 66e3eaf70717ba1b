"""examples/pigrep_hip.cpp on several files: it reads them all into one buffer (Pire::Hip::FileSet), makes ONE call
(BatchRunner::RunLines().Files()) and takes the name in front of every hit from the device's answer.  On 1, 2 and 40 files --
an empty one, one without a final newline followed by another, `-` in the middle fed from stdin -- it must print what the
reference's own pigrep prints, byte for byte.  A guard: the output is what it was when every file was a call of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "bin")

pytestmark = pytest.mark.gpu


def run(binary, args, files, stdin=None):
    r = subprocess.run([os.path.join(BIN, binary)] + args + files, cwd=ROOT, input=stdin, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stdout, r.stderr


STDIN = b"from stdin needle-8\nnothing here\nlast line of stdin needle-9, no newline"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not (os.path.exists(os.path.join(BIN, "pigrep_hip")) and os.path.exists(os.path.join(BIN, "pigrep_ref"))):
        pytest.skip("oracle/_ref/bin was not built (needs the reference tree at build time)")
    d = tmp_path_factory.mktemp("pigrep_files")
    texts = []
    for k in range(40):
        lines = [b"file %d line %d%s" % (k, i, b" needle-%d" % (i % 10) if (i * 7 + k) % 5 == 0 else b"") for i in range(k % 7 + (k % 3 == 0))]
        texts.append(b"\n".join(lines) + (b"\n" if lines and k % 4 else b""))
    texts[3] = b""                                             # an empty file
    texts[4] = b"alpha needle-1\nbeta\ngamma needle-2"         # no final newline, and another file behind it
    texts[5] = b"needle-3 opens the next file\n\n"
    texts[6] = b"\n"                                           # one empty line
    assert not texts[7] and texts[8] and not texts[8].endswith(b"\n") and texts[39].endswith(b"\n")
    paths = []
    for k, text in enumerate(texts):
        p = d / ("f%02d.txt" % k)
        p.write_bytes(text)
        paths.append(str(p))
    return paths


PATTERNS = [["needle-[0-9]"], ["^$"], ["-i", "LINE 2|GAMMA"], ["e$"]]


@pytest.mark.parametrize("args", PATTERNS, ids=lambda a: " ".join(a))
def test_one_two_and_forty_files_print_what_the_reference_prints(files, args):
    selected = 0
    for names, stdin in (([files[4]], None), ([files[3]], None), (["-"], STDIN), ([files[4], files[5]], None), ([files[3], files[6]], None),
                         ([files[4], "-", files[5]], STDIN), (files, None), (files[:20] + ["-"] + files[20:], STDIN)):
        want = run("pigrep_ref", args, names, stdin)
        got = run("pigrep_hip", args, names, stdin)
        assert want[0] == 0 and got[0] == 0, (names, got[2][-2000:])
        assert got[1] == want[1], names
        selected += len(want[1])
    assert selected, "the pattern selects nothing in any file: it does not test anything"


def test_a_file_that_cannot_be_opened_ends_the_run_behind_the_hits_in_front_of_it(files):
    names = [files[4], files[5], os.path.join(os.path.dirname(files[0]), "missing.txt"), files[8]]
    want = run("pigrep_ref", ["needle-[0-9]"], names)
    got = run("pigrep_hip", ["needle-[0-9]"], names)
    assert want[0] != 0 and got[0] != 0 and b"cannot open file" in got[2]
    assert got[1] == want[1] and want[1].count(b"\n") == 3
