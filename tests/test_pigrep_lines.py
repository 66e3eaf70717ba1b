"""examples/pigrep_hip.cpp reads a file as it is and leaves the cutting into lines to the GPU (BatchRunner::RunLines): on
files that try the edges of that -- a last line without a newline, CR LF, empty lines, a line longer than several tiles of
the split pass, an empty file, several files -- it must print what the reference's own pigrep prints, byte for byte."""
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


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not (os.path.exists(os.path.join(BIN, "pigrep_hip")) and os.path.exists(os.path.join(BIN, "pigrep_ref"))):
        pytest.skip("oracle/_ref/bin was not built (needs the reference tree at build time)")
    d = tmp_path_factory.mktemp("pigrep_lines")
    long_line = (b"lorem ipsum needle-7 dolor " * 2600)[:70000]
    assert len(long_line) == 70000
    texts = {
        "no_final_newline.txt": b"alpha needle-1\nbeta\ngamma needle-2",
        "crlf.txt": b"alpha needle-1\r\nbeta\r\n\r\nneedle-3 gamma\r\nend\r\n",
        "empty_lines.txt": b"\n\nneedle-4\n\n\n\nx\n\n",
        "long_line.txt": b"short needle-5\n" + long_line + b"\nafter the long line needle-6\n" + b"y" * 70000 + b"\n",
        "empty.txt": b"",
        "only_newlines.txt": b"\n" * 40,
    }
    paths = {}
    for name, text in texts.items():
        p = d / name
        p.write_bytes(text)
        paths[name] = str(p)
    return paths


PATTERNS = [["needle-[0-9]"], ["^$"], ["a$"], ["-i", "GAMMA|END"], ["\\r$"], ["^[^\\r]*$"], ["y{100}$"]]


@pytest.mark.parametrize("args", PATTERNS, ids=lambda a: " ".join(a))
def test_each_file_alone(files, args):
    selected = 0
    for name, path in sorted(files.items()):
        want = run("pigrep_ref", args, [path])
        got = run("pigrep_hip", args, [path])
        assert got[0] == 0, (name, got[2][-2000:])
        assert got[1] == want[1], name
        selected += len(want[1])
    assert selected, "the pattern selects nothing in any file: it does not test anything"


@pytest.mark.parametrize("args", PATTERNS[:4], ids=lambda a: " ".join(a))
def test_several_files_and_stdin(files, args):
    order = [files[k] for k in ("crlf.txt", "empty.txt", "no_final_newline.txt", "long_line.txt", "empty_lines.txt", "only_newlines.txt")]
    want = run("pigrep_ref", args, order)
    got = run("pigrep_hip", args, order)
    assert got[0] == 0, got[2][-2000:]
    assert got[1] == want[1] and want[1]
    with open(files["no_final_newline.txt"], "rb") as f:
        text = f.read()
    want = run("pigrep_ref", args, [files["crlf.txt"], "-"], stdin=text)
    got = run("pigrep_hip", args, [files["crlf.txt"], "-"], stdin=text)
    assert got[0] == 0 and got[1] == want[1]
