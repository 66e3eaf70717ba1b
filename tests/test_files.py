"""pire_hip_files and the two lines forms on top of it: from a hit list and file boundaries to hits by file -- grep -c / -l /
-L / -H -n over many files laid end to end in one buffer -- on the device (files.hip).

Exact equality everywhere.  The expected values come from `model_files` and `model_file_lines` -- the formulas of
include/pire_hip.h written down with numpy, held against a hand-written truth table and, where there is one, against the
system's grep --, applied, where a scan is involved, to what the C oracle says of every line and to Python's own split (the
buffers, tables and verdicts are tests/test_context.py's, computed once for both files).  Nothing expected comes from the
library.  Every output of a GPU call sits between poisoned guard bytes and is compared bytewise, what the call had no business
writing included."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pire_amd
from pire_amd import binding as pb
from tests import test_context as TC

ROOT = TC.ROOT
POISON, GUARD, EINVAL, BE, ZERO = TC.POISON, TC.GUARD, TC.EINVAL, TC.BE, TC.ZERO
u8, u64, one, py_lines, stream_of = TC.u8, TC.u64, TC.one, TC.py_lines, TC.stream_of
gpu = pytest.mark.gpu
NAMES = ("pire_hip_files", "pire_hip_run_lines_files_select", "pire_hip_slow_lines_files_select")
LINES_FORMS = NAMES[1:]
WITHOUT = pb.FILES_WITHOUT


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_files(hits, bounds, without=False):
    """include/pire_hip.h: first[f] = the hits in front of bounds[f]; the file of a hit = the one f with bounds[f] <= hit <
    bounds[f + 1] (the LAST f with bounds[f] <= hit: behind a run of empty files, the one that holds the line); its line = hit -
    bounds[f]; listed: the f with a hit, or, without, those with none."""
    h, b = np.asarray(hits, dtype=np.int64), np.asarray(bounds, dtype=np.int64)
    first = np.searchsorted(h, b, side="left")
    counts = np.diff(first)
    hit_file = np.searchsorted(b, h, side="right") - 1
    listed = np.flatnonzero((counts > 0) != bool(without))
    return {"first": first.astype(np.uint64), "counts": counts, "hit_file": hit_file.astype(np.uint64),
            "hit_line": (h - b[hit_file]).astype(np.uint64) if h.size else np.zeros(0, np.uint64), "files": listed.astype(np.uint64),
            "count": int(listed.size)}


def model_file_lines(raw, delim, file_bytes):
    """a line belongs to the file that holds its first byte: file_lines[f] = the lines that begin in front of file_bytes[f];
    straddles = the boundaries strictly inside the buffer, not the first, whose byte in front is not the delimiter"""
    _, spans = py_lines(raw, bytes([delim]))
    fb = np.asarray(file_bytes, dtype=np.int64)
    lines = np.searchsorted(spans[:, 0].astype(np.int64), fb, side="left")
    raw = bytes(raw)
    straddles = sum(1 for f in range(1, len(fb) - 1) if 0 < fb[f] < len(raw) and raw[fb[f] - 1] != delim)
    return lines.astype(np.uint64), straddles


# (hits, bounds, without) -> (first, hit_file, hit_line, files)
TRUTH = [
    (([], [0], False), ([0], [], [], [])),
    (([], [0, 0, 0], True), ([0, 0, 0], [], [], [0, 1])),
    (([], [0, 0, 0], False), ([0, 0, 0], [], [], [])),
    (([0, 4], [0, 5], False), ([0, 2], [0, 0], [0, 4], [0])),
    # empty files in front, between and behind; a hit on the first and on the last line of a file
    (([2, 4, 5, 9], [0, 0, 0, 2, 5, 5, 5, 10, 10], False), ([0, 0, 0, 0, 2, 2, 2, 4, 4], [3, 3, 6, 6], [0, 2, 0, 4], [3, 6])),
    (([2, 4, 5, 9], [0, 0, 0, 2, 5, 5, 5, 10, 10], True), ([0, 0, 0, 0, 2, 2, 2, 4, 4], [3, 3, 6, 6], [0, 2, 0, 4], [0, 1, 2, 4, 5, 7])),
    (([0, 1, 2], [0, 1, 2, 3], False), ([0, 1, 2, 3], [0, 1, 2], [0, 0, 0], [0, 1, 2])),          # one line a file
    (([3], [0, 3, 3, 3, 6], False), ([0, 0, 0, 0, 1], [3], [0], [3])),                           # the LAST f with bounds[f] <= hit
    (([2], [0, 3, 3, 3, 6], True), ([0, 1, 1, 1, 1], [0], [2], [1, 2, 3])),
]


def test_the_model_against_a_hand_written_truth_table():
    for (hits, bounds, without), (first, hit_file, hit_line, files) in TRUTH:
        got = model_files(hits, bounds, without)
        assert got["first"].tolist() == first and got["hit_file"].tolist() == hit_file, (hits, bounds)
        assert got["hit_line"].tolist() == hit_line and got["files"].tolist() == files and got["count"] == len(files), (hits, bounds, without)
    # a boundary inside line 1 ("cd"): the line is the first file's; a boundary behind a delimiter straddles nothing
    lines, straddles = model_file_lines(b"ab\ncd\nef", 10, [0, 4, 6, 8])
    assert lines.tolist() == [0, 2, 2, 3] and straddles == 1
    lines, straddles = model_file_lines(b"ab\n\ncd\n", 10, [0, 0, 3, 4, 7, 7])
    assert lines.tolist() == [0, 0, 1, 2, 3, 3] and straddles == 0


def file_set(texts, delim=b"\n"):
    """Pire::Hip::FileSet: the files end to end, the delimiter behind a non-empty file that lacks one; (raw, file_bytes)"""
    raw, fb = b"", [0]
    for t in texts:
        raw += t + (delim if t and not t.endswith(delim) else b"")
        fb.append(len(raw))
    return raw, fb


def _grep():
    exe = shutil.which("grep")
    if not exe:
        return None
    r = subprocess.run([exe, "-L", "x", "-"], input=b"y\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return exe if r.stdout == b"(standard input)\n" else None


@pytest.mark.skipif(_grep() is None, reason="no grep that accepts -L")
def test_the_model_against_grep(tmp_path):
    """grep -c, -l, -L and -Hn on temporary files written from a FileSet-style concatenation"""
    exe = _grep()
    texts = [b"", b"needle 1\nhay\nneedle 2\n", b"hay\nhay", b"", b"\n", b"hay\nneedle at the end", b"needle alone\n", b"needle\n\nhay\nneedle\n", b""]
    raw, fb = file_set(texts)
    parts, _ = py_lines(raw)
    hits = [i for i, s in enumerate(parts) if b"needle" in s]
    file_lines, straddles = model_file_lines(raw, 10, fb)
    assert straddles == 0 and file_lines[-1] == len(parts)
    names = []
    for k, t in enumerate(texts):
        (tmp_path / ("f%d" % k)).write_bytes(raw[fb[k]:fb[k + 1]])
        names.append("f%d" % k)

    def grep(*opts):
        return subprocess.run([exe] + list(opts) + ["needle"] + names, cwd=str(tmp_path), stdout=subprocess.PIPE).stdout.decode().splitlines()

    exp = model_files(hits, file_lines)
    assert grep("-c") == ["f%d:%d" % (k, c) for k, c in enumerate(exp["counts"].tolist())]
    assert grep("-l") == ["f%d" % f for f in exp["files"].tolist()]
    assert grep("-L") == ["f%d" % f for f in model_files(hits, file_lines, True)["files"].tolist()]
    assert grep("-Hn") == ["f%d:%d:%s" % (f, i + 1, parts[h].decode()) for h, f, i in zip(hits, exp["hit_file"].tolist(), exp["hit_line"].tolist())]
    assert len(hits) == 6 and exp["count"] == 4


# ---- CPU: the surface and what it refuses -----------------------------------------------------------------------------------------

def test_the_library_exports_the_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        src = f.read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in {n for n, _, _ in pb.ABI}
        assert re.search(r"\nint %s\(" % name, src), name
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    assert int(re.search(r"#define PIRE_HIP_ABI_VERSION (\d+)", src).group(1)) == 6
    assert re.search(r"#define PIRE_HIP_FILES_WITHOUT +1u", src) and pb.FILES_WITHOUT == 1
    assert "pire_hip_files" not in " ".join(pb.selftested_kernels())


def _guarded():
    return {k: np.full(256, POISON, dtype=np.uint8) for k in ("hits", "spans", "first", "hit_file", "hit_line", "files", "lines")}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_files_refuses_before_any_device_is_touched():
    L = pb.lib()
    hits, bounds = u64([1, 4, 6]), u64([0, 2, 2, 8])
    bufs, cnt = _guarded(), C.c_uint64(77)
    h, b, c = hits.ctypes.data, bounds.ctypes.data, C.addressof(cnt)
    fi, hf, hl, fl = (bufs[k].ctypes.data for k in ("first", "hit_file", "hit_line", "files"))
    # (hits, hit_cap, n, bounds, files, file_mode, out_files, file_cap, out_file_count)
    cases = {
        "null out_file_count": (h, 3, 8, b, 3, 0, fl, 4, None),
        "hit_cap > 0 with null hits": (None, 3, 8, b, 3, 0, fl, 4, c),
        "files > 0 with null bounds": (h, 3, 8, None, 3, 0, fl, 4, c),
        "file_cap > 0 with null out_files": (h, 3, 8, b, 3, 0, None, 4, c),
        "unknown file_mode": (h, 3, 8, b, 3, 2, fl, 4, c),
        "files == 0 with n > 0": (h, 3, 8, b, 0, 0, fl, 4, c),
        "2^32 lines or more": (h, 3, 1 << 32, b, 3, 0, fl, 4, c),
        "2^32 hits or more": (h, 1 << 32, 8, b, 3, 0, fl, 4, c),
        "2^32 files or more": (h, 3, 8, b, 1 << 32, 0, fl, 4, c),
    }
    for what, (a_h, cap, n, a_b, files, mode, a_fl, fcap, a_c) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_files(a_h, None, cap, n, a_b, files, mode, flags, fi, hf, hl, a_fl, fcap, a_c, None) == EINVAL, what
            msg = L.pire_hip_last_error().decode()
            assert what in msg and msg.startswith("pire_hip_files: "), (what, msg)
    # host pointers: the list and the bounds themselves, before anything is written
    for what, bad_h, bad_b, n in (("strictly ascending", [4, 1, 6], [0, 2, 2, 8], 8), ("strictly ascending", [1, 1, 6], [0, 2, 2, 8], 8),
                                  ("hit out of range", [1, 4, 8], [0, 2, 2, 8], 8), ("bounds must be non-decreasing", [1, 4, 6], [0, 5, 2, 8], 8),
                                  ("bounds[0] != 0", [1, 4, 6], [1, 2, 2, 8], 8), ("bounds[files] != n", [1, 4, 6], [0, 2, 2, 7], 8),
                                  ("bounds[files] != n", [1, 4, 6], [0, 2, 2, 9], 8)):
        bad_h, bad_b = u64(bad_h), u64(bad_b)
        for mode in (0, WITHOUT):
            assert L.pire_hip_files(bad_h.ctypes.data, None, 3, n, bad_b.ctypes.data, 3, mode, 0, fi, hf, hl, fl, 4, c, None) == EINVAL, what
            msg = L.pire_hip_last_error().decode()
            assert what in msg and msg.startswith("pire_hip_files: "), (what, msg)
    assert cnt.value == 77 and _untouched(bufs)
    # no files: zeros, and no device
    for mode in (0, WITHOUT):
        cnt.value = 77
        assert L.pire_hip_files(None, None, 0, 0, None, 0, mode, 0, fi, hf, hl, fl, 4, c, None) == 0, L.pire_hip_last_error()
        assert cnt.value == 0 and bufs["first"].view(np.uint64)[0] == 0 and (bufs["first"][8:] == POISON).all()
        bufs["first"][:8] = POISON
        assert _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="strictly ascending"):   # (the wrappers raise what the library refuses)
        pb.files_host([3, 2], 10, [0, 10])
    with pytest.raises(pb.PireHipError, match="non-decreasing"):
        pb.files_host([2, 3], 10, [0, 7, 5, 10])


def _slow_blob(name):
    return TC._slow_blob(name)


def lines_form(who, table, raw_ptr, size, delim, flags, pick, a_fb, files, mode, a_n, a_hits, a_spans, a_hf, a_hl, cap, a_cnt, a_lines, a_first, a_files,
               fcap, a_fcnt, a_straddles, stream=None):
    """one of the two C calls; pick: want (a pointer) or mode"""
    return getattr(pb.lib(), who)(table, raw_ptr, size, delim, flags, pick, a_fb, files, mode, a_n, a_hits, a_spans, a_hf, a_hl, cap, a_cnt, a_lines,
                                  a_first, a_files, fcap, a_fcnt, a_straddles, stream)


def _tables():
    return {"run": TC.table_of("set_a"), "slow": TC.table_of("slow_a30")}


def test_the_lines_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    text = b"ab" * 20 + b"\nb\n"
    raw = u8(text).copy()
    tables = _tables()
    bufs = _guarded()
    n, cnt, fcnt, straddles = (C.c_uint64(70 + k) for k in range(4))
    good = u64([0, 41, 41, raw.size])
    r, g = raw.ctypes.data, good.ctypes.data
    np_, cp, fp, sp = (C.addressof(v) for v in (n, cnt, fcnt, straddles))
    hi, spn, hf, hl, li, fi, fl = (bufs[k].ctypes.data for k in ("hits", "spans", "hit_file", "hit_line", "lines", "first", "files"))
    for who in LINES_FORMS:
        t = tables["slow" if "slow" in who else "run"]._h
        # (table, raw, size, delim, pick, file_bytes, files, mode, out_line_count, out_hits, out_hit_spans, hit_cap, out_hit_count, out_files,
        #  file_cap, out_file_count, out_straddles)
        ok = (t, r, raw.size, 10, 0, g, 3, 0, np_, hi, spn, 4, cp, fl, 4, fp, sp)

        def but(**kw):
            keys = ("t", "raw", "size", "delim", "pick", "fb", "files", "mode", "n", "hits", "spans", "cap", "cnt", "fl", "fcap", "fcnt", "straddles")
            return tuple(kw.get(k, v) for k, v in zip(keys, ok))

        cases = {
            "null table": but(t=None),
            "delim > 255": but(delim=256),
            "null out_line_count": but(n=None),
            "size > 0 with null raw": but(raw=None),
            "null out_hit_count": but(cnt=None),
            "hit_cap > 0 with null out_hits": but(hits=None, spans=None),
            "out_hit_spans without out_hits": but(hits=None, cap=0),
            "null out_file_count": but(fcnt=None),
            "null out_straddles": but(straddles=None),
            "files > 0 with null file_bytes": but(fb=None),
            "file_cap > 0 with null out_files": but(fl=None),
            "unknown file_mode": but(mode=2),
            "files == 0 with size > 0": but(files=0),
            "2^32 files or more": but(files=1 << 32),
        }
        if "slow" in who:
            cases["unknown mode"] = but(pick=2)
        for what, (a_t, a_r, size, delim, pick, a_fb, files, mode, a_n, a_hi, a_sp, cap, a_c, a_fl, fcap, a_fc, a_st) in cases.items():
            for flags in (3, 3 | pb.FLAG_ON_DEVICE):
                rc = lines_form(who, a_t, a_r, size, delim, flags, pick, a_fb, files, mode, a_n, a_hi, a_sp, hf, hl, cap, a_c, li, fi, a_fl, fcap, a_fc, a_st)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (who, what, rc, msg)
        # host pointers: file_bytes itself
        for what, bad in (("file_bytes must be non-decreasing", [0, 41, 40, raw.size]), ("file_bytes[0] != 0", [1, 41, 41, raw.size]),
                          ("file_bytes[files] != size", [0, 41, 41, raw.size - 1]), ("file_bytes[files] != size", [0, 41, 41, raw.size + 1])):
            bad = u64(bad)
            rc = lines_form(who, t, r, raw.size, 10, 3, 0, bad.ctypes.data, 3, 0, np_, hi, spn, hf, hl, 4, cp, li, fi, fl, 4, fp, sp)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (who, what, rc, msg)
    assert [v.value for v in (n, cnt, fcnt, straddles)] == [70, 71, 72, 73] and _untouched(bufs)
    assert raw.tobytes() == text


def test_empty_host_buffers_answer_zeros_without_a_device():
    tables = _tables()
    zeros = u64([0, 0, 0, 0])
    for who in LINES_FORMS:
        t = tables["slow" if "slow" in who else "run"]._h
        for pick in (0, ZERO) if "slow" in who else (0,):
            for mode, files, fcap in ((0, 3, 4), (WITHOUT, 3, 4), (WITHOUT, 3, 2), (WITHOUT, 0, 0), (0, 0, 0)):
                bufs = _guarded()
                n, cnt, fcnt, straddles = (C.c_uint64(70 + k) for k in range(4))
                rc = lines_form(who, t, None, 0, 10, 3, pick, zeros.ctypes.data if files else None, files, mode, C.addressof(n), bufs["hits"].ctypes.data,
                                bufs["spans"].ctypes.data, bufs["hit_file"].ctypes.data, bufs["hit_line"].ctypes.data, 4, C.addressof(cnt),
                                bufs["lines"].ctypes.data, bufs["first"].ctypes.data, bufs["files"].ctypes.data if fcap else None, fcap,
                                C.addressof(fcnt), C.addressof(straddles))
                assert rc == 0, pb.lib().pire_hip_last_error()
                listed = files if mode else 0
                assert [v.value for v in (n, cnt, fcnt, straddles)] == [0, 0, listed, 0]
                for k in ("lines", "first"):
                    assert (bufs[k][:8 * (files + 1)] == 0).all() and (bufs[k][8 * (files + 1):] == POISON).all()
                    bufs[k][:] = POISON
                m = min(listed, fcap)
                assert bufs["files"][:8 * m].view(np.uint64).tolist() == list(range(m)) and (bufs["files"][8 * m:] == POISON).all()
                bufs["files"][:] = POISON
                assert _untouched(bufs)
    # the wrappers on nothing
    got = tables["run"].run_lines_files_host(b"", [0, 0, 0], without=True)
    assert (got["lines"], got["count"], got["file_count"], got["straddles"]) == (0, 0, 2, 0) and got["files"].tolist() == [0, 1]
    assert got["first"].tolist() == [0, 0, 0] and got["file_lines"].tolist() == [0, 0, 0] and got["hit_file"].size == 0
    got = tables["slow"].lines_files_host(b"", [0], invert=True)
    assert (got["lines"], got["count"], got["file_count"]) == (0, 0, 0) and got["first"].tolist() == [0]


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """files.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "files.hip" in ba.NO_SCRATCH and "files.hip" in ba.UNITS and "files" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bfiles\.hip\b", mk)) == 2                              # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("files.hip")
    assert not fails, fails
    assert len(seen) == 5 and all("File" in k for k in seen), seen                  # bounds, classify, scatter, locate, lines


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "files.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src
    assert "atomic" not in src.lower().replace("no atomics", "").replace("no atomic", "")
    # the shared kernel pair between the bounds and the locate kernel, the shared search and stage; the lines kernel scans its own row
    for shared in ('#include "tile_pass.h"', "TilePass t(", "t.Front(", "t.Classify(", "t.Scan(", "t.Scatter(", "t.Done(", "LaunchTileScan(",
                   "WaveBound<true>(", "LoadU64(", "list.Count(", "list.List(", "list.Back()"):
        assert shared in src, shared
    assert "BlockExclusive" not in src and "asm" not in src                        # (the scan is select.hip's; plain HIP)
    assert src.count("__global__") == 3 and src.count("hipLaunchKernelGGL") == 3   # (bounds, locate, lines)
    assert src.count("hipGetLastError") == 1                                       # (the lines launcher's)
    for copy in ("TileBallot(", "TileRank(", "TileCompaction(", "__shfl", "UnalignedU64", "hipMemcpyDeviceToHost"):
        assert copy not in src, copy
    before = pb.lib().pire_hip_last_kernel()
    assert pb.files_host([], 0, [0])["count"] == 0 and pb.lib().pire_hip_last_kernel() == before


# ---- GPU: the pass alone ---------------------------------------------------------------------------------------------------------

class Bounds:
    """bounds[files + 1] on the host and on the device"""

    def __init__(self, torch, bounds):
        self.np = u64(bounds)
        self.files = len(self.np) - 1
        self.t = torch.as_tensor(self.np.view(np.int64).copy(), device="cuda")

    def ptr(self, device):
        return self.t.data_ptr() if device else self.np.ctypes.data


def run_pass(torch, device, hl, n, bd, exp, what, without=False, hit_count=None, hit_cap=None, file_cap=None, null=()):
    """pire_hip_files, and its outputs against exp -- the model's answer for the k the call was given; null: the outputs left out"""
    files = bd.files
    cap = hl.k if hit_cap is None else hit_cap
    fcap = files if file_cap is None else file_cap
    k = len(exp["hit_file"])
    out = TC.Outs(torch, device, {"count": 8, "first": None if "first" in null else 8 * (files + 1), "hit_file": None if "hit_file" in null else 8 * cap,
                                  "hit_line": None if "hit_line" in null else 8 * cap, "files": None if "files" in null else 8 * fcap,
                                  "k": None if hit_count is None else 8})
    if hit_count is not None:
        if device:
            out.dev["k"][GUARD:GUARD + 8] = torch.as_tensor(one(hit_count).view(np.uint8), device="cuda")
        else:
            out.host["k"][GUARD:GUARD + 8] = one(hit_count).view(np.uint8)
    rc = pb.lib().pire_hip_files(hl.ptr(device) if cap else None, out.ptr("k"), cap, n, bd.ptr(device), files, WITHOUT if without else 0,
                                 pb.FLAG_ON_DEVICE if device else 0, out.ptr("first"), out.ptr("hit_file") if cap else None,
                                 out.ptr("hit_line") if cap else None, out.ptr("files") if fcap else None, 0 if "files" in null else fcap,
                                 out.ptr("count"), stream_of(torch) if device else None)
    assert rc == 0, (what, pb.lib().pire_hip_last_error())
    assert k <= cap
    want = {"count": one(exp["count"]), "first": exp["first"], "hit_file": exp["hit_file"], "hit_line": exp["hit_line"],
            "files": exp["files"][:min(exp["count"], fcap)]}
    if hit_count is not None:
        want["k"] = one(hit_count)
    return out.check(want, what)


SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
FILES = (1, 2, 64, 65, 1024, 1025, 2049)


def hit_lists(n):
    return {"empty": [], "full": np.arange(n), "every 37th": np.arange(0, n, 37), "the first and the last line": sorted({0, n - 1})}


def random_bounds(n, files, seed):
    cuts = np.sort(np.random.RandomState(seed).randint(0, n + 1, size=files - 1))
    return np.concatenate([[0], cuts, [n]])


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_from_host_pointers_and_on_the_device(torch_cuda, n):
    """every hit list against bounds drawn at random for every number of files, both file_modes"""
    torch = torch_cuda
    calls = 0
    lists = [(name, TC.Hits(torch, hits), hits) for name, hits in hit_lists(n).items()]
    for files in FILES:
        bd = Bounds(torch, random_bounds(n, files, 1000 * n + files))
        for k, (name, hl, hits) in enumerate(lists):
            for without in (False, True):
                exp = model_files(hits, bd.np, without)
                for device in (True, False):
                    run_pass(torch, device, hl, n, bd, exp, (n, files, name, without, "device" if device else "host"), without=without)
                    calls += 1
    for name, hl, hits in lists:
        got = hl.dev_room.cpu().numpy()
        assert got[hl.dev_lead:hl.dev_lead + 8 * hl.k].tobytes() == u64(hits).tobytes(), "the list was written to"
        assert (got[:hl.dev_lead] == POISON).all() and (got[hl.dev_lead + 8 * hl.k:] == POISON).all(), "the list's surroundings were written to"
    assert calls == 7 * 4 * 2 * 2


@gpu
def test_no_files_from_host_pointers_and_on_the_device(torch_cuda):
    """files == 0 (and so n == 0, and no hits): a file count of 0 and first[0] = 0, in either mode; no list is touched"""
    torch = torch_cuda
    hl, bd = TC.Hits(torch, []), Bounds(torch, [0])
    assert bd.files == 0
    for without in (False, True):
        exp = model_files([], bd.np, without)
        assert exp["count"] == 0 and exp["first"].tolist() == [0]
        for null in ((), ("first",), ("first", "files")):
            for device in (True, False):
                run_pass(torch, device, hl, 0, bd, exp, (without, null, "device" if device else "host"), without=without, null=null)
    assert bd.t.cpu().numpy().tolist() == [0]


def hand_bounds():
    rng = np.random.RandomState(11)
    return {
        "all lines in the last file behind 1 500 empty ones": (2000, [0] * 1501 + [2000]),
        "all lines in the first file in front of 1 500 empty ones": (2000, [0] + [2000] * 1501),
        "one line a file": (2049, np.arange(2050)),
        "a file that spans three hit tiles": (5000, [0, 100, 4000, 5000]),
        "a file that spans three hit tiles between empty ones": (5000, [0, 0, 100, 100, 100, 4000, 4000, 5000, 5000]),
        "1 500 files inside one hit tile": (5000, np.concatenate([[0], np.sort(rng.randint(1100, 1900, size=1499)), [5000]])),
        "1 500 empty files on one line": (5000, np.concatenate([[0], [1500] * 1499, [5000]])),
    }


@gpu
@pytest.mark.parametrize("case", sorted(hand_bounds()))
def test_bounds_made_by_hand(torch_cuda, case):
    torch = torch_cuda
    n, bounds = hand_bounds()[case]
    bd = Bounds(torch, bounds)
    for name, hits in (("full", np.arange(n)), ("every 3rd", np.arange(0, n, 3)), ("every 37th", np.arange(0, n, 37)), ("around the cuts", sorted(
            {int(h) for b in np.unique(bd.np).tolist() for h in (b - 1, b) if 0 <= h < n}))):
        hl = TC.Hits(torch, hits)
        if name == "full":
            assert hl.k >= 3073 or n < 5000
        for without in (False, True):
            exp = model_files(hits, bd.np, without)
            for device in (True, False):
                run_pass(torch, device, hl, n, bd, exp, (case, name, without, device), without=without)


@gpu
def test_counts_caps_and_k(torch_cuda):
    torch = torch_cuda
    n, files = 2049, 300
    hits = np.flatnonzero(np.random.RandomState(5).randint(0, 40, size=n) == 0)
    hl = TC.Hits(torch, hits)
    bd = Bounds(torch, random_bounds(n, files, 6))
    half = len(hits) // 2
    for without in (False, True):
        exp = model_files(hits, bd.np, without)
        count = exp["count"]
        assert 20 < count < files - 20
        for device in (True, False):
            for fcap in (0, 1, count - 1, count, count + 5):
                run_pass(torch, device, hl, n, bd, exp, ("file_cap", fcap, device), without=without, file_cap=fcap)
            for null in ("first", "hit_file", "hit_line", "files"):
                run_pass(torch, device, hl, n, bd, exp, ("null", null, device), without=without, null=(null,))
            run_pass(torch, device, hl, n, bd, exp, ("counts only", device), without=without, null=("first", "hit_file", "hit_line", "files"))
            # k: *hit_count where it is smaller than hit_cap, hit_cap where it is not, hit_cap where there is no hit_count
            short = model_files(hits[:half], bd.np, without)
            run_pass(torch, device, hl, n, bd, short, ("k = *hit_count", device), without=without, hit_count=half)
            run_pass(torch, device, hl, n, bd, short, ("hit_count > hit_cap", device), without=without, hit_count=len(hits) + 7, hit_cap=half)
            run_pass(torch, device, hl, n, bd, short, ("no hit_count", device), without=without, hit_cap=half)
            none = model_files([], bd.np, without)
            run_pass(torch, device, hl, n, bd, none, ("*hit_count == 0", device), without=without, hit_count=0)
            run_pass(torch, device, hl, n, bd, none, ("hit_cap == 0", device), without=without, hit_cap=0)
    # no files at all, on the device: the count and first[0]
    empty = Bounds(torch, [0])
    for device in (True, False):
        run_pass(torch, device, TC.Hits(torch, []), 0, empty, model_files([], [0]), ("no files", device))
    # the wrappers, and the same input twice: the same bits
    exp = model_files(hits, bd.np)
    w = pb.files_host(hits, n, bd.np, file_cap=5)
    assert w["count"] == exp["count"] and (w["files"] == exp["files"][:5]).all() and (w["first"] == exp["first"]).all()
    assert (w["hit_file"] == exp["hit_file"]).all() and (w["hit_line"] == exp["hit_line"]).all()
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    outs = torch.full((2, 3, n), -1, dtype=torch.int64, device="cuda")     # first, hit_file, hit_line
    listed = torch.full((2, files), -1, dtype=torch.int64, device="cuda")
    for k in range(2):
        pb.files_device(hl.dev, hl.k, n, bd.ptr(True), files, cnt[k:].data_ptr(), out_file_first_ptr=outs[k, 0].data_ptr(),
                        out_hit_file_ptr=outs[k, 1].data_ptr(), out_hit_line_ptr=outs[k, 2].data_ptr(), out_files_ptr=listed[k].data_ptr(),
                        file_cap=files, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [exp["count"]] * 2
    got, got_l = outs.cpu().numpy(), listed.cpu().numpy()
    assert (got[0] == got[1]).all() and (got_l[0] == got_l[1]).all()
    assert (got[0, 0, :files + 1] == exp["first"].astype(np.int64)).all() and (got[0, 1, :hl.k] == exp["hit_file"].astype(np.int64)).all()
    assert (got[0, 2, :hl.k] == exp["hit_line"].astype(np.int64)).all() and (got_l[0, :exp["count"]] == exp["files"].astype(np.int64)).all()


@gpu
def test_host_pointers_refuse_bad_lists_and_bad_bounds_and_write_nothing(torch_cuda):
    n = 1500
    good_h, good_b = [5, 900, 1400], [0, 10, 10, 1000, n]
    for bad_h, bad_b in (([5, 900, 899, 1400], good_b), ([5, 900, 900, 1400], good_b), ([5, 900, 1400, n], good_b), (good_h, [0, 10, 9, 1000, n]),
                         (good_h, [1, 10, 10, 1000, n]), (good_h, [0, 10, 10, 1000, n - 1]), (good_h, [0, 10, 10, 1000, n + 1])):
        hl, bd = TC.Hits(torch_cuda, bad_h), Bounds(torch_cuda, bad_b)
        out = TC.Outs(torch_cuda, False, {"count": 8, "first": 8 * 5, "hit_file": 8 * hl.k, "hit_line": 8 * hl.k, "files": 8 * 4})
        rc = pb.lib().pire_hip_files(hl.ptr(False), None, hl.k, n, bd.ptr(False), 4, 0, 0, out.ptr("first"), out.ptr("hit_file"), out.ptr("hit_line"),
                                     out.ptr("files"), 4, out.ptr("count"), None)
        assert rc == EINVAL and pb.lib().pire_hip_last_error().decode().startswith("pire_hip_files: "), (bad_h, bad_b)
        out.check({"count": b"", "first": b"", "hit_file": b"", "hit_line": b"", "files": b""}, (bad_h, bad_b))
    run_pass(torch_cuda, False, TC.Hits(torch_cuda, good_h), n, Bounds(torch_cuda, good_b), model_files(good_h, good_b), "good")


@gpu
@pytest.mark.parametrize("shift", range(1, 8))
def test_misaligned_hits(torch_cuda, shift):
    n = 2049
    hits = np.flatnonzero(np.random.RandomState(shift).randint(0, 3, size=n) == 0)
    hl = TC.Hits(torch_cuda, hits, shift=shift)
    bd = Bounds(torch_cuda, random_bounds(n, 70, shift))
    for device in (True, False):
        for without in (False, True):
            run_pass(torch_cuda, device, hl, n, bd, model_files(hits, bd.np, without), (shift, device, without), without=without)


# ---- GPU: the lines forms ----------------------------------------------------------------------------------------------------------

def cut_into_files(raw, delim, seed, files=40):
    """file_bytes: boundaries behind delimiters drawn with a fixed seed, zero-length files among them, and a file of one empty
    line (where the buffer has two delimiters in a row)"""
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    behind = np.flatnonzero(b == delim) + 1
    behind = behind[behind < len(b)]
    rng = np.random.RandomState(seed)
    cuts = list(rng.choice(behind, size=min(files, len(behind)), replace=False)) if len(behind) else []
    cuts += cuts[:3] + cuts[:1]                                            # zero-length files, two of them in a row
    twice = np.flatnonzero((b[:-1] == delim) & (b[1:] == delim)) if len(b) > 1 else []
    if len(twice):
        s = int(twice[len(twice) // 2]) + 1                                # raw[s - 1] and raw[s] are delimiters: raw[s, s + 1) is one empty line
        cuts += [s, s + 1]
    return np.array([0, 0] + sorted(int(c) for c in cuts) + [len(b), len(b)], dtype=np.uint64)


def lines_call(torch, who, tab, device, raw, delim, pick, fb, without, cap, fcap, null=()):
    keep = torch.as_tensor(np.array(raw), device="cuda") if device and len(raw) else raw
    rp = (keep.data_ptr() if device else keep.ctypes.data) if len(raw) else None
    files = len(fb) - 1
    bd = Bounds(torch, fb)
    sizes = {"n": 8, "cnt": 8, "fcnt": 8, "straddles": 8, "hits": 8 * cap, "spans": 16 * cap, "hit_file": 8 * cap, "hit_line": 8 * cap,
             "lines": 8 * (files + 1), "first": 8 * (files + 1), "files": 8 * fcap}
    for k in null:
        sizes[k] = None
    out = TC.Outs(torch, device, sizes)
    if "slow" not in who:
        wm = tab.want_mask([pick])
        want = torch.as_tensor(wm.view(np.int64), device="cuda") if device else wm
        pick = want.data_ptr() if device else want.ctypes.data
    rc = lines_form(who, tab._h, rp, len(raw), delim, BE | (pb.FLAG_ON_DEVICE if device else 0), pick, bd.ptr(device), files, WITHOUT if without else 0,
                    out.ptr("n"), out.ptr("hits") if cap else None, out.ptr("spans") if cap else None, out.ptr("hit_file") if cap else None,
                    out.ptr("hit_line") if cap else None, cap, out.ptr("cnt"), out.ptr("lines"), out.ptr("first"),
                    out.ptr("files") if fcap else None, fcap if "files" not in null else 0, out.ptr("fcnt"), out.ptr("straddles"), stream_of(torch))
    assert rc == 0, (who, pb.lib().pire_hip_last_error())
    return out, keep


def expected(name, k, pick, raw, delim, fb, without, cap, fcap):
    parts, spans = py_lines(raw, bytes([delim]))
    hits = np.flatnonzero(TC.verdicts(name, k, pick))
    file_lines, straddles = model_file_lines(raw, delim, fb)
    exp = model_files(hits, file_lines, without)
    m = min(len(hits), cap)
    return exp, hits, parts, {"n": one(len(parts)), "cnt": one(len(hits)), "fcnt": one(exp["count"]), "straddles": one(straddles), "hits": u64(hits[:m]),
                              "spans": spans[hits][:m], "hit_file": exp["hit_file"][:m], "hit_line": exp["hit_line"][:m], "lines": file_lines,
                              "first": exp["first"], "files": exp["files"][:min(exp["count"], fcap)]}


COMBOS = [("set_a", 0), ("slow_a30", 0), ("slow_a30", ZERO), ("slow_alt", 0), ("slow_alt", ZERO)]


def form_of(name):
    return LINES_FORMS[1] if name in TC.SLOW_INPUTS else LINES_FORMS[0]


@gpu
@pytest.mark.parametrize("name,pick", COMBOS)
def test_files_in_matching_lines_by_file_out(torch_cuda, name, pick):
    torch = torch_cuda
    tab, who = TC.table_of(name), form_of(name)
    for k, (raw, delim) in enumerate(TC.buffers_of(name)):
        fb = cut_into_files(raw, delim, 100 + k)
        files = len(fb) - 1
        n_hits, n_lines = int(TC.verdicts(name, k, pick).sum()), len(TC.verdicts(name, k, pick))
        for without in (False, True):
            for device in (True, False):
                for cap, fcap in sorted({(n_lines + 5, files), (max(n_hits - 1, 0), 3)}) if k < 3 else [(n_lines, files)]:
                    what = (name, pick, k, without, "device" if device else "host", cap, fcap)
                    exp, hits, parts, want = expected(name, k, pick, raw, delim, fb, without, cap, fcap)
                    out, keep = lines_call(torch, who, tab, device, raw, delim, pick, fb, without, cap, fcap)
                    out.check(want, what)
                    if device and len(raw):
                        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
        if k == 0:
            assert files > 40 and (np.diff(fb.astype(np.int64)) == 0).sum() >= 5 and any(bytes(raw[a:b]) == b"\n" for a, b in zip(fb[:-1], fb[1:]))
            # each nullable output left out in turn
            for null in ("hits", "hit_file", "hit_line", "lines", "first", "files"):
                gone = (null, "spans", "hit_file", "hit_line") if null == "hits" else (null,)
                for device in (True, False):
                    exp, hits, parts, want = expected(name, k, pick, raw, delim, fb, False, n_lines, files)
                    out, _ = lines_call(torch, who, tab, device, raw, delim, pick, fb, False, 0 if null == "hits" else n_lines, files, null=gone)
                    out.check(want, (name, pick, "null", null, device))
    # the wrappers
    raw, delim = TC.buffers_of(name)[0]
    fb = cut_into_files(raw, delim, 100)
    exp, hits, parts, want = expected(name, 0, pick, raw, delim, fb, True, len(raw), len(fb) - 1)
    if name in TC.SLOW_INPUTS:
        w = tab.lines_files_host(raw, fb, invert=pick == ZERO, without=True)
    else:
        w = tab.run_lines_files_host(raw, fb, want=[pick], without=True)
    assert (w["lines"], w["count"], w["file_count"], w["straddles"]) == (len(parts), len(hits), exp["count"], 0)
    assert (w["hits"] == hits).all() and (w["hit_file"] == exp["hit_file"]).all() and (w["hit_line"] == exp["hit_line"]).all()
    assert (w["first"] == exp["first"]).all() and (w["files"] == exp["files"]).all() and (w["file_lines"] == want["lines"]).all()


@gpu
@pytest.mark.parametrize("name,pick", [("set_a", 0), ("slow_a30", ZERO)])
def test_boundaries_inside_lines_and_on_the_split_tile_edge(torch_cuda, name, pick):
    torch = torch_cuda
    tab, who = TC.table_of(name), form_of(name)
    raw, delim = TC.buffers_of(name)[0]
    parts, spans = py_lines(raw)
    spans = spans.astype(np.int64).tolist()
    # two boundaries inside lines: line 36 -- a match of the scanners, not of the inverted form -- and line 2000
    assert spans[36][1] - spans[36][0] > 4 and spans[2000][1] - spans[2000][0] > 2
    fb = u64([0, spans[10][0], spans[36][0] + 3, spans[1000][0], spans[2000][0] + 1, len(raw)])
    lines, straddles = model_file_lines(raw, delim, fb)
    assert straddles == 2 and lines.tolist() == [0, 10, 37, 1000, 2001, 3000]   # the straddling line is counted for its first file
    T = pb.SPLIT_TILE
    assert len(raw) > 2 * T + 1
    edge = u64([0, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, len(raw)])
    for bounds in (fb, edge):
        for without in (False, True):
            for device in (True, False):
                exp, hits, _, want = expected(name, 0, pick, raw, delim, bounds, without, len(parts), len(bounds) - 1)
                out, _ = lines_call(torch, who, tab, device, raw, delim, pick, bounds, without, len(parts), len(bounds) - 1)
                now = out.check(want, (name, pick, bounds.tolist(), without, device))
                if bounds is fb:
                    assert now["straddles"][GUARD:GUARD + 8].view(np.uint64)[0] == 2
                    if pick != ZERO:
                        assert 36 in hits and exp["hit_file"][list(hits).index(36)] == 1 and exp["hit_line"][list(hits).index(36)] == 26
                else:
                    assert int(want["straddles"][0]) >= 1


@gpu
@pytest.mark.parametrize("name,pick", [("set_a", 0), ("slow_alt", 0)])
def test_the_chain_with_device_pointers_and_one_read_back(torch_cuda, name, pick):
    """the lines form with device pointers, first[] read back once, then out_hit_spans + 2 * first[f] with first[f + 1] - first[f]
    spans into pire_hip_gather_spans: the matching lines of file f"""
    torch = torch_cuda
    tab = TC.table_of(name)
    raw, delim = TC.buffers_of(name)[1]
    parts, _ = py_lines(raw)
    n, size = len(parts), len(raw)
    fb = cut_into_files(raw, delim, 7, files=12)
    files = len(fb) - 1
    hits = np.flatnonzero(TC.verdicts(name, 1, pick))
    file_lines, _ = model_file_lines(raw, delim, fb)
    exp = model_files(hits, file_lines)
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(np.array(raw), device="cuda")
    d_fb = torch.as_tensor(fb.view(np.int64).copy(), device="cuda")
    d_cnt = torch.zeros(5, dtype=torch.int64, device="cuda")      # lines, hits, listed files, straddles, bytes
    d_hits = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    d_first = torch.zeros(files + 1, dtype=torch.int64, device="cuda")
    common = dict(out_hits_ptr=d_hits.data_ptr(), out_hit_spans_ptr=d_spans.data_ptr(), hit_cap=n, out_file_first_ptr=d_first.data_ptr(),
                  stream=stream)
    if name in TC.SLOW_INPUTS:
        tab.lines_files_device(d_raw.data_ptr(), size, BE, d_fb.data_ptr(), files, d_cnt.data_ptr(), d_cnt[1:].data_ptr(), d_cnt[2:].data_ptr(),
                               d_cnt[3:].data_ptr(), **common)
    else:
        want = torch.as_tensor(tab.want_mask([pick]).view(np.int64), device="cuda")
        tab.run_lines_files_device(d_raw.data_ptr(), size, BE, d_fb.data_ptr(), files, d_cnt.data_ptr(), d_cnt[1:].data_ptr(), d_cnt[2:].data_ptr(),
                                   d_cnt[3:].data_ptr(), want_ptr=want.data_ptr(), **common)
    first = d_first.cpu().numpy()                                  # the one read-back
    assert (first == exp["first"].astype(np.int64)).all()
    d_text = torch.full((size + n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    busiest = sorted(range(files), key=lambda f: -exp["counts"][f])[:3] + [int(np.flatnonzero(exp["counts"] == 0)[0])]
    for f in busiest:
        d_text.fill_(POISON)
        k = int(first[f + 1] - first[f])
        pb.gather_spans_device(d_raw.data_ptr(), size, d_spans.data_ptr() + 16 * int(first[f]), d_cnt[4:].data_ptr(), span_cap=k, tail=delim,
                               out_text_ptr=d_text.data_ptr(), text_cap=size + n, out_offsets_ptr=d_ends.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        joined = b"".join(parts[h] + bytes([delim]) for h in hits if file_lines[f] <= h < file_lines[f + 1])
        got = d_text.cpu().numpy()
        assert int(d_cnt[4]) == len(joined) and got[:len(joined)].tobytes() == joined and (got[len(joined):] == POISON).all(), f
    assert d_cnt.cpu().tolist()[:4] == [n, len(hits), exp["count"], 0] and exp["counts"][busiest[0]] > 3
