"""pire_hip_context and the four lines forms on top of it: from a hit list to the hits and their neighbours -- grep -A / -B /
-C -- on the device (context.hip).

Exact equality everywhere.  The expected values come from `model_context` -- the formula of include/pire_hip.h written down
with numpy, held against a hand-written truth table and, where there is one, against GNU grep --, applied, where a scan is
involved, to what the C oracle says of every line and to Python's own split.  Nothing expected comes from the library.  Every
output of a GPU call sits between poisoned guard bytes and is compared bytewise, what the call had no business writing
included.

Not here: the device form inside a stream capture.  The tests have no capture helper (the one capture of the suite,
tests/test_background_adapt.py, is written out for its own call), so that case is left out."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
GUARD = 64                     # poisoned bytes around every output
EINVAL = -1
BE = ob.FLAG_BEGIN | ob.FLAG_END
ZERO = pb.FINAL_SELECT_ZERO
HIT, GROUP = pb.CONTEXT_HIT, pb.CONTEXT_GROUP
MAX64 = (1 << 64) - 1
gpu = pytest.mark.gpu
NAMES = ("pire_hip_context", "pire_hip_run_lines_context_select", "pire_hip_run_lines_context_gather",
         "pire_hip_slow_lines_context_select", "pire_hip_slow_lines_context_gather")
LINES_FORMS = NAMES[1:]


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_context(hits, n, before, after):
    """include/pire_hip.h: selected(i) <=> some hit h has h - before <= i <= h + after, over the integers (a window wider than
    n is n wide); HIT: i is a hit; GROUP: i == 0 or i - 1 is not selected.  Lines, flags, count, groups."""
    h, i = np.asarray(hits, dtype=np.int64), np.arange(n, dtype=np.int64)
    sel = np.zeros(n, dtype=bool)
    if h.size and n:
        pred, succ = np.searchsorted(h, i, side="right") - 1, np.searchsorted(h, i, side="left")
        sel = ((pred >= 0) & (i - h[np.maximum(pred, 0)] <= min(after, n))) | ((succ < h.size) & (h[np.minimum(succ, h.size - 1)] - i <= min(before, n)))
    group = sel & ~np.concatenate([[False], sel[:-1]])
    lines = np.flatnonzero(sel)
    flags = (np.isin(lines, h) * HIT | group[lines] * GROUP).astype(np.uint8)
    return {"lines": lines.astype(np.uint64), "flags": flags, "count": int(lines.size), "groups": int(group.sum())}


def py_lines(raw, delim=b"\n"):
    """getline: the runs between delimiters; no extra empty line behind a trailing delimiter.  (lines, [begin, end) of every line)"""
    parts = bytes(raw).split(delim)
    if parts and parts[-1] == b"":
        parts.pop()
    spans, pos = [], 0
    for s in parts:
        spans.append((pos, pos + len(s)))
        pos += len(s) + 1
    return parts, np.array(spans, dtype=np.uint64).reshape(-1, 2)


# (hits, n, before, after) -> (lines, flags); H = a hit, G = the first line of a run
TRUTH = [
    (([], 5, 3, 3), ([], [])),
    (([2], 0, 3, 3), ([], [])),
    (([2], 5, 0, 0), ([2], [HIT | GROUP])),
    (([0, 1, 2], 3, 0, 0), ([0, 1, 2], [HIT | GROUP, HIT, HIT])),
    (([2], 6, 1, 2), ([1, 2, 3, 4], [GROUP, HIT, 0, 0])),
    (([0], 4, 5, 1), ([0, 1], [HIT | GROUP, 0])),                       # clipped in front of line 0
    (([3], 4, 1, 9), ([2, 3], [GROUP, HIT])),                           # ... and behind line n - 1
    (([1, 4], 7, 1, 1), ([0, 1, 2, 3, 4, 5], [GROUP, HIT, 0, 0, HIT, 0])),          # the windows touch: one run
    (([1, 5], 8, 1, 1), ([0, 1, 2, 4, 5, 6], [GROUP, HIT, 0, GROUP, HIT, 0])),      # one line between them: two
    (([1, 3], 6, 0, 1), ([1, 2, 3, 4], [HIT | GROUP, 0, HIT, 0])),
    (([1, 3], 6, 1, 0), ([0, 1, 2, 3], [GROUP, HIT, 0, HIT])),
    (([4], 6, MAX64, 0), ([0, 1, 2, 3, 4], [GROUP, 0, 0, 0, HIT])),
    (([1], 4, 0, MAX64), ([1, 2, 3], [HIT | GROUP, 0, 0])),
    (([2], 5, MAX64, MAX64), ([0, 1, 2, 3, 4], [GROUP, 0, HIT, 0, 0])),
]


def test_the_model_against_a_hand_written_truth_table():
    for (hits, n, before, after), (lines, flags) in TRUTH:
        got = model_context(hits, n, before, after)
        assert got["lines"].tolist() == lines and got["flags"].tolist() == flags, (hits, n, before, after)
        assert got["count"] == len(lines) and got["groups"] == sum(1 for f in flags if f & GROUP)
    assert py_lines(b"a\n\nbc")[1].tolist() == [[0, 1], [2, 2], [3, 5]] and py_lines(b"\n")[0] == [b""] and py_lines(b"")[0] == []


def _grep_with_contexts():
    exe = shutil.which("grep")
    if not exe:
        return None
    r = subprocess.run([exe, "--no-group-separator", "-A", "1", "x"], input=b"x\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return exe if r.returncode == 0 and r.stdout == b"x\n" else None


@pytest.mark.skipif(_grep_with_contexts() is None, reason="no grep that accepts --no-group-separator")
def test_the_model_against_grep(tmp_path):
    """grep -n -A a -B b on 40 lines: `N:` a hit, `N-` a neighbour, `--` in front of every run but the first"""
    exe = _grep_with_contexts()
    hits = [0, 3, 4, 11, 17, 18, 19, 30, 39]
    text = [b"needle %d" % i if i in hits else b"hay %d" % i for i in range(40)]
    path = tmp_path / "lines.txt"
    path.write_bytes(b"\n".join(text) + b"\n")
    for after, before in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (5, 5), (3, 7), (40, 0), (0, 40), (100, 100)):
        exp = model_context(hits, 40, before, after)
        out = subprocess.run([exe, "-n", "-A", str(after), "-B", str(before), "needle", str(path)], stdout=subprocess.PIPE, check=True).stdout
        lines, flags, fresh = [], [], True
        for row in out.split(b"\n")[:-1]:
            if row == b"--":
                fresh = True
                continue
            m = re.match(rb"(\d+)([:-])(.*)$", row)
            i = int(m.group(1)) - 1
            assert m.group(3) == text[i]
            lines.append(i)
            flags.append((HIT if m.group(2) == b":" else 0) | (GROUP if fresh else 0))
            fresh = False
        assert lines == exp["lines"].tolist() and flags == exp["flags"].tolist(), (after, before)
        assert out.count(b"\n--\n") == exp["groups"] - 1
        plain = subprocess.run([exe, "--no-group-separator", "-A", str(after), "-B", str(before), "needle", str(path)], stdout=subprocess.PIPE,
                               check=True).stdout
        assert plain == b"".join(text[i] + b"\n" for i in exp["lines"].tolist())


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
    assert re.search(r"#define PIRE_HIP_CONTEXT_HIT +1u", src) and re.search(r"#define PIRE_HIP_CONTEXT_GROUP +2u", src)
    assert (pb.CONTEXT_HIT, pb.CONTEXT_GROUP) == (1, 2)
    assert "pire_hip_context" not in " ".join(pb.selftested_kernels())


def _guarded():
    return {k: np.full(256, POISON, dtype=np.uint8) for k in ("lines", "flags", "spans", "text", "offsets")}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_context_refuses_before_any_device_is_touched():
    L = pb.lib()
    hits = u64([1, 4, 6])
    bufs, cnt, grp = _guarded(), C.c_uint64(77), C.c_uint64(78)
    h, o, f, c, g = hits.ctypes.data, bufs["lines"].ctypes.data, bufs["flags"].ctypes.data, C.addressof(cnt), C.addressof(grp)
    # (hits, hit_cap, n, out_lines, out_line_flags, line_cap, out_line_count, out_group_count)
    cases = {
        "null out_line_count": (h, 3, 8, o, f, 4, None, g),
        "hit_cap > 0 with null hits": (None, 3, 8, o, f, 4, c, g),
        "line_cap > 0 with null out_lines": (h, 3, 8, None, None, 4, c, g),
        "out_line_flags without out_lines": (h, 3, 8, None, f, 0, c, g),
        "2^32 lines or more": (h, 3, 1 << 32, o, f, 4, c, g),
        "2^32 hits or more": (h, 1 << 32, 8, o, f, 4, c, g),
    }
    for what, (a_h, cap, n, a_o, a_f, lcap, a_c, a_g) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            for window in ((1, 1), (MAX64, MAX64)):
                assert L.pire_hip_context(a_h, None, cap, n, window[0], window[1], flags, a_o, a_f, lcap, a_c, a_g, None) == EINVAL, what
                msg = L.pire_hip_last_error().decode()
                assert what in msg and msg.startswith("pire_hip_context: "), (what, msg)
    # host pointers: the list itself, before anything is written (k follows hit_count where it is smaller)
    for what, bad, n in (("strictly ascending", [4, 1, 6], 8), ("strictly ascending", [1, 1, 6], 8), ("hit out of range", [1, 4, 8], 8),
                         ("hit out of range", [0], 0)):
        bad = u64(bad)
        assert L.pire_hip_context(bad.ctypes.data, None, len(bad), n, 1, 1, 0, o, f, 4, c, g, None) == EINVAL, what
        msg = L.pire_hip_last_error().decode()
        assert what in msg and msg.startswith("pire_hip_context: "), (what, msg)
    assert (cnt.value, grp.value) == (77, 78) and _untouched(bufs)
    # no lines, no hits, a hit_count of 0 in front of a list that would be refused: zeros, and no device
    none, nines = C.c_uint64(0), u64([9, 9])
    for a_h, k, cap, n in ((None, None, 0, 0), (None, None, 0, 8), (h, None, 0, 8), (nines.ctypes.data, C.addressof(none), 2, 8)):
        cnt.value, grp.value = 77, 78
        assert L.pire_hip_context(a_h, k, cap, n, 2, 2, 0, o, f, 4, c, g, None) == 0, L.pire_hip_last_error()
        assert (cnt.value, grp.value) == (0, 0) and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="strictly ascending"):   # (the wrappers raise what the library refuses)
        pb.context_host([3, 2], 10)
    got = pb.context_host([], 10, 1, 1)
    assert got["count"] == 0 and got["groups"] == 0 and got["lines"].size == 0 and got["flags"].size == 0


def _slow_blob(name):
    return H.load_blob([c for c in H.golden()["slow"] if c["name"] == name][0]["blob"])


def _big(name):
    big = [b for b in H.big_sets() if b["name"] == name][0]
    return big, H.load_blob(big["blob"])


def lines_form(who, table, raw_ptr, size, delim, flags, pick, before, after, a_n, a_lines, a_flags, a_spans, cap, a_sel, a_grp, a_hit, gather, stream=None):
    """one of the four C calls; pick: want (a pointer) or mode; gather: (tail, out_text, text_cap, out_offsets, out_bytes) in the _gather forms"""
    assert who.endswith("gather") == (gather is not None)
    return getattr(pb.lib(), who)(table, raw_ptr, size, delim, flags, pick, before, after, a_n, a_lines, a_flags, a_spans, cap, a_sel, a_grp, a_hit,
                                  *(tuple(gather) if gather else ()), stream)


def test_the_lines_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"ab" * 20 + b"\nb\n").copy()
    tables = {"run": pb.Table(_big("set_a")[1]), "slow": pb.SlowTable(_slow_blob("slow_a30"))}
    bufs = _guarded()
    n, sel, grp, hit, total = (C.c_uint64(70 + k) for k in range(5))
    r, o, f, s = raw.ctypes.data, bufs["lines"].ctypes.data, bufs["flags"].ctypes.data, bufs["spans"].ctypes.data
    np_, sp, gp, hp, bp = (C.addressof(v) for v in (n, sel, grp, hit, total))
    x, xo = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data
    for who in LINES_FORMS:
        t = tables["slow" if "slow" in who else "run"]._h
        gathers = who.endswith("gather")
        ok_g = (10, x, 32, xo, bp) if gathers else None
        # (table, raw, size, delim, pick, out_line_count, out_lines, out_line_flags, out_line_spans, line_cap, out_sel_count, gather)
        cases = {
            "null table": (None, r, raw.size, 10, 0, np_, o, f, s, 4, sp, ok_g),
            "delim > 255": (t, r, raw.size, 256, 0, np_, o, f, s, 4, sp, ok_g),
            "null out_line_count": (t, r, raw.size, 10, 0, None, o, f, s, 4, sp, ok_g),
            "size > 0 with null raw": (t, None, raw.size, 10, 0, np_, o, f, s, 4, sp, ok_g),
            "null out_sel_count": (t, r, raw.size, 10, 0, np_, o, f, s, 4, None, ok_g),
            "out_line_flags without out_lines": (t, r, raw.size, 10, 0, np_, None, f, None, 0, sp, ok_g),
            "out_line_spans without out_lines": (t, r, raw.size, 10, 0, np_, None, None, s, 0, sp, ok_g),
        }
        if "slow" in who:
            cases["unknown mode"] = (t, r, raw.size, 10, 2, np_, o, f, s, 4, sp, ok_g)
        if gathers:
            cases.update({
                "null out_bytes": (t, r, raw.size, 10, 0, np_, o, f, s, 4, sp, (10, x, 32, xo, None)),
                "tail > 255": (t, r, raw.size, 10, 0, np_, o, f, s, 4, sp, (256, x, 32, xo, bp)),
                "idx_cap > 0 with null out_offsets (idx_cap = line_cap)": (t, r, raw.size, 10, 0, np_, o, f, s, 4, sp, (10, x, 32, None, bp)),
                "text_cap > 0 with null out_text": (t, r, raw.size, 10, 0, np_, o, f, s, 4, sp, (10, None, 32, xo, bp)),
                "out_text overlaps the source": (t, r, raw.size, 10, 0, np_, o, f, s, 4, sp, (10, r + 8, 16, xo, bp)),
            })
        else:
            cases["line_cap > 0 with null out_lines"] = (t, r, raw.size, 10, 0, np_, None, None, None, 4, sp, ok_g)
        for what, (a_t, a_r, size, delim, pick, a_n, a_o, a_f, a_s, cap, a_sel, g) in cases.items():
            for flags in (3, 3 | pb.FLAG_ON_DEVICE):
                rc = lines_form(who, a_t, a_r, size, delim, flags, pick, 2, 2, a_n, a_o, a_f, a_s, cap, a_sel, gp, hp, g)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (who, what, rc, msg)
    assert [v.value for v in (n, sel, grp, hit, total)] == [70, 71, 72, 73, 74] and _untouched(bufs)
    assert (raw == u8(b"ab" * 20 + b"\nb\n")).all()


def test_empty_host_buffers_answer_zeros_without_a_device():
    tables = {"run": pb.Table(_big("set_a")[1]), "slow": pb.SlowTable(_slow_blob("slow_a30"))}
    for who in LINES_FORMS:
        t = tables["slow" if "slow" in who else "run"]._h
        for pick in (0, ZERO) if "slow" in who else (0,):
            bufs = _guarded()
            n, sel, grp, hit, total = (C.c_uint64(70 + k) for k in range(5))
            g = (10, bufs["text"].ctypes.data, 32, bufs["offsets"].ctypes.data, C.addressof(total)) if who.endswith("gather") else None
            rc = lines_form(who, t, None, 0, 10, 3, pick, 2, MAX64, C.addressof(n), bufs["lines"].ctypes.data, bufs["flags"].ctypes.data,
                            bufs["spans"].ctypes.data, 4, C.addressof(sel), C.addressof(grp), C.addressof(hit), g)
            assert rc == 0, pb.lib().pire_hip_last_error()
            assert [v.value for v in (n, sel, grp, hit)] == [0, 0, 0, 0]
            if g:
                assert total.value == 0 and bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
                bufs["offsets"][:8] = POISON
            assert _untouched(bufs)
    # the wrappers on nothing
    got = tables["run"].run_lines_context_host(b"", 1, 1, gather=True)
    assert (got["lines"], got["count"], got["groups"], got["hits"], got["bytes"]) == (0, 0, 0, 0, 0) and got["offsets"].tolist() == [0]
    got = tables["slow"].lines_context_host(b"", 1, 1, invert=True)
    assert (got["lines"], got["count"], got["groups"], got["hits"]) == (0, 0, 0, 0) and got["context"].size == 0 and got["spans"].shape == (0, 2)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """context.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "context.hip" in ba.NO_SCRATCH and "context.hip" in ba.UNITS and "context" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bcontext\.hip\b", mk)) == 2                            # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("context.hip")
    assert not fails, fails
    assert len(seen) == 2 and all("Context" in k for k in seen), seen              # classify, scatter


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "context.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src
    assert "atomic" not in src.lower().replace("no atomics", "").replace("no atomic", "")
    # its own classify kernel between the shared launcher's steps, the second scan for the runs, the shared search and stage
    for shared in ('#include "tile_pass.h"', "TilePass t(", "t.Front(", "TileBallot(", "t.Scan(", "LaunchTileScan(", "t.Scatter(", "t.Done(",
                   "WaveBound<false>(", "LoadU64(", "list.Count(", "list.List(", "list.Back()"):
        assert shared in src, shared
    assert "BlockExclusive" not in src                                             # (the scan is select.hip's, not a copy)
    assert src.count("__global__") == 1 and src.count("hipLaunchKernelGGL") == 1   # (the classify kernel; the scatter is the shared one)
    for copy in ("TileRank(", "TileCompaction(", "__shfl", "UnalignedU64", "hipGetLastError", "hipMemcpyDeviceToHost"):
        assert copy not in src, copy


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class Outs:
    """The outputs of one call, host or device, each `bytes` long between GUARD poisoned bytes (and `shift` bytes further in,
    for an output off its natural alignment); check() compares every one of them bytewise with what the model says the call
    writes -- and leaves alone."""

    def __init__(self, torch, device, sizes, shift=None):
        self.torch, self.device, self.shift = torch, device, shift or {}
        self.host = {k: np.full(2 * GUARD + s, POISON, dtype=np.uint8) for k, s in sizes.items() if s is not None}
        self.dev = {k: torch.as_tensor(v, device="cuda") for k, v in self.host.items()} if device else {}

    def ptr(self, name):
        if name not in self.host:
            return None
        return (self.dev[name].data_ptr() if self.device else self.host[name].ctypes.data) + GUARD + self.shift.get(name, 0)

    def read(self):
        if self.device:
            self.torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in self.dev.items()}
        return {k: v.copy() for k, v in self.host.items()}

    def check(self, want, what=""):
        """want: the payload of every output"""
        now = self.read()
        assert set(want) >= set(now), (set(now), set(want))
        for name, got in now.items():
            payload = want[name] if isinstance(want[name], bytes) else np.ascontiguousarray(want[name]).tobytes()
            full = np.full(len(got), POISON, dtype=np.uint8)
            at = GUARD + self.shift.get(name, 0)
            full[at:at + len(payload)] = u8(payload)
            bad = np.flatnonzero(got != full)
            assert bad.size == 0, (what, name, "first differing byte %d of %d (payload %d bytes)" % (bad[0] - at, len(got) - 2 * GUARD, len(payload)))
        return now


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream or None


def one(v):
    return np.array([v], dtype=np.uint64)


class Hits:
    """a hit list on the host and on the device, `shift` bytes off its natural alignment, poisoned around"""

    def __init__(self, torch, hits, shift=0):
        hits = u64(hits)
        self.k = len(hits)
        self.room = np.full(8 * self.k + 2 * GUARD, POISON, dtype=np.uint8)
        lead = (-self.room.ctypes.data) % 8 + 8 + shift
        self.room[lead:lead + 8 * self.k] = hits.view(np.uint8)
        self.host = self.room.ctypes.data + lead
        self.dev_room = torch.full((8 * self.k + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.dev_lead = (-self.dev_room.data_ptr()) % 8 + 8 + shift
        self.dev_room[self.dev_lead:self.dev_lead + 8 * self.k] = torch.as_tensor(hits.view(np.uint8).copy(), device="cuda")
        self.dev = self.dev_room.data_ptr() + self.dev_lead
        assert self.host % 8 == shift % 8 == self.dev % 8

    def ptr(self, device):
        return (self.dev if device else self.host) if self.k else None


def run_pass(torch, device, hl, n, before, after, line_cap, exp, what, hit_count=None, hit_cap=None, lists=True, flags=True, groups=True,
             flags_shift=0):
    """pire_hip_context, and its outputs against exp -- the model's answer for the k the call was given"""
    out = Outs(torch, device, {"count": 8, "groups": 8 if groups else None, "lines": 8 * line_cap if lists else None,
                               "flags": line_cap if lists and flags else None, "k": None if hit_count is None else 8}, {"flags": flags_shift})
    if hit_count is not None:
        if device:
            out.dev["k"][GUARD:GUARD + 8] = torch.as_tensor(one(hit_count).view(np.uint8), device="cuda")
        else:
            out.host["k"][GUARD:GUARD + 8] = one(hit_count).view(np.uint8)
    rc = pb.lib().pire_hip_context(hl.ptr(device), out.ptr("k"), hl.k if hit_cap is None else hit_cap, n, before, after,
                                   pb.FLAG_ON_DEVICE if device else 0, out.ptr("lines") if line_cap else None, out.ptr("flags") if line_cap else None,
                                   line_cap if lists else 0, out.ptr("count"), out.ptr("groups"), stream_of(torch) if device else None)
    assert rc == 0, (what, pb.lib().pire_hip_last_error())
    m = min(exp["count"], line_cap)
    want = {"count": one(exp["count"]), "groups": one(exp["groups"]), "lines": exp["lines"][:m], "flags": exp["flags"][:m]}
    if hit_count is not None:
        want["k"] = one(hit_count)
    return out.check(want, what)


# ---- GPU: the pass alone -----------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 17)
WINDOWS = (0, 1, 2, 63, 64, 1023, 1024, 1025, "n", MAX64)


def hit_lists(n):
    rng = np.random.RandomState(n)
    lists = {"empty": [], "every line": np.arange(n), "only line 0": [0], "only line n - 1": [n - 1],
             "63|64 and 1023|1024": [h for h in (63, 64, 1023, 1024) if h < n]}
    for d in (2, 50, 1000):
        lists["density 1/%d" % d] = np.flatnonzero(rng.randint(0, d, size=n) == 0)
    return lists


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_from_host_pointers_and_on_the_device(torch_cuda, n):
    """every hit list with before = after = 0 (the list itself comes back) and five of the hundred windows, drawn per list"""
    torch = torch_cuda
    calls = 0
    for k, (name, hits) in enumerate(hit_lists(n).items()):
        hl = Hits(torch, hits)
        rng = np.random.RandomState(1000 * n + k)
        pairs = [(0, 0)] + [tuple(WINDOWS[j] for j in rng.randint(0, len(WINDOWS), size=2)) for _ in range(5)]
        for before, after in pairs:
            before, after = (n if w == "n" else w for w in (before, after))
            exp = model_context(hits, n, before, after)
            if (before, after) == (0, 0):
                assert exp["lines"].tolist() == list(hits) and set(exp["flags"].tolist()) <= {HIT, HIT | GROUP}
            for device in (True, False):
                run_pass(torch, device, hl, n, before, after, n, exp, (n, name, before, after, "device" if device else "host"))
                calls += 1
        got = hl.dev_room.cpu().numpy()
        assert got[hl.dev_lead:hl.dev_lead + 8 * hl.k].tobytes() == u64(hits).tobytes(), "the list was written to"
        assert (got[:hl.dev_lead] == POISON).all() and (got[hl.dev_lead + 8 * hl.k:] == POISON).all(), "the list's surroundings were written to"
    assert calls == 8 * 6 * 2


@gpu
def test_no_lines_from_host_pointers_and_on_the_device(torch_cuda):
    """n == 0: a line count and a run count of 0, whatever the window and the capacity; no list is touched, on either side.  On
    the device a list may stand there all the same (nothing of it is read)."""
    torch = torch_cuda
    exp = model_context([], 0, 0, 0)
    assert (exp["count"], exp["groups"]) == (0, 0)
    for hl in (Hits(torch, []), Hits(torch, [0, 5, 9])):
        for before, after in ((0, 0), (2, 1), (MAX64, MAX64)):
            for line_cap in (0, 4):
                for groups in (True, False):
                    for device in (True, False) if hl.k == 0 else (True,):
                        run_pass(torch, device, hl, 0, before, after, line_cap, exp, (hl.k, before, after, line_cap, groups, device), groups=groups)
        hl_now = hl.dev_room.cpu().numpy()
        assert (np.delete(hl_now, np.arange(hl.dev_lead, hl.dev_lead + 8 * hl.k)) == POISON).all(), "the list's surroundings were written to"


@gpu
@pytest.mark.parametrize("mirror", (False, True))
def test_neighbours_several_tiles_away(torch_cuda, mirror):
    """one hit, a window of 5 000 lines: five tiles take their neighbour from outside their slice of the list, the sixth is empty"""
    n = 6000
    hits, before, after = ([n - 1], 5000, 0) if mirror else ([0], 0, 5000)
    exp = model_context(hits, n, before, after)
    assert exp["count"] == 5001 and exp["groups"] == 1 and exp["lines"].tolist() == list(range(n - 5001, n) if mirror else range(5001))
    hl = Hits(torch_cuda, hits)
    for device in (True, False):
        run_pass(torch_cuda, device, hl, n, before, after, n, exp, (mirror, device))


@gpu
@pytest.mark.parametrize("edge", (64, 1024, 2048))
def test_group_boundaries_across_wave_and_tile_edges(torch_cuda, edge):
    """two windows that exactly touch are one run, one line between them makes two -- with the seam on either side of the edge"""
    n, before, after = edge + 40, 3, 2
    for h1 in range(edge - 2 * (before + after) - 2, edge + 2):
        for gap, groups in ((0, 1), (1, 2)):
            h2 = h1 + after + 1 + gap + before                  # h2 - before == h1 + after + 1 + gap
            exp = model_context([h1, h2], n, before, after)
            assert exp["groups"] == groups and exp["count"] == 2 * (before + after + 1)
            hl = Hits(torch_cuda, [h1, h2])
            run_pass(torch_cuda, True, hl, n, before, after, n, exp, (edge, h1, gap))
    exp = model_context([h1, h2], n, before, after)
    run_pass(torch_cuda, False, hl, n, before, after, n, exp, (edge, "host"))


@gpu
def test_counts_caps_and_k(torch_cuda):
    torch = torch_cuda
    n = 2049
    hits = np.flatnonzero(np.random.RandomState(5).randint(0, 40, size=n) == 0)
    hl = Hits(torch, hits)
    exp = model_context(hits, n, 2, 3)
    count = exp["count"]
    assert 100 < count < n - 100 and exp["groups"] > 10
    for device in (True, False):
        for cap in (0, 1, count - 1, count, count + 5):
            run_pass(torch, device, hl, n, 2, 3, cap, exp, ("cap", cap, device))
        # counts only, lines without flags, no group count
        run_pass(torch, device, hl, n, 2, 3, 0, exp, ("counts only", device), lists=False)
        run_pass(torch, device, hl, n, 2, 3, count, exp, ("no flags", device), flags=False)
        run_pass(torch, device, hl, n, 2, 3, count, exp, ("no groups", device), groups=False)
        # k: *hit_count where it is smaller than hit_cap, hit_cap where it is not, hit_cap where there is no hit_count
        half = len(hits) // 2
        run_pass(torch, device, hl, n, 2, 3, n, model_context(hits[:half], n, 2, 3), ("k = *hit_count", device), hit_count=half)
        run_pass(torch, device, hl, n, 2, 3, n, model_context(hits[:half], n, 2, 3), ("k = hit_cap", device), hit_count=len(hits) + 7, hit_cap=half)
        run_pass(torch, device, hl, n, 2, 3, n, model_context(hits[:half], n, 2, 3), ("no hit_count", device), hit_cap=half)
        run_pass(torch, device, hl, n, 2, 3, n, model_context([], n, 2, 3), ("*hit_count == 0", device), hit_count=0)
    # the wrappers, and the same input twice: the same bits
    w = pb.context_host(hits, n, 2, 3, line_cap=5)
    assert w["count"] == count and w["groups"] == exp["groups"] and (w["lines"] == exp["lines"][:5]).all() and (w["flags"] == exp["flags"][:5]).all()
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    lists = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    marks = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    for k in range(2):
        pb.context_device(hl.dev, hl.k, n, cnt[2 * k:].data_ptr(), 2, 3, out_lines_ptr=lists[k].data_ptr(), out_line_flags_ptr=marks[k].data_ptr(),
                          line_cap=n, out_group_count_ptr=cnt[2 * k + 1:].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [count, exp["groups"]] * 2
    assert (lists.cpu().numpy()[:, :count] == exp["lines"].astype(np.int64)).all() and (marks.cpu().numpy()[:, :count] == exp["flags"]).all()


@gpu
def test_host_pointers_refuse_a_list_that_is_not_ascending_or_out_of_range(torch_cuda):
    n = 1500
    for bad in ([5, 900, 899, 1400], [5, 900, 900, 1400], [5, 900, 1400, n]):
        hl = Hits(torch_cuda, bad)
        out = Outs(torch_cuda, False, {"count": 8, "groups": 8, "lines": 8 * n, "flags": n})
        rc = pb.lib().pire_hip_context(hl.ptr(False), None, hl.k, n, 1, 1, 0, out.ptr("lines"), out.ptr("flags"), n, out.ptr("count"), out.ptr("groups"),
                                       None)
        assert rc == EINVAL and pb.lib().pire_hip_last_error().decode().startswith("pire_hip_context: "), bad
        out.check({"count": b"", "groups": b"", "lines": b"", "flags": b""}, bad)
    # the same list one entry shorter is fine
    run_pass(torch_cuda, False, Hits(torch_cuda, [5, 900, 1400]), n, 1, 1, n, model_context([5, 900, 1400], n, 1, 1), "ascending")


@gpu
@pytest.mark.parametrize("shift", range(1, 8))
def test_misaligned_hits_and_flags(torch_cuda, shift):
    n = 1025
    hits = np.flatnonzero(np.random.RandomState(shift).randint(0, 30, size=n) == 0)
    hl = Hits(torch_cuda, hits, shift=shift)
    exp = model_context(hits, n, 1, 2)
    for device in (True, False):
        run_pass(torch_cuda, device, hl, n, 1, 2, n, exp, (shift, device), flags_shift=shift)
        run_pass(torch_cuda, device, hl, n, MAX64, 0, n, model_context(hits, n, MAX64, 0), (shift, device, "unbounded"), flags_shift=8 - shift)


# ---- GPU: the scanners, their buffers and what the oracle says of every line (shared, computed once) ---------------------------

# name -> (the alphabet of the random lines: none of them matches; the witness behind every 37th line: it does)
SLOW_INPUTS = {"slow_a30": (b"bc ", b"a" + b"b" * 30), "slow_alt": (b"xyz d", b"abc")}
FAST_INPUT = (b"fghijk 0123", bytes.fromhex("68656c6c6f2020776f726c64"))   # set_a, regexp 0: hello\s+w.+d$
_tables, _buffers, _verdicts = {}, {}, {}


def table_of(name):
    if name not in _tables:
        _tables[name] = pb.SlowTable(_slow_blob(name)) if name in SLOW_INPUTS else pb.Table(_big(name)[1])
    return _tables[name]


def buffers_of(name):
    """(raw, delim): about 3 000 random lines, a witness in every 37th, empty lines among them -- with and without a trailing
    delimiter, and with another delimiter --; nothing; a single delimiter; delimiters only"""
    if name not in _buffers:
        alphabet, witness = SLOW_INPUTS[name] if name in SLOW_INPUTS else FAST_INPUT
        lines = H.random_strings(np.random.RandomState(37), 3000, 60, alphabet)
        lines = [s + witness if i % 37 == 36 else s for i, s in enumerate(lines)]
        lines[500:503] = [b""] * 3
        assert not any(b"\n" in s or b"|" in s for s in lines)
        joined = b"\n".join(lines)
        _buffers[name] = [(u8(joined + b"\n").copy(), 10), (u8(joined).copy(), 10), (u8(b"|".join(lines[:1100]) + b"|").copy(), ord("|")),
                          (u8(b"").copy(), 10), (u8(b"\n").copy(), 10), (u8(b"\n" * 70).copy(), 10)]
        for b, _ in _buffers[name]:
            b.setflags(write=False)
    return _buffers[name]


def verdicts(name, k, pick):
    """which lines of buffer k match, from the oracle: bool[n]; pick: mode (slow) or the wanted regexp (Scanner)"""
    key = (name, k)
    if key not in _verdicts:
        raw, delim = buffers_of(name)[k]
        parts, _ = py_lines(raw, bytes([delim]))
        if not parts:
            _verdicts[key] = np.zeros((0, 1), dtype=bool)
        elif name in SLOW_INPUTS:
            fin, _ = ob.OracleSlowScanner(_slow_blob(name)).run_strings(parts, flags=BE)
            _verdicts[key] = (np.asarray(fin) != 0).reshape(-1, 1)
        else:
            t = table_of(name)
            text, offs = H.pack(parts)
            idx = ob.OracleScanner(_big(name)[1]).run(text, offs, flags=BE, threads=4)[0]
            accepted = {s: set(t.AcceptedRegexps(s)) for s in np.unique(idx).tolist()}
            _verdicts[key] = np.array([[r in accepted[s] for r in range(t.RegexpsCount)] for s in idx.tolist()], dtype=bool)
        _verdicts[key].setflags(write=False)
    v = _verdicts[key]
    if name in SLOW_INPUTS:
        return v[:, 0] != (pick == ZERO)
    return v[:, pick]


def test_the_buffers_of_the_gpu_part_have_a_witness_in_every_37th_line_and_nowhere_else():
    for name, pick in (("slow_a30", 0), ("slow_alt", 0), ("set_a", 0)):
        hit = verdicts(name, 0, pick)
        assert len(hit) == 3000 and np.flatnonzero(hit).tolist() == list(range(36, 3000, 37)), name
        assert len(verdicts(name, 2, pick)) == 1100 and len(verdicts(name, 5, pick)) == 70 and not verdicts(name, 5, pick).any()
    assert verdicts("slow_a30", 0, ZERO).sum() == 3000 - 81


def lines_call(torch, who, tab, device, raw, delim, pick, before, after, cap, gather=None, lists=True):
    """gather: None, or (tail, text_cap); pick: mode, or the wanted regexp (staged as a mask where the call runs)"""
    keep = torch.as_tensor(np.array(raw), device="cuda") if device and len(raw) else raw
    rp = (keep.data_ptr() if device else keep.ctypes.data) if len(raw) else None
    sizes = {"n": 8, "sel": 8, "groups": 8, "hit": 8, "lines": 8 * cap if lists else None, "flags": cap if lists else None,
             "spans": 16 * cap if lists else None}
    if gather:
        sizes.update({"text": gather[1], "offsets": 8 * (cap + 1), "bytes": 8})
    out = Outs(torch, device, sizes)
    if "slow" not in who:
        wm = tab.want_mask([pick])
        want = torch.as_tensor(wm.view(np.int64), device="cuda") if device else wm
        pick = want.data_ptr() if device else want.ctypes.data
    g = (gather[0], out.ptr("text") if gather[1] else None, gather[1], out.ptr("offsets"), out.ptr("bytes")) if gather else None
    rc = lines_form(who, tab._h, rp, len(raw), delim, BE | (pb.FLAG_ON_DEVICE if device else 0), pick, before, after, out.ptr("n"),
                    out.ptr("lines") if cap else None, out.ptr("flags") if cap else None, out.ptr("spans") if cap else None, cap, out.ptr("sel"),
                    out.ptr("groups"), out.ptr("hit"), g, stream_of(torch))
    assert rc == 0, (who, pb.lib().pire_hip_last_error())
    return out, keep


LINES_WINDOWS = ((0, 0), (2, 1), (0, 40), (MAX64, 3))


@gpu
@pytest.mark.parametrize("name,pick", [("set_a", 0), ("slow_a30", 0), ("slow_a30", ZERO), ("slow_alt", 0), ("slow_alt", ZERO)])
def test_lines_in_matching_lines_and_their_neighbours_out(torch_cuda, name, pick):
    torch = torch_cuda
    tab = table_of(name)
    select, gather = [w for w in LINES_FORMS if ("slow" in w) == (name in SLOW_INPUTS)]
    for k, (raw, delim) in enumerate(buffers_of(name)):
        d = bytes([delim])
        parts, spans = py_lines(raw, d)
        hit = verdicts(name, k, pick)
        hits = np.flatnonzero(hit)
        for before, after in LINES_WINDOWS if k < 2 else LINES_WINDOWS[1:2]:
            exp = model_context(hits, len(parts), before, after)
            idx = exp["lines"].astype(np.int64)
            count = exp["count"]
            for device in (True, False):
                for cap in sorted({len(parts), max(count - 1, 0)}):
                    what = (name, pick, k, before, after, "device" if device else "host", cap)
                    m = min(count, cap)
                    base = {"n": one(len(parts)), "sel": one(count), "groups": one(exp["groups"]), "hit": one(len(hits)), "lines": exp["lines"][:m],
                            "flags": exp["flags"][:m], "spans": spans[idx][:m]}
                    out, keep = lines_call(torch, select, tab, device, raw, delim, pick, before, after, cap)
                    now = out.check(base, what)
                    got = now["spans"][GUARD:GUARD + 16 * m].view(np.uint64).reshape(-1, 2)
                    assert [bytes(raw[b:e]) for b, e in got.tolist()] == [parts[i] for i in idx[:m].tolist()], what
                    # the bytes: tail = delim is grep -A -B --no-group-separator's output; m lines where the list is short
                    text = b"".join(parts[i] + d for i in idx[:m].tolist())
                    ends = np.cumsum([0] + [len(parts[i]) + 1 for i in idx[:m].tolist()]).astype(np.uint64)
                    full = dict(base, text=text, offsets=ends, bytes=one(len(text)))
                    out, keep = lines_call(torch, gather, tab, device, raw, delim, pick, before, after, cap, gather=(delim, len(raw) + cap))
                    out.check(full, what)
                    if device and len(raw):
                        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
            # the gather form without a list of the caller's, no tail, and a text_cap in the middle of a line: the whole total, the
            # bytes in front of the cap
            if count:
                bare = b"".join(parts[i] for i in idx.tolist())
                room = max(len(bare) - 3, 0)
                ends = np.cumsum([0] + [len(parts[i]) for i in idx.tolist()]).astype(np.uint64)
                for device in (True, False):
                    out, _ = lines_call(torch, gather, tab, device, raw, delim, pick, before, after, len(parts), gather=(pb.NO_TAIL, room), lists=False)
                    out.check({"n": one(len(parts)), "sel": one(count), "groups": one(exp["groups"]), "hit": one(len(hits)), "text": bare[:room],
                               "offsets": ends, "bytes": one(len(bare))}, (name, pick, k, "no tail", device))
    # the wrappers: grep -C 2 of the buffer (slow, inverted: grep -v -C 2)
    raw, _ = buffers_of(name)[0]
    parts, spans = py_lines(raw)
    exp = model_context(np.flatnonzero(verdicts(name, 0, pick)), len(parts), 2, 2)
    if name in SLOW_INPUTS:
        w = tab.lines_context_host(raw, 2, 2, invert=pick == ZERO, gather=True)
    else:
        w = tab.run_lines_context_host(raw, 2, 2, want=[pick], gather=True)
    assert (w["lines"], w["count"], w["groups"], w["hits"]) == (len(parts), exp["count"], exp["groups"], int(verdicts(name, 0, pick).sum()))
    assert (w["context"] == exp["lines"]).all() and (w["flags"] == exp["flags"]).all() and (w["spans"] == spans[exp["lines"].astype(np.int64)]).all()
    assert w["text"].tobytes() == b"".join(parts[i] + b"\n" for i in exp["lines"].tolist())
    # ... and on device pointers: the select form, then the gather form
    d_raw = torch.as_tensor(np.array(raw), device="cuda")
    words = torch.zeros(5, dtype=torch.int64, device="cuda")      # lines, selected, runs, hits, bytes
    d_lines = torch.full((len(parts),), -1, dtype=torch.int64, device="cuda")
    d_flags = torch.zeros(len(parts), dtype=torch.uint8, device="cuda")
    d_text = torch.zeros(len(raw) + len(parts), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(len(parts) + 1, dtype=torch.int64, device="cuda")
    want = None if name in SLOW_INPUTS else torch.as_tensor(tab.want_mask([pick]).view(np.int64), device="cuda")
    for out_bytes in (None, words[4:].data_ptr()):
        common = dict(out_lines_ptr=d_lines.data_ptr(), out_line_flags_ptr=d_flags.data_ptr(), line_cap=len(parts),
                      out_group_count_ptr=words[2:].data_ptr(), out_hit_count_ptr=words[3:].data_ptr(), out_bytes_ptr=out_bytes,
                      out_text_ptr=d_text.data_ptr(), text_cap=d_text.numel(), out_offsets_ptr=d_offs.data_ptr(), stream=stream_of(torch) or 0)
        if name in SLOW_INPUTS:
            tab.lines_context_device(d_raw.data_ptr(), len(raw), BE, words.data_ptr(), words[1:].data_ptr(), 2, 2, invert=pick == ZERO, **common)
        else:
            tab.run_lines_context_device(d_raw.data_ptr(), len(raw), BE, words.data_ptr(), words[1:].data_ptr(), 2, 2, want_ptr=want.data_ptr(),
                                         **common)
        torch.cuda.synchronize()
        assert words.cpu().tolist() == [len(parts), exp["count"], exp["groups"], int(verdicts(name, 0, pick).sum()), 0 if out_bytes is None else w["bytes"]]
        assert (d_lines.cpu().numpy()[:exp["count"]] == exp["lines"].astype(np.int64)).all() and (d_flags.cpu().numpy()[:exp["count"]] == exp["flags"]).all()
    assert d_text.cpu().numpy()[:w["bytes"]].tobytes() == w["text"].tobytes() and (d_offs.cpu().numpy()[:exp["count"] + 1] == w["offsets"].astype(np.int64)).all()


@gpu
@pytest.mark.parametrize("k", (0, 1))
def test_the_chain_with_device_pointers_and_one_read_back(torch_cuda, k):
    """pire_hip_split with out_text == NULL, pire_hip_run_lines_select for the hits, pire_hip_context, pire_hip_gather with
    NO_TAIL over raw and the split's offsets: the selected lines with their delimiters"""
    torch = torch_cuda
    name, pick = "set_a", 0
    tab = table_of(name)
    raw, delim = buffers_of(name)[k]
    parts, _ = py_lines(raw)
    n, size = len(parts), len(raw)
    exp = model_context(np.flatnonzero(verdicts(name, k, pick)), n, 1, 2)
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(np.array(raw), device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(6, dtype=torch.int64, device="cuda")      # n, lines of the scan, hits, selected, groups, bytes
    d_hits = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_lines = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_text = torch.full((size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    want = torch.as_tensor(tab.want_mask([pick]).view(np.int64), device="cuda")
    pb.split_device(d_raw.data_ptr(), size, d_cnt[0:].data_ptr(), out_offsets_ptr=d_off.data_ptr(), offsets_cap=n, stream=stream)
    tab.run_lines_select_device(d_raw.data_ptr(), size, BE, d_cnt[1:].data_ptr(), d_cnt[2:].data_ptr(), want_ptr=want.data_ptr(),
                                out_hits_ptr=d_hits.data_ptr(), hit_cap=n, stream=stream)
    pb.context_device(d_hits.data_ptr(), n, n, d_cnt[3:].data_ptr(), 1, 2, hit_count_ptr=d_cnt[2:].data_ptr(), out_lines_ptr=d_lines.data_ptr(),
                      line_cap=n, out_group_count_ptr=d_cnt[4:].data_ptr(), stream=stream)
    pb.gather_device(d_raw.data_ptr(), d_off.data_ptr(), n, d_cnt[5:].data_ptr(), idx_ptr=d_lines.data_ptr(), idx_count_ptr=d_cnt[3:].data_ptr(),
                     idx_cap=n, tail=None, out_text_ptr=d_text.data_ptr(), text_cap=size, out_offsets_ptr=d_ends.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ends = np.cumsum([0] + [len(p) + 1 for p in parts])
    ends[-1] = size                                                # (the last line of buffer 1 has no delimiter behind it)
    joined = b"".join(bytes(raw[ends[i]:ends[i + 1]]) for i in exp["lines"].tolist())
    assert d_cnt.cpu().tolist() == [n, n, int(verdicts(name, k, pick).sum()), exp["count"], exp["groups"], len(joined)]
    got = d_text.cpu().numpy()
    assert got[:len(joined)].tobytes() == joined and (got[len(joined):] == POISON).all()
    assert (d_lines.cpu().numpy()[:exp["count"]] == exp["lines"].astype(np.int64)).all()
