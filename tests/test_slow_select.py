"""pire_hip_final_select, the two slow run forms and the two slow lines forms: from a SlowScanner's Final flags to the strings
(lines) that matched -- or, with PIRE_HIP_FINAL_SELECT_ZERO, did not -- on the device (slow_hits.hip).

Exact equality everywhere.  The expected values come from `model_final_select` -- the formula of include/pire_hip.h written down
with numpy --, applied, where a scan is involved, to what the C oracle's SlowScanner walk says (tests/test_slow.py holds it
against the unmodified reference; where that reference is built, three scanners are compiled by it here), and for lines to
Python's own split.  Nothing expected comes from the library.  Every output of a call sits between poisoned guard bytes and
is compared bytewise, what the call had no business writing included."""
import ctypes as C
import json
import os
import re

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
gpu = pytest.mark.gpu
NAMES = ("pire_hip_final_select", "pire_hip_slow_run_select", "pire_hip_slow_run_select_strided", "pire_hip_slow_lines_select",
         "pire_hip_slow_lines_gather")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_final_select(final, invert=False):
    """include/pire_hip.h: selected(i) <=> (final[i] != 0) != invert; every hit, ascending, and their number"""
    final = np.asarray(final, dtype=np.uint8)
    hits = np.flatnonzero((final != 0) != bool(invert)).astype(np.uint64)
    return {"hits": hits, "count": int(hits.size)}


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


def test_the_model_against_a_hand_written_truth_table():
    fin = [0, 1, 0, 2, 0x80, 0, 0xFF]
    assert model_final_select(fin)["hits"].tolist() == [1, 3, 4, 6] and model_final_select(fin)["count"] == 4
    assert model_final_select(fin, True)["hits"].tolist() == [0, 2, 5]
    assert model_final_select([])["count"] == 0 and model_final_select([], True)["count"] == 0
    assert [p for p in py_lines(b"a\n\nbc\n")[0]] == [b"a", b"", b"bc"] and py_lines(b"a\n\nbc")[1].tolist() == [[0, 1], [2, 2], [3, 5]]
    assert py_lines(b"")[0] == [] and py_lines(b"\n")[0] == [b""] and py_lines(b"x|y|", b"|")[0] == [b"x", b"y"]


# ---- the scanners, their batches and what the oracle says (shared; the oracle runs once per scanner and flag combination) -----
# name -> (where the Save() form comes from, the alphabet of the random strings, what is appended to every third string).
# The appended witness makes a third of the batch match where random text alone would not (hello.{20}world) or would only rarely.
GOLDEN_SLOW = ("slow_a30", "slow_x40_utf8", "slow_alt")
GOLDEN_WIDE = "slow_x300"                                                   # 607 states: the wave-per-string kernel
REF = {"ref_a30": ("a.{30}$", ""), "ref_x40_utf8": ("x.{40}$", "u"), "ref_hello": ("hello.{20}world", "")}
INPUTS = {
    "slow_a30": (b"ab", None),
    "slow_x40_utf8": (b"xyzw abc", b"x" + b"abc yzw " * 5),
    "slow_alt": (b"abcde", None),
    "slow_x300": (b"xyab", None),
    "ref_a30": (b"ab", None),
    "ref_x40_utf8": (b"xyzw abc", b"x" + b"abc yzw " * 5),
    "ref_hello": (b"helowrd abcxyz0123456789", b"hello 0123456789abcdef xyworld"),
}
MAX_LEN = {"slow_x300": 900}
ALL_CASES = GOLDEN_SLOW + (GOLDEN_WIDE,) + tuple(REF)
needs_ref = pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref/libpire_ref.so not built")
CASE_PARAMS = [pytest.param(n, marks=needs_ref) if n in REF else n for n in ALL_CASES]
_blobs, _batches, _oracle = {}, {}, {}


def blob_of(name):
    if name not in _blobs:
        if name in REF:
            _blobs[name] = ob.RefSlowScanner.compile(*REF[name]).save()
        elif name == GOLDEN_WIDE:
            with open(os.path.join(H.GOLDEN, "slow_wide.json")) as f:
                _blobs[name] = H.load_blob([c for c in json.load(f)["slow_wide"] if c["name"] == name][0]["blob"])
        else:
            _blobs[name] = H.load_blob([c for c in H.golden()["slow"] if c["name"] == name][0]["blob"])
    return _blobs[name]


def batch(name):
    """3 000 random strings of the scanner's alphabet, the witness behind every third, and b"" """
    if name not in _batches:
        alphabet, witness = INPUTS[name]
        strings = H.random_strings(np.random.RandomState(11), 3000, MAX_LEN.get(name, 200), alphabet)
        if witness:
            strings = [s + witness if i % 3 == 0 else s for i, s in enumerate(strings)]
        _batches[name] = strings + [b""]
    return _batches[name]


def oracle_final(name, flags, strings=None):
    """Final per string of the batch (or of `strings`) from the C oracle, and the state sets"""
    key = (name, flags)
    if strings is None and key in _oracle:
        return _oracle[key]
    fin, bits = ob.OracleSlowScanner(blob_of(name)).run_strings(batch(name) if strings is None else strings, flags=flags)
    fin, bits = np.ascontiguousarray(fin, dtype=np.uint8), np.ascontiguousarray(bits, dtype=np.uint32)
    if strings is None:
        fin.setflags(write=False)
        bits.setflags(write=False)
        _oracle[key] = (fin, bits)
    return fin, bits


# ---- CPU -----------------------------------------------------------------------------------------------------------------

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
    assert re.search(r"#define PIRE_HIP_FINAL_SELECT_ZERO 1u", src) and pb.FINAL_SELECT_ZERO == 1


def _guarded(cap=4):
    return {"hits": np.full(8 * (cap + 2), POISON, dtype=np.uint8), "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8),
            "final": np.full(16, POISON, dtype=np.uint8), "text": np.full(64, POISON, dtype=np.uint8),
            "offsets": np.full(8 * (cap + 3), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


# what pire_hip_final_select refuses of (final, n, mode, out_hits, hit_cap, out_hit_count): the message, and the arguments as
# a function of the valid ones
PASS_REFUSALS = {
    "unknown mode": lambda f, h, c: (f, 6, 2, h, 4, c),
    "unknown mode ": lambda f, h, c: (f, 6, 0x80000000, h, 4, c),
    "n > 0 with null final": lambda f, h, c: (None, 6, 0, h, 4, c),
    "null out_hit_count": lambda f, h, c: (f, 6, ZERO, h, 4, None),
    "hit_cap > 0 with null out_hits": lambda f, h, c: (f, 6, ZERO, None, 4, c),
    "2^32 strings or more": lambda f, h, c: (f, 1 << 32, 0, h, 4, c),
}


def test_final_select_refuses_before_any_device_is_touched():
    L = pb.lib()
    fin = np.array([0, 1, 2, 0, 0x80, 0], dtype=np.uint8)
    bufs, cnt = _guarded(), C.c_uint64(77)
    for what, args in PASS_REFUSALS.items():
        a_f, n, mode, a_h, cap, a_c = args(fin.ctypes.data, bufs["hits"].ctypes.data, C.addressof(cnt))
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_final_select(a_f, n, mode, flags, a_h, cap, a_c, None) == EINVAL, what
            msg = L.pire_hip_last_error().decode()
            assert what.strip() in msg and msg.startswith("pire_hip_final_select: "), (what, msg)
    assert cnt.value == 77 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="hit_cap > 0 with null out_hits"):   # (the wrappers raise what the library refuses)
        pb.final_select_device(fin.ctypes.data, 6, C.addressof(cnt), hit_cap=3)


def test_the_run_forms_refuse_before_any_device_is_touched():
    """what pire_hip_final_select refuses (a scan has its flags: `n > 0 with null final` has no counterpart), and what the run
    call refuses: no table, no offsets, a stride smaller than the records"""
    L = pb.lib()
    text, offs = H.pack([b"ab" * 20, b"b"])
    text, offs = text.copy(), offs.copy()
    tab = pb.SlowTable(blob_of("slow_a30"))
    bufs, cnt = _guarded(), C.c_uint64(77)
    x, o, f, h, c = text.ctypes.data, offs.ctypes.data, bufs["final"].ctypes.data, bufs["hits"].ctypes.data, C.addressof(cnt)
    # (table, n, mode, out_hits, hit_cap, out_hit_count)
    cases = {
        "unknown mode": (tab._h, 2, 2, h, 4, c),
        "null out_hit_count": (tab._h, 2, 0, h, 4, None),
        "hit_cap > 0 with null out_hits": (tab._h, 2, ZERO, None, 4, c),
        "2^32 strings or more": (tab._h, 1 << 32, 0, h, 4, c),
        "null table": (None, 2, 0, h, 4, c),
    }
    for what, (a_t, n, mode, a_h, cap, a_c) in cases.items():
        for flags in (3, 3 | pb.FLAG_ON_DEVICE):
            for who in ("pire_hip_slow_run_select", "pire_hip_slow_run_select_strided"):
                if who.endswith("strided"):
                    rc = L.pire_hip_slow_run_select_strided(a_t, x, n, 1, 1, flags, mode, f, None, None, a_h, cap, a_c, None)
                else:
                    rc = L.pire_hip_slow_run_select(a_t, x, o, n, flags, mode, f, None, None, a_h, cap, a_c, None)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (who, what, rc, msg)
    for flags in (3, 3 | pb.FLAG_ON_DEVICE):
        assert L.pire_hip_slow_run_select(tab._h, x, None, 2, flags, 0, f, None, None, h, 4, c, None) == EINVAL
        assert L.pire_hip_last_error().decode() == "pire_hip_slow_run_select: null offsets"
        assert L.pire_hip_slow_run_select_strided(tab._h, x, 2, 8, 4, flags, 0, f, None, None, h, 4, c, None) == EINVAL
        assert L.pire_hip_last_error().decode() == "pire_hip_slow_run_select_strided: stride smaller than len"
    assert cnt.value == 77 and _untouched(bufs)


def test_the_lines_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"ab" * 20 + b"\nb\n").copy()
    tab = pb.SlowTable(blob_of("slow_a30"))
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    r, lp, h, s, c = raw.ctypes.data, C.addressof(lines), bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    x, xo, bp = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data, C.addressof(total)
    # (table, raw, size, delim, mode, out_line_count, out_hits, out_hit_spans, hit_cap, out_hit_count)
    select = {
        "null table": (None, r, raw.size, 10, 0, lp, h, s, 4, c),
        "unknown mode": (tab._h, r, raw.size, 10, 2, lp, h, s, 4, c),
        "null out_hit_count": (tab._h, r, raw.size, 10, 0, lp, h, s, 4, None),
        "hit_cap > 0 with null out_hits": (tab._h, r, raw.size, 10, ZERO, lp, None, None, 4, c),
        "out_hit_spans without out_hits": (tab._h, r, raw.size, 10, 0, lp, None, s, 0, c),
        "delim > 255": (tab._h, r, raw.size, 300, 0, lp, h, s, 4, c),
        "null out_line_count": (tab._h, r, raw.size, 10, 0, None, h, s, 4, c),
        "size > 0 with null raw": (tab._h, None, raw.size, 10, ZERO, lp, h, s, 4, c),
    }
    for what, (a_t, a_r, size, delim, mode, a_l, a_h, a_s, cap, a_c) in select.items():
        for flags in (3, 3 | pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_slow_lines_select(a_t, a_r, size, delim, flags, mode, a_l, a_h, a_s, cap, a_c, None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_slow_lines_select: "), (what, rc, msg)
    # (table, raw, size, delim, mode, tail, out_line_count, out_hits, hit_cap, out_hit_count, out_text, text_cap, out_offsets, out_bytes)
    gather = {
        "null table": (None, r, raw.size, 10, 0, 10, lp, h, 4, c, x, 32, xo, bp),
        "unknown mode": (tab._h, r, raw.size, 10, 3, 10, lp, h, 4, c, x, 32, xo, bp),
        "null out_hit_count": (tab._h, r, raw.size, 10, 0, 10, lp, h, 4, None, x, 32, xo, bp),
        "delim > 255": (tab._h, r, raw.size, 256, 0, 10, lp, h, 4, c, x, 32, xo, bp),
        "null out_line_count": (tab._h, r, raw.size, 10, 0, 10, None, h, 4, c, x, 32, xo, bp),
        "size > 0 with null raw": (tab._h, None, raw.size, 10, ZERO, 10, lp, h, 4, c, x, 32, xo, bp),
        "null out_bytes": (tab._h, r, raw.size, 10, ZERO, 10, lp, h, 4, c, x, 32, xo, None),
        "tail > 255": (tab._h, r, raw.size, 10, 0, 256, lp, h, 4, c, x, 32, xo, bp),
        "idx_cap > 0 with null out_offsets (idx_cap = hit_cap)": (tab._h, r, raw.size, 10, 0, 10, lp, h, 4, c, x, 32, None, bp),
        "text_cap > 0 with null out_text": (tab._h, r, raw.size, 10, 0, 10, lp, h, 4, c, None, 32, xo, bp),
        "out_text overlaps the source": (tab._h, r, raw.size, 10, 0, 10, lp, h, 4, c, r + 8, 16, xo, bp),
    }
    for what, a in gather.items():
        for flags in (3, 3 | pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_slow_lines_gather(a[0], a[1], a[2], a[3], flags, *a[4:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_slow_lines_gather: "), (what, rc, msg)
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)
    assert (raw == u8(b"ab" * 20 + b"\nb\n")).all()


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    tab = pb.SlowTable(blob_of("slow_a30"))
    offs0 = np.zeros(1, dtype=np.uint64)
    dummy = np.zeros(16, dtype=np.uint8)
    for mode in (0, ZERO):
        bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
        h, s, f, c, lp = bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, bufs["final"].ctypes.data, C.addressof(cnt), C.addressof(lines)
        for fin in (None, dummy.ctypes.data):
            cnt.value = 77
            assert L.pire_hip_final_select(fin, 0, mode, 0, h, 4, c, None) == 0, L.pire_hip_last_error()
            assert cnt.value == 0
        cnt.value = 77
        assert L.pire_hip_slow_run_select(tab._h, None, offs0.ctypes.data, 0, 3, mode, f, None, None, h, 4, c, None) == 0
        assert cnt.value == 0
        cnt.value = 77
        assert L.pire_hip_slow_run_select_strided(tab._h, None, 0, 128, 144, 3, mode, f, None, None, h, 4, c, None) == 0
        assert cnt.value == 0 and lines.value == 78
        cnt.value = 77
        assert L.pire_hip_slow_lines_select(tab._h, None, 0, 10, 3, mode, lp, h, s, 4, c, None) == 0
        assert (cnt.value, lines.value) == (0, 0)
        assert _untouched(bufs)
        cnt.value, lines.value = 77, 78
        assert L.pire_hip_slow_lines_gather(tab._h, None, 0, 10, 3, mode, 10, lp, h, 4, c, bufs["text"].ctypes.data, 32, bufs["offsets"].ctypes.data,
                                            C.addressof(total), None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0)
        assert bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
        bufs["offsets"][:8] = POISON
        assert _untouched(bufs)
    # the wrappers on nothing
    for invert in (False, True):
        got = pb.final_select_host(np.zeros(0, dtype=np.uint8), invert=invert)
        assert got["count"] == 0 and got["hits"].size == 0
        got = tab.run_select(np.zeros(0, np.uint8), offs0, invert=invert)
        assert got["count"] == 0 and got["hits"].size == 0 and got["final"].size == 0
        assert tab.run_select_strings([], invert=invert)["count"] == 0
        gl = tab.lines_select_host(b"", invert=invert)
        assert gl["lines"] == 0 and gl["count"] == 0 and gl["hits"].size == 0 and gl["spans"].shape == (0, 2)
        gg = tab.lines_gather_host(b"", invert=invert)
        assert gg["lines"] == 0 and gg["count"] == 0 and gg["bytes"] == 0 and gg["text"].size == 0 and gg["offsets"].tolist() == [0]


@pytest.mark.parametrize("name", CASE_PARAMS)
def test_every_input_of_the_gpu_part_selects_some_strings_and_not_all(name):
    """... between 1 % and 99 % of them on the oracle's own numbers under BEGIN | END, in both modes: no list or count of the
    GPU part can be right by being empty or full.  With neither flag a pattern that ends in `$` is Final nowhere (its last
    step is End()'s): those batches select nothing, and everything when inverted -- stated here, not excused: the patterns
    without `$` meet the condition there as well."""
    strings = batch(name)
    alphabet, witness = INPUTS[name]
    assert len(strings) == 3001 and strings[-1] == b"" and not any(b"\n" in s or b"|" in s for s in strings)
    assert name in REF or blob_of(name)
    fin, _ = oracle_final(name, BE)
    for invert in (False, True):
        share = model_final_select(fin, invert)["count"] / len(strings)
        assert 0.01 <= share <= 0.99, (name, invert, share)
    none, _ = oracle_final(name, 0)
    dollar = name not in ("slow_alt", "ref_hello")
    if dollar:
        assert not none.any(), name
    else:
        assert 0.01 <= np.count_nonzero(none) / len(strings) <= 0.99, name
    # the lines forms' buffers are cut from the same strings: first and last line of them match
    lines = lines_of(name)
    lf, _ = oracle_final(name, BE, strings=lines)
    assert lf[0] and lf[-1] and not lf[1] and 0.01 <= np.count_nonzero(lf) / len(lines) <= 0.99 and lines.count(b"") >= 3


def lines_of(name):
    """~1 000 lines of the batch, none with a delimiter in it: a first and a last line that match, a second that does not,
    three empty lines in a row"""
    strings = batch(name)
    fin, _ = oracle_final(name, BE)
    hit = strings[int(np.flatnonzero(fin)[0])]
    miss = [s for s, f in zip(strings, fin) if s and not f][0]
    body = [s for s in strings[:1000] if s]
    return [hit, miss] + body[:100] + [b""] * 3 + body[100:] + [hit]


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """slow_hits.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "slow_hits.hip" in ba.NO_SCRATCH and "slow_hits.hip" in ba.UNITS and "slow_hits" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bslow_hits\.hip\b", mk)) == 2                          # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("slow_hits.hip")
    assert not fails, fails
    assert len(seen) == 2 and all("Final" in k for k in seen), seen                # classify, scatter


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "slow_hits.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
    for shared in ('#include "tile_pass.h"', "TilePass t(", "t.Front(", "t.Classify(", "t.Tail(", "list.Count(", "list.List("):
        assert shared in src, shared
    assert "__shfl" not in src and "__ballot" not in src and "BlockExclusive" not in src   # (the scan is select.hip's, not a copy)
    # both kernels, the launcher and the copies back are the shared ones: the unit has a predicate and a Write, nothing else of a pass
    for copy in ("__global__", "hipLaunchKernelGGL", "TileBallot(", "TileRank(", "LaunchTileScan(", "TileCompaction(", "hipGetLastError", "hipMemcpy"):
        assert copy not in src, copy


def test_the_copy_back_of_a_hit_list_has_two_homes():
    """"The lists come back only as far as they were written" is HitStage::Back (select.hip) and its row-pitch form HitsBack
    (api.cpp): none of the eight hit passes copies from the device on its own, nor do the two scans that stage a capture pass."""
    csrc = os.path.join(ROOT, "pire_amd", "csrc")
    units = ("select.hip", "capture_select.hip", "count_select.hip", "slow_hits.hip", "affix.hip", "context.hip", "files.hip", "combine.hip")
    for unit in units + ("slow_capture.hip",):
        with open(os.path.join(csrc, unit)) as f:
            src = f.read()
        assert src.count("hipMemcpyDeviceToHost") == (1 if unit == "select.hip" else 0), unit
    with open(os.path.join(csrc, "select.hip")) as f:
        back = f.read().split("int HitStage::Back()")[1].split("\n}\n")[0]
    assert "hipMemcpyDeviceToHost" in back and "std::min<uint64_t>(count, cap)" in back
    with open(os.path.join(csrc, "api.cpp")) as f:
        api = f.read()
    assert api.count("const uint64_t written = std::min(") == 2   # HitsBack, and the gather's offsets in LinesFrame::Close


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class Outs:
    """The outputs of one call, host or device, each `bytes` long between GUARD poisoned bytes; check() compares every one of
    them bytewise with what the model says the call writes -- and leaves alone."""

    def __init__(self, torch, device, cap, hits=True, spans=False, lines=False, final=0, bits=0, text=None):
        self.torch, self.device, self.cap = torch, device, cap
        sizes = {"count": 8, "hits": 8 * cap if hits else None, "spans": 16 * cap if spans else None, "lines": 8 if lines else None,
                 "final": final or None, "bits": 4 * bits or None, "text": text, "offsets": None if text is None else 8 * (cap + 1),
                 "bytes": None if text is None else 8}
        self.host = {k: np.full(2 * GUARD + s, POISON, dtype=np.uint8) for k, s in sizes.items() if s is not None}
        self.dev = {k: torch.as_tensor(v, device="cuda") for k, v in self.host.items()} if device else {}

    def ptr(self, name):
        if name not in self.host:
            return None
        return (self.dev[name].data_ptr() if self.device else self.host[name].ctypes.data) + GUARD

    def read(self):
        if self.device:
            self.torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in self.dev.items()}
        return {k: v.copy() for k, v in self.host.items()}

    def check(self, exp, what="", **more):
        """exp: the model's answer with every hit; the first min(count, cap) entries of the list, and nothing else, were written.
        more: the payload of every other output the call has"""
        now = self.read()
        k = min(exp["count"], self.cap)
        want = {"count": np.array([exp["count"]], dtype=np.uint64), "hits": exp["hits"][:k].astype(np.uint64)}
        want.update(more)
        assert set(want) >= set(now), (set(now), set(want))
        for name, got in now.items():
            payload = want[name] if isinstance(want[name], bytes) else np.ascontiguousarray(want[name]).tobytes()
            full = np.full(len(got), POISON, dtype=np.uint8)
            full[GUARD:GUARD + len(payload)] = u8(payload)
            bad = np.flatnonzero(got != full)
            assert bad.size == 0, (what, name, "first differing byte %d of %d (payload %d bytes)" % (bad[0] - GUARD, len(got) - 2 * GUARD, len(payload)))
        return now


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream or None


# ---- GPU: the pass alone -----------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, (1 << 20) + 1025)   # the last: 1 026 tiles, the tile scan carries between two steps
PATTERNS = ("none", "all", "every third", "only the last", "lane 0 of every wave")


def flags_of(pattern, n, value):
    fin = np.zeros(n, dtype=np.uint8)
    if pattern == "all":
        fin[:] = value
    elif pattern == "every third":
        fin[::3] = value
    elif pattern == "only the last":
        fin[-1] = value
    elif pattern == "lane 0 of every wave":
        fin[::64] = value
    return fin


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_on_flags_written_by_the_test(torch_cuda, n):
    """The classify kernel loads its flags byte by byte: no alignment cases.  The flags lie 3 bytes behind a 16-byte boundary
    all the same, on the host and on the device."""
    torch = torch_cuda
    assert (n + 1023) // 1024 > 1024 or n <= 2049
    room = np.zeros(n + 32, dtype=np.uint8)
    lead = 3 + (-room.ctypes.data % 16)
    fin = room[lead:lead + n]
    dev_room = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    dev_lead = 3 + (-dev_room.data_ptr() % 16)
    calls = 0
    for pattern in PATTERNS:
        for value in (1, 2, 0x80):
            fin[:] = flags_of(pattern, n, value)
            dev_room[dev_lead:dev_lead + n] = torch.as_tensor(fin, device="cuda")
            for mode in (0, ZERO):
                exp = model_final_select(fin, mode == ZERO)
                count = exp["count"]
                assert count == {"none": 0, "all": n, "every third": (n + 2) // 3, "only the last": 1, "lane 0 of every wave": (n + 63) // 64}[
                    pattern] if mode == 0 else count + model_final_select(fin)["count"] == n
                for cap in sorted({c for c in (0, count - 1, count, count + 7) if c >= 0}):
                    for device in (True, False):
                        out = Outs(torch, device, cap)
                        ptr = dev_room.data_ptr() + dev_lead if device else fin.ctypes.data
                        rc = pb.lib().pire_hip_final_select(ptr, n, mode, pb.FLAG_ON_DEVICE if device else 0, out.ptr("hits") if cap else None, cap,
                                                            out.ptr("count"), stream_of(torch) if device else None)
                        assert rc == 0, pb.lib().pire_hip_last_error()
                        out.check(exp, (n, pattern, value, mode, cap, "device" if device else "host"))
                        calls += 1
    assert calls >= 5 * 3 * 2 * 2 * 2                                           # (count == 0: the capacities are 0 and 7 alone)
    got = dev_room.cpu().numpy()
    assert (got[dev_lead:dev_lead + n] == fin).all() and not got[:dev_lead].any() and not got[dev_lead + n:].any(), "the input was written to"
    # the wrappers, and the same input twice: the same bits
    w = pb.final_select_host(fin, invert=True, hit_cap=5)
    exp = model_final_select(fin, True)
    assert w["count"] == exp["count"] and (w["hits"] == exp["hits"][:5]).all()
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    lists = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    for k in range(2):
        pb.final_select_device(dev_room.data_ptr() + dev_lead, n, cnt[k:].data_ptr(), invert=False, out_hits_ptr=lists[k].data_ptr(), hit_cap=n,
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    exp = model_final_select(fin)
    assert cnt.cpu().tolist() == [exp["count"]] * 2 and (lists.cpu().numpy()[:, :exp["count"]] == exp["hits"].astype(np.int64)).all()


@gpu
def test_no_strings_from_host_pointers_and_on_the_device(torch_cuda):
    """n == 0: a count of 0 in either mode, whatever the capacity; the list is not touched, on either side"""
    torch = torch_cuda
    room = np.zeros(16, dtype=np.uint8)                       # (somewhere to point: nothing of it is read)
    dev_room = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for mode in (0, ZERO):
        exp = model_final_select(room[:0], mode == ZERO)
        assert exp["count"] == 0
        for cap in (0, 7):
            for device in (True, False):
                out = Outs(torch, device, cap)
                rc = pb.lib().pire_hip_final_select(dev_room.data_ptr() if device else room.ctypes.data, 0, mode, pb.FLAG_ON_DEVICE if device else 0,
                                                    out.ptr("hits") if cap else None, cap, out.ptr("count"), stream_of(torch) if device else None)
                assert rc == 0, pb.lib().pire_hip_last_error()
                out.check(exp, (mode, cap, "device" if device else "host"))


@gpu
def test_the_pass_behind_the_final_flags_of_a_dfa_scan(torch_cuda):
    """out_final of pire_hip_run: the pass reads any flag array, whoever wrote it"""
    big = [b for b in H.big_sets() if b["name"] == "set_a"][0]
    blob = H.load_blob(big["blob"])
    strings = H.random_strings(np.random.RandomState(3), 1500, 120, b"abcdefgh 0123") + [bytes.fromhex(h) for h in big["witnesses_hex"]]
    text, offs = H.pack(strings)
    _, of = ob.OracleScanner(blob).run(text, offs, threads=2)
    _, gf = pb.Table(blob).run(text, offs)[:2]
    assert (gf == of).all() and 0 < np.count_nonzero(of) < len(strings)
    for invert in (False, True):
        w = pb.final_select_host(gf, invert=invert)
        exp = model_final_select(of, invert)
        assert w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all()


# ---- GPU: behind the slow scan's launch forms -----------------------------------------------------------------------------------

def run_form(torch, tab, device, batch_ptrs, n, flags, mode, cap, keep, strided=None):
    """the run + pass call; keep: the caller has out_final / out_state_bits (poisoned first)"""
    out = Outs(torch, device, cap, final=n if keep else 0, bits=n * tab.words if keep else 0)
    f = flags | (pb.FLAG_ON_DEVICE if device else 0)
    stream = stream_of(torch) if device else None
    if strided:
        rc = pb.lib().pire_hip_slow_run_select_strided(tab._h, batch_ptrs[0], n, strided[0], strided[1], f, mode, out.ptr("final"), out.ptr("bits"),
                                                       None, out.ptr("hits") if cap else None, cap, out.ptr("count"), stream)
    else:
        rc = pb.lib().pire_hip_slow_run_select(tab._h, batch_ptrs[0], batch_ptrs[1], n, f, mode, out.ptr("final"), out.ptr("bits"), None,
                                               out.ptr("hits") if cap else None, cap, out.ptr("count"), stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out


@gpu
@pytest.mark.parametrize("name", CASE_PARAMS)
def test_behind_the_slow_kernels(torch_cuda, name, cfg):
    torch = torch_cuda
    tab = pb.SlowTable(blob_of(name))
    text, offs = H.pack(batch(name))
    text, offs = text.copy(), offs.copy()
    n = len(offs) - 1
    dev_batch = (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))
    ptrs = {True: (dev_batch[0].data_ptr(), dev_batch[1].data_ptr()), False: (text.ctypes.data, offs.ctypes.data)}
    kernels = set()
    for no_list in (0, 1):
        cfg.set(slow_no_list=no_list)
        for flags in (BE, 0):
            of, obits = oracle_final(name, flags)
            pf, pbits = tab.run(text, offs, flags=flags)
            plain = pb.last_kernel()
            kernels.add(plain)
            assert (pf == of).all() and (pbits == obits).all()
            for mode in (0, ZERO):
                exp = model_final_select(of, mode == ZERO)
                for device in (True, False):
                    for keep in (True, False):
                        cap = n if keep else max(exp["count"] - 1, 0)
                        what = (name, no_list, flags, mode, "device" if device else "host", keep, cap)
                        out = run_form(torch, tab, device, ptrs[device], n, flags, mode, cap, keep)
                        assert pb.last_kernel() == plain, what
                        if keep:
                            out.check(exp, what, final=pf, bits=pbits)
                        else:
                            out.check(exp, what)
    wide = tab.words > 8
    assert kernels == {"slow_list", "slow_wide" if wide else "slow"}, kernels
    assert (dev_batch[0].cpu().numpy() == text).all() and (dev_batch[1].cpu().numpy().view(np.uint64) == offs).all()
    # the wrappers
    of, obits = oracle_final(name, BE)
    for invert in (False, True):
        exp = model_final_select(of, invert)
        w = tab.run_select_strings(batch(name), invert=invert)
        assert w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all() and (w["final"] == of).all() and (w["bits"] == obits).all()
        w = tab.run_select(text, offs, invert=invert, hit_cap=3, results=False)
        assert w["count"] == exp["count"] and (w["hits"] == exp["hits"][:3]).all() and "final" not in w
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        hits = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        tab.run_select_device(ptrs[True][0], ptrs[True][1], n, BE, cnt.data_ptr(), invert=invert, out_hits_ptr=hits.data_ptr(), hit_cap=n,
                              stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(cnt.cpu()[0]) == exp["count"] and (hits.cpu().numpy()[:exp["count"]] == exp["hits"].astype(np.int64)).all()
        assert (hits.cpu().numpy()[exp["count"]:] == -1).all()


@gpu
def test_the_strided_form(torch_cuda, cfg):
    """3 000 records of 128 bytes 144 apart (3 000 % 64 != 0), x.{40}$ planted in every third; the bytes between the records
    would match if they were read"""
    torch = torch_cuda
    name = "slow_x40_utf8"
    tab = pb.SlowTable(blob_of(name))
    n, length, stride = 3000, 128, 144
    assert n % 64 != 0
    rng = np.random.RandomState(3)
    data = rng.choice(u8(b"yzw abc"), size=(n, stride)).astype(np.uint8)
    data[::3, length - 41] = ord("x")
    data[1::3, stride - 41] = ord("x")                               # behind the record: 40 bytes in front of the NEXT record's begin
    records = [bytes(r[:length]) for r in data]
    flat = data.reshape(-1)[:(n - 1) * stride + length].copy()
    dev = torch.as_tensor(flat, device="cuda")
    for flags in (BE, 0):
        of, obits = ob.OracleSlowScanner(blob_of(name)).run_strings(records, flags=flags)
        if flags == BE:
            assert (np.flatnonzero(of) == np.arange(0, n, 3)).all()
        for no_list in (0, 1):
            cfg.set(slow_no_list=no_list)
            for mode in (0, ZERO):
                exp = model_final_select(of, mode == ZERO)
                for device in (True, False):
                    for keep in (True, False):
                        cap = n if keep else max(exp["count"] - 1, 0)
                        what = (no_list, flags, mode, device, keep, cap)
                        out = run_form(torch, tab, device, (dev.data_ptr() if device else flat.ctypes.data,), n, flags, mode, cap, keep, strided=(length, stride))
                        assert pb.last_kernel() == ("slow" if no_list else "slow_list"), what
                        if keep:
                            out.check(exp, what, final=of, bits=obits)
                        else:
                            out.check(exp, what)
    assert (dev.cpu().numpy() == flat).all()
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    hits = torch.zeros(n, dtype=torch.int64, device="cuda")
    tab.run_select_strided_device(dev.data_ptr(), n, length, stride, BE, cnt.data_ptr(), invert=True, out_hits_ptr=hits.data_ptr(), hit_cap=n,
                                  stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n - n // 3 and (hits.cpu().numpy()[:n - n // 3] == np.flatnonzero(np.arange(n) % 3 != 0)).all()


# ---- GPU: lines ---------------------------------------------------------------------------------------------------------------

LINES_CASES = [pytest.param(n, marks=needs_ref) if n in REF else n for n in ("slow_a30", "slow_alt", GOLDEN_WIDE, "ref_hello")]


def lines_call(torch, tab, device, raw, delim, flags, mode, cap, gather=None):
    """gather: None -- pire_hip_slow_lines_select --, or (tail, text_cap, with out_hits) -- pire_hip_slow_lines_gather"""
    keep = torch.as_tensor(raw, device="cuda") if device and len(raw) else raw
    rp = (keep.data_ptr() if device else keep.ctypes.data) if len(raw) else None
    f = flags | (pb.FLAG_ON_DEVICE if device else 0)
    if gather is None:
        out = Outs(torch, device, cap, spans=True, lines=True)
        rc = pb.lib().pire_hip_slow_lines_select(tab._h, rp, len(raw), delim, f, mode, out.ptr("lines"), out.ptr("hits") if cap else None,
                                                 out.ptr("spans") if cap else None, cap, out.ptr("count"), stream_of(torch))
    else:
        tail, text_cap, with_hits = gather
        out = Outs(torch, device, cap, hits=with_hits, lines=True, text=text_cap)
        rc = pb.lib().pire_hip_slow_lines_gather(tab._h, rp, len(raw), delim, f, mode, tail, out.ptr("lines"), out.ptr("hits") if cap else None,
                                                 cap, out.ptr("count"), out.ptr("text") if text_cap else None, text_cap, out.ptr("offsets"),
                                                 out.ptr("bytes"), stream_of(torch))
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out, keep


@gpu
@pytest.mark.parametrize("name", LINES_CASES)
def test_lines_in_matching_lines_out(torch_cuda, name):
    torch = torch_cuda
    tab = pb.SlowTable(blob_of(name))
    lines = lines_of(name)
    joined = b"\n".join(lines)
    buffers = [(u8(joined).copy(), 10), (u8(joined + b"\n").copy(), 10), (u8(b"\n" * 70).copy(), 10), (u8(b"").copy(), 10),
               (u8(b"|".join(lines) + b"|").copy(), ord("|"))]
    for raw, delim in buffers:
        d = bytes([delim])
        parts, spans = py_lines(raw, d)
        assert len(parts) == (0 if not len(raw) else 70 if raw[0] == 10 else len(lines))
        for flags in (BE, 0):
            fin = oracle_final(name, flags, strings=parts)[0] if parts else np.zeros(0, dtype=np.uint8)
            for mode in (0, ZERO):
                exp = model_final_select(fin, mode == ZERO)
                idx = exp["hits"].astype(np.int64)
                count = exp["count"]
                for device in (True, False):
                    for cap in sorted({len(parts), max(count - 1, 0)}):
                        what = (name, len(raw), delim, flags, mode, "device" if device else "host", cap)
                        k = min(count, cap)
                        out, keep = lines_call(torch, tab, device, raw, delim, flags, mode, cap)
                        now = out.check(exp, what, spans=spans[idx][:k], lines=np.array([len(parts)], dtype=np.uint64))
                        got = now["spans"][GUARD:GUARD + 16 * k].view(np.uint64).reshape(-1, 2)
                        assert [bytes(raw[b:e]) for b, e in got.tolist()] == [parts[i] for i in idx[:k].tolist()], what
                        # the bytes: tail = delim is grep's output (inverted: grep -v's); k lines where the list is short
                        want = b"".join(parts[i] + d for i in idx[:k].tolist())
                        ends = np.cumsum([0] + [len(parts[i]) + 1 for i in idx[:k].tolist()]).astype(np.uint64)
                        for with_hits in (True, False):
                            out, keep = lines_call(torch, tab, device, raw, delim, flags, mode, cap, gather=(delim, len(raw) + cap, with_hits))
                            out.check(exp, what, text=want, offsets=ends, bytes=np.array([len(want)], dtype=np.uint64),
                                      lines=np.array([len(parts)], dtype=np.uint64))
                        if device and len(raw):
                            assert (keep.cpu().numpy() == raw).all(), "the input was written to"
                # no tail, and a text_cap in the middle of a line: the whole total, the bytes in front of the cap
                if count and len(raw):
                    bare = b"".join(parts[i] for i in idx.tolist())
                    room = max(len(bare) - 3, 0)
                    out, _ = lines_call(torch, tab, True, raw, delim, flags, mode, len(parts), gather=(pb.NO_TAIL, room, True))
                    ends = np.cumsum([0] + [len(parts[i]) for i in idx.tolist()]).astype(np.uint64)
                    pad = np.concatenate([ends, np.zeros(0, np.uint64)])
                    out.check(exp, (name, "no tail", flags, mode), text=bare[:room], offsets=pad, bytes=np.array([len(bare)], dtype=np.uint64),
                              lines=np.array([len(parts)], dtype=np.uint64))
    # the wrappers: grep and grep -v of the buffer
    raw = u8(joined + b"\n")
    parts, spans = py_lines(raw)
    fin = oracle_final(name, BE, strings=parts)[0]
    for invert in (False, True):
        exp = model_final_select(fin, invert)
        w = tab.lines_select_host(raw, invert=invert)
        assert w["lines"] == len(parts) and w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all()
        assert (w["spans"] == spans[exp["hits"].astype(np.int64)]).all()
        g = tab.lines_gather_host(raw, invert=invert)
        want = b"".join(parts[i] + b"\n" for i in exp["hits"].tolist())
        assert g["text"].tobytes() == want and g["bytes"] == len(want) and g["count"] == exp["count"] and (g["hits"] == exp["hits"]).all()
    both = sorted(tab.lines_gather_host(raw)["text"].tobytes().split(b"\n")[:-1] + tab.lines_gather_host(raw, invert=True)["text"].tobytes().split(b"\n")[:-1])
    assert both == sorted(parts)
