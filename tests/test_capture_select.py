"""pire_hip_capture_select / pire_hip_capture_run_select / pire_hip_capture_lines_gather: from capture positions to the
captured substrings, on the device (capture_select.hip).

Exact equality everywhere.  The expected values come from `restate_capture_select` -- the formulas of include/pire_hip.h
written down with numpy -- applied, where a scan is involved, to what the C oracle's capture() says (tests/test_capture.py
holds that oracle against the unmodified reference), and for lines from tests/test_split.py's `restate` and
tests/test_gather.py's `restate_spans`.  Nothing expected comes from the library.  Every output buffer of a call sits
between poisoned guard zones, and whatever the call had no business writing is looked at afterwards."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H
from tests.test_capture_shapes import FLAGS, OWN_CHOICE, build_batch
from tests.test_gather import restate_spans
from tests.test_split import restate as restate_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TAIL = 0xFFFFFFFF
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8                      # poisoned words around every 64-bit output
GUARD_B = 64                   # poisoned bytes around out_text
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SHAPES = ("capture_kv", "capture_gap", "capture_rep", "capture_dotgap", "capture_ascii124", "capture_begin_mark")
LINES_OF = ("capture_kv", "capture_gap", "capture_rep")      # the fixtures of the lines tests: no newline in their strings
gpu = pytest.mark.gpu


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def restate_capture_select(offsets, begin, end, final, B, need_final, cap=None, shift=0):
    """include/pire_hip.h: (hits[k], spans[k, 2], count), k = min(count, cap); string i lies shift * i bytes further into
    the buffer the spans are counted in."""
    offsets = [int(x) for x in np.asarray(offsets).tolist()]
    begin, end = np.asarray(begin).tolist(), np.asarray(end).tolist()
    hits, spans = [], []
    for i in range(len(offsets) - 1):
        captured = begin[i] >= 0 and end[i] >= 0
        if not (captured and (not need_final or final[i] != 0)):
            continue
        ln = offsets[i + 1] - offsets[i]
        b = min(max(begin[i] - B, 0), ln)
        e = min(max(end[i] - B, b), ln)
        hits.append(i)
        spans.append((offsets[i] + b + shift * i, offsets[i] + e + shift * i))
    k = len(hits) if cap is None else min(len(hits), cap)
    return np.array(hits[:k], dtype=np.uint64), np.array(spans[:k], dtype=np.uint64).reshape(-1, 2), len(hits)


# ---- the fixtures and their batches (shared; the oracle runs once per fixture and flag combination) -------------------------

def case_of(name):
    g = H.golden()
    return [c for c in g["capturing"] + g["capturing_edge"] if c["name"] == name][0]


_batches, _oracle = {}, {}


def batch_of(name):
    """The strings the GPU tests run: tests/test_capture_shapes.py's build_batch; for capture_begin_mark, which has no
    alphabet of its own, the batch of that file's test_begin_capture_on_the_begin_mark_step."""
    if name not in _batches:
        case = case_of(name)
        if "alphabet_hex" in case:
            many = build_batch(case, 5)
        else:
            rng = np.random.RandomState(3)
            a = u8(b"ab1cc x")
            many = [bytes.fromhex(h) for h in case["strings_hex"]]
            for k in range(300):
                many += [b"1cc" + b"x" * (k % 7), b"", b"7cc" + bytes(a[rng.randint(0, len(a), size=k)])][:1 + k % 3]
            many += [bytes(a[rng.randint(0, len(a), size=int(rng.randint(0, 200)))]) for _ in range(600)]
        _batches[name] = many
    return _batches[name]


def oracle_capture(name, flags):
    """(text, offsets, final, begin, end) of the fixture's batch from the C oracle"""
    if (name, flags) not in _oracle:
        text, offs = H.pack(batch_of(name))
        o = ob.OracleCountingScanner(H.load_blob(case_of(name)["blob"]), 0)
        idx, fin, cap, b, e = o.capture(text, offs, flags=flags)
        for a in (fin, b, e):
            a.setflags(write=False)
        _oracle[(name, flags)] = (text, offs, fin, b, e)
    return _oracle[(name, flags)]


# ---- CPU -----------------------------------------------------------------------------------------------------------------

NAMES = ("pire_hip_capture_select", "pire_hip_capture_run_select", "pire_hip_capture_lines_gather")


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
    # the section sits behind pire_hip_capture_run and states the formulas
    assert src.index("int pire_hip_capture_run(") < src.index("the captured substrings, on the device") < src.index("int pire_hip_capture_select(")
    for formula in ("b_i         = clamp(begin[i] - B, 0, len_i)", "e_i         = clamp(end[i]   - B, b_i, len_i)"):
        assert formula in src


# rows of (length, begin, end) and what the span inside the string is for B = 0 and B = 1 (None: not captured)
HAND = [
    ((10, -1, 5), None, None),                 # begin unset
    ((10, 3, -1), None, None),                 # end unset
    ((10, -1, -1), None, None),
    ((10, 3, 7), (3, 7), (2, 6)),              # well-formed
    ((10, 0, 4), (0, 4), (0, 3)),              # begin == 0: under B = 1 the action fired on the BeginMark step, clamped to 0
    ((10, 6, 2), (6, 6), (5, 5)),              # end < begin: empty at b_i
    ((10, 4, 12), (4, 10), (3, 10)),           # end - B > len: clamped to len
    ((10, 4, 11), (4, 10), (3, 10)),           # end - B == len under B = 1: a capture that closes on the EndMark step
    ((10, 4, 10), (4, 10), (3, 9)),            # end - B == len under B = 0
    ((0, 1, 1), (0, 0), (0, 0)),               # an empty string
    ((0, 0, 0), (0, 0), (0, 0)),
    ((5, 9, 9), (5, 5), (5, 5)),               # begin behind the string
    ((5, I64_MAX, I64_MAX), (5, 5), (5, 5)),
    ((5, 1, I64_MAX), (1, 5), (0, 5)),
    ((5, I64_MIN, 3), None, None),
]


@pytest.mark.parametrize("need_final", (0, 1))
@pytest.mark.parametrize("B", (0, 1))
def test_restatement_on_hand_written_rows(B, need_final):
    lens = [r[0][0] for r in HAND]
    offs = np.concatenate([[7], 7 + np.cumsum(lens)]).astype(np.uint64)          # (the first string does not begin at 0)
    begin, end = [r[0][1] for r in HAND], [r[0][2] for r in HAND]
    final = [(i * 7 // 3) % 2 for i in range(len(HAND))]
    want_hits, want_spans = [], []
    for i, r in enumerate(HAND):
        inside = r[1 + B]
        if inside is not None and (not need_final or final[i]):
            want_hits.append(i)
            want_spans.append([int(offs[i]) + inside[0], int(offs[i]) + inside[1]])
    assert 0 < len(want_hits) < len(HAND)
    hits, spans, count = restate_capture_select(offs, begin, end, final, B, need_final)
    assert hits.tolist() == want_hits and spans.tolist() == want_spans and count == len(want_hits)
    for cap in (0, 1, count - 1, count + 1):
        h, s, c = restate_capture_select(offs, begin, end, final, B, need_final, cap=cap)
        assert c == count and h.tolist() == want_hits[:cap] and s.tolist() == want_spans[:cap]
    h, s, c = restate_capture_select(offs, begin, end, final, B, need_final, shift=1)
    assert s.tolist() == [[b + i, e + i] for i, (b, e) in zip(want_hits, want_spans)]
    for (b, e), i in zip(s.tolist(), h.tolist()):
        assert int(offs[i]) + i <= b <= e <= int(offs[i + 1]) + i              # a span never leaves its string


# What the reference's own unit test holds (tests/capture_ut.cpp of the reference: the line of the assertion, the string, the verdict)
REFERENCE_VERDICTS = {
    "capture_google": [(102, b"google_id = 'abcde';", b"abcde"),
                       (107, b"var google_id = 'abcde'; eval(google_id);", b"abcde"),
                       (111, b"google_id != 'abcde';", None),
                       (123, b"google_id = 'abcde'; google_id = 'xyz';", b"abcde"),
                       (128, b"var google_id = 'abc de'; google_id = 'xyz';", b"xyz")],
    "capture_digits": [(140, b"=12345;", b"12345")],
    "capture_path": [(152, b"/some/table/path/to-match-with", b"/to-match-with")],
}


def test_the_reference_held_verdicts():
    for name, rows in REFERENCE_VERDICTS.items():
        o = ob.OracleCountingScanner(H.load_blob(case_of(name)["blob"]), 0)
        strings = [s for _, s, _ in rows]
        text, offs = H.pack(strings)
        idx, fin, cap, b, e = o.capture(text, offs, flags=3)                     # RunRegexp: Begin(), Run(), End()
        hits, spans, count = restate_capture_select(offs, b, e, fin, 1, 0)
        got = {int(i): text[int(s0):int(s1)].tobytes() for i, (s0, s1) in zip(hits.tolist(), spans.tolist())}
        for i, (line, s, verdict) in enumerate(rows):
            assert got.get(i) == verdict, (name, line, s, got.get(i))
        assert count == sum(v is not None for _, _, v in rows)


def test_the_batches_of_the_gpu_tests_are_not_vacuous():
    """With the oracle alone: every fixture's batch has captured and uncaptured strings under each flag combination that
    captures at all; need_final changes some list; capture_begin_mark brings begin - B < 0."""
    captured_not_final = final_not_captured = 0
    for name in SHAPES:
        some = 0
        for flags in FLAGS:
            text, offs, fin, b, e = oracle_capture(name, flags)
            n = len(offs) - 1
            cap = (b >= 0) & (e >= 0)
            captured_not_final += int((cap & (fin == 0)).sum())               # need_final drops these from the list
            final_not_captured += int(((fin != 0) & ~cap).sum())              # Final alone does not select
            if not cap.any():
                continue
            some += 1
            assert 0 < cap.sum() < n, (name, flags, int(cap.sum()))
        # (capture_begin_mark never takes EndCapture: nothing of it is captured under any flags, and its lists are empty.  What
        # it brings is begin == 0 under BEGIN, the row the pass must clamp -- the synthetic arrays hold that row selected)
        assert some == (0 if name == "capture_begin_mark" else 4), (name, some)
        if name in LINES_OF:
            assert 10 not in set(np.unique(oracle_capture(name, 3)[0]).tolist()), "the fixture's strings hold the delimiter"
    b = oracle_capture("capture_begin_mark", 3)[3]
    assert ((b >= 0) & (b - 1 < 0)).sum() > 100
    assert captured_not_final > 0 and final_not_captured > 0, (captured_not_final, final_not_captured)


def _guarded():
    hits = np.full(8, POISON64, dtype=np.uint64)
    spans = np.full(16, POISON64, dtype=np.uint64)
    return hits, spans, C.c_uint64(77)


def test_capture_select_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    offs = np.array([0, 3, 6], dtype=np.uint64)
    b, e = np.array([1, 2], dtype=np.int64), np.array([2, 3], dtype=np.int64)
    f = np.array([1, 0], dtype=np.uint8)
    hits, spans, cnt = _guarded()
    o, bp, ep, fp, h, s, c = (offs.ctypes.data, b.ctypes.data, e.ctypes.data, f.ctypes.data, hits.ctypes.data, spans.ctypes.data,
                              C.addressof(cnt))
    cases = {
        "null out_hit_count": (o, 2, bp, ep, fp, 0, h, s, 4, None),
        "null offsets, begin or end": (None, 2, bp, ep, fp, 0, h, s, 4, c),
        "null offsets, begin or end ": (o, 2, None, ep, fp, 0, h, s, 4, c),
        "null offsets, begin or end  ": (o, 2, bp, None, fp, 0, h, s, 4, c),
        "need_final with null final": (o, 2, bp, ep, None, 1, h, s, 4, c),
        "hit_cap > 0 with null out_hits and null out_spans": (o, 2, bp, ep, fp, 0, None, None, 4, c),
        "2^32 strings or more": (o, 1 << 32, bp, ep, fp, 0, h, s, 4, c),
    }
    for what, (a_o, n, a_b, a_e, a_f, nf, a_h, a_s, cap, a_c) in cases.items():
        for flags in (0, 1, pb.FLAG_ON_DEVICE, pb.FLAG_ON_DEVICE | 1):
            assert L.pire_hip_capture_select(a_o, n, flags, a_b, a_e, a_f, nf, a_h, a_s, cap, a_c, None) == -1, what
            assert what.strip() in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    assert cnt.value == 77 and (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all()
    # no string at all, host pointers: a count of 0 and no device
    assert L.pire_hip_capture_select(None, 0, 0, None, None, None, 0, h, s, 4, c, None) == 0 and cnt.value == 0
    cnt.value = 77
    assert L.pire_hip_capture_select(o, 0, 1, bp, ep, fp, 1, None, None, 0, c, None) == 0 and cnt.value == 0
    assert (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all()


def test_capture_run_select_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    t = pb.CountingTable(H.load_blob(case_of("capture_digits")["blob"]), 0)
    text, offs = H.pack([b"=12345;", b"abc"])
    text, offs = text.copy(), offs.copy()
    hits, spans, cnt = _guarded()
    x, o, h, s, c = text.ctypes.data, offs.ctypes.data, hits.ctypes.data, spans.ctypes.data, C.addressof(cnt)
    cases = {
        "bad argument": (None, x, o, 2, 0, h, s, 4, c),                             # what pire_hip_capture_run refuses: no table,
        "bad argument ": (t._h, x, None, 2, 0, h, s, 4, c),                         # ... no offsets
        "null out_hit_count": (t._h, x, o, 2, 0, h, s, 4, None),
        "hit_cap > 0 with null out_hits and null out_spans": (t._h, x, o, 2, 1, None, None, 4, c),
        "2^32 strings or more": (t._h, x, o, 1 << 32, 0, h, s, 4, c),
    }
    for what, (a_t, a_x, a_o, n, nf, a_h, a_s, cap, a_c) in cases.items():
        for flags in (3, 3 | pb.FLAG_ON_DEVICE):
            assert L.pire_hip_capture_run_select(a_t, a_x, a_o, n, flags, nf, None, None, None, None, a_h, a_s, cap, a_c, None) == -1, what
            assert what.strip() in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    assert cnt.value == 77 and (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all()
    assert L.pire_hip_capture_run_select(t._h, None, o, 0, 3, 1, None, None, None, None, h, s, 4, c, None) == 0 and cnt.value == 0
    assert (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all()


def test_capture_lines_gather_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    t = pb.CountingTable(H.load_blob(case_of("capture_digits")["blob"]), 0)
    raw = u8(b"a=12345;\nabc\n").copy()
    hits, spans, cnt = _guarded()
    text = np.full(64, POISON, dtype=np.uint8)
    offs = np.full(16, POISON64, dtype=np.uint64)
    lines, total = C.c_uint64(78), C.c_uint64(79)
    r, lp, cp, h, s, tp, op, bp = (raw.ctypes.data, C.addressof(lines), C.addressof(cnt), hits.ctypes.data, spans.ctypes.data,
                                   text.ctypes.data, offs.ctypes.data, C.addressof(total))
    cases = {
        "null table": (None, r, raw.size, 10, 10, lp, h, s, 4, cp, tp, 64, op, bp),
        "delim > 255": (t._h, r, raw.size, 300, 10, lp, h, s, 4, cp, tp, 64, op, bp),
        "null out_line_count": (t._h, r, raw.size, 10, 10, None, h, s, 4, cp, tp, 64, op, bp),
        "size > 0 with null raw": (t._h, None, raw.size, 10, 10, lp, h, s, 4, cp, tp, 64, op, bp),
        "null out_hit_count": (t._h, r, raw.size, 10, 10, lp, h, s, 4, None, tp, 64, op, bp),
        "hit_cap > 0 with null out_hits and null out_spans": (t._h, r, raw.size, 10, 10, lp, None, None, 4, cp, None, 0, None, None),
        "null out_bytes": (t._h, r, raw.size, 10, 10, lp, h, s, 4, cp, tp, 64, op, None),
        "tail > 255": (t._h, r, raw.size, 10, 256, lp, h, s, 4, cp, tp, 64, op, bp),
        "idx_cap > 0 with null out_offsets": (t._h, r, raw.size, 10, 10, lp, h, s, 4, cp, tp, 64, None, bp),
        "text_cap > 0 with null out_text": (t._h, r, raw.size, 10, 10, lp, h, s, 4, cp, None, 64, op, bp),
        "overlaps": (t._h, r, raw.size, 10, 10, lp, h, s, 4, cp, r + 3, 64, op, bp),
    }
    for what, (a_t, a_r, size, delim, tail, a_l, a_h, a_s, cap, a_c, a_x, tcap, a_o, a_b) in cases.items():
        for flags in (3, 3 | pb.FLAG_ON_DEVICE):
            for nf in (0, 1):
                rc = L.pire_hip_capture_lines_gather(a_t, a_r, size, delim, flags, nf, tail, a_l, a_h, a_s, cap, a_c, a_x, tcap, a_o, a_b, None)
                assert rc == -1, what
                assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    assert (lines.value, cnt.value, total.value) == (78, 77, 79)
    assert (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all() and (text == POISON).all() and (offs == np.uint64(POISON64)).all()
    # host pointers, no byte at all: zeros, and no device
    assert L.pire_hip_capture_lines_gather(t._h, None, 0, 10, 3, 0, 10, lp, h, s, 4, cp, tp, 64, op, bp, None) == 0
    assert (lines.value, cnt.value, total.value) == (0, 0, 0) and offs.tolist() == [0] + [POISON64] * 15
    assert (hits == np.uint64(POISON64)).all() and (spans == np.uint64(POISON64)).all() and (text == POISON).all()
    lines.value, cnt.value = 78, 77
    assert L.pire_hip_capture_lines_gather(t._h, None, 0, 10, 3, 0, 10, lp, None, s, 4, cp, None, 0, None, None, None) == 0   # spans only
    assert (lines.value, cnt.value) == (0, 0) and (spans == np.uint64(POISON64)).all()


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """capture_select.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "capture_select.hip" in ba.NO_SCRATCH and "capture_select.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"^CAPSEL\s*:= capture_select\$\(suffix \.hip\)$", mk, re.M)) == 1 and mk.count("$(CAPSEL)") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("capture_select.hip")
    assert not fails, fails
    assert len(seen) == 2 and all("Capture" in k for k in seen), seen            # (the scan is select.hip's)


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


class Lists:
    """out_hits, out_spans and out_hit_count of one call, host or device, each between GUARD poisoned words."""

    def __init__(self, torch, device, cap, hits=True, spans=True):
        self.torch, self.device, self.cap = torch, device, cap
        self.host = {"hits": np.full(2 * GUARD + cap, POISON64, dtype=np.uint64) if hits else None,
                     "spans": np.full(2 * GUARD + 2 * cap, POISON64, dtype=np.uint64) if spans else None,
                     "count": np.full(2 * GUARD + 1, POISON64, dtype=np.uint64)}
        self.dev = {k: torch.as_tensor(i64(v), device="cuda") for k, v in self.host.items() if v is not None} if device else {}

    def ptr(self, name):
        if self.host[name] is None:
            return None
        return (self.dev[name].data_ptr() if self.device else self.host[name].ctypes.data) + 8 * GUARD

    def check(self, exp_hits, exp_spans, exp_count, what=""):
        """exp_*: the restatement with cap = None; the first min(count, cap) entries, and nothing else, were written"""
        if self.device:
            self.torch.cuda.synchronize()
        now = {k: (self.dev[k].cpu().numpy().view(np.uint64) if self.device else v) for k, v in self.host.items() if v is not None}
        c = now["count"]
        assert int(c[GUARD]) == exp_count, (what, "count", int(c[GUARD]), exp_count)
        assert (np.delete(c, GUARD) == np.uint64(POISON64)).all(), (what, "words around out_hit_count written")
        k = min(exp_count, self.cap)
        for name, width, exp in (("hits", 1, exp_hits), ("spans", 2, exp_spans)):
            if name not in now:
                continue
            a = now[name]
            got, want = a[GUARD:GUARD + width * k], np.asarray(exp[:k], dtype=np.uint64).reshape(-1)
            assert (got == want).all(), (what, name, np.flatnonzero(got != want)[:5], got[:6], want[:6])
            assert (a[:GUARD] == np.uint64(POISON64)).all() and (a[GUARD + width * k:] == np.uint64(POISON64)).all(), \
                (what, "out_%s written outside its first min(count, hit_cap) entries" % name)
        return now


# ---- GPU: the pass alone ---------------------------------------------------------------------------------------------------

PATTERNS = ("none", "all", "first_lane", "last_lane", "last_string", "wave_next_to_empty", "half", "thousandth")


def draw_selection(rng, n, pattern):
    i = np.arange(n)
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "first_lane": i % 64 == 0, "last_lane": i % 64 == 63,
            "last_string": i == n - 1, "wave_next_to_empty": (i // 64) % 2 == 1, "half": rng.rand(n) < 0.5,
            "thousandth": rng.rand(n) < 0.001}[pattern]


def synthetic(rng, n, sel, need_final):
    """offsets, begin, end, final in which exactly the strings of `sel` are selected; the positions run through every clamp
    row of the hand-written list, INT64_MIN and INT64_MAX included, the ways of not being selected through all of theirs."""
    lens = rng.randint(0, 24, size=n).astype(np.int64)
    lens[rng.rand(n) < 0.1] = 0
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    offs += np.uint64(5)
    kind = rng.randint(0, 8, size=n)
    inside = (rng.rand(n) * (lens + 2)).astype(np.int64)
    begin = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0, lens + 3, I64_MAX, 1], default=inside)
    more = (rng.rand(n) * 5).astype(np.int64)
    end = np.select([kind == 4, kind == 5, kind == 6, kind == 7], [np.maximum(begin - 2, 0), lens + 1, lens, I64_MAX], default=begin + more)
    end = np.where(kind == 2, I64_MAX - (more & 1), end)
    final = np.ones(n, dtype=np.uint8) if need_final else (rng.rand(n) < 0.5).astype(np.uint8)
    final[final != 0] = rng.randint(1, 256, size=int((final != 0).sum()))                     # (any non-zero byte is Final)
    out = rng.randint(0, 5 if need_final else 4, size=n)
    out[sel] = -1
    begin = np.where(out == 0, -1, np.where(out == 3, I64_MIN, begin))
    end = np.where(out == 1, -1, np.where(out == 2, I64_MIN, end))
    begin = np.where((out == 2) & (kind < 4), -1 - more, begin)
    final[out == 4] = 0
    return offs, begin.astype(np.int64), end.astype(np.int64), final


def run_pass(torch, device, inputs, dev_inputs, B, need_final, cap, hits, spans, stream=None, out=None):
    offs, begin, end, final = inputs
    n = len(offs) - 1
    out = out or Lists(torch, device, cap, hits, spans)
    if device:
        ptrs = [t.data_ptr() for t in dev_inputs]
    else:
        ptrs = [a.ctypes.data for a in inputs]
    flags = B | (pb.FLAG_ON_DEVICE if device else 0)
    rc = pb.lib().pire_hip_capture_select(ptrs[0], n, flags, ptrs[1] if n else None, ptrs[2] if n else None, (ptrs[3] or ptrs[0]) if need_final else None,   # (no string: a final nobody reads)
                                          need_final, out.ptr("hits"), out.ptr("spans"), cap, out.ptr("count"), stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out


SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1, (1 << 20) + 1025)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_on_synthetic_arrays(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.RandomState(1000 + n % 977)
    big = n > 4096                                          # the size that crosses a scan step's carry: fewer combinations
    calls = 0
    for pattern in (("half", "thousandth", "all", "last_string") if big else PATTERNS):
        for need_final in (0, 1):
            sel = draw_selection(rng, n, pattern)
            inputs = synthetic(rng, n, sel, need_final)
            before = [a.copy() for a in inputs]
            dev_inputs = [torch.as_tensor(i64(a) if a.dtype != np.uint8 else a, device="cuda") for a in inputs]
            for B in ((pattern == "half") & 1,) if big else (0, 1):
                eh, es, count = restate_capture_select(*inputs, B, need_final)
                assert count == int(sel.sum()) and (eh == np.flatnonzero(sel)).all()
                lo, hi = inputs[0][eh.astype(np.int64)], inputs[0][eh.astype(np.int64) + 1]
                assert ((lo <= es[:, 0]) & (es[:, 0] <= es[:, 1]) & (es[:, 1] <= hi)).all()
                caps = sorted({c for c in (0, 1, count - 1, count, count + 1, n) if c >= 0})
                if big:
                    caps = [count - 1, count] if pattern == "half" else [count + 1]
                for cap in caps:
                    for hits, spans in ((True, True),) if big else ((True, False), (False, True), (True, True)):
                        for device in (True,) if big and pattern != "thousandth" else (True, False):
                            what = (n, pattern, need_final, B, cap, hits, spans, "device" if device else "host")
                            first = run_pass(torch, device, inputs, dev_inputs, B, need_final, cap, hits, spans).check(eh, es, count, what)
                            calls += 1
                            if device and cap == count and hits and spans:      # the same input: the same bits
                                again = run_pass(torch, device, inputs, dev_inputs, B, need_final, cap, hits, spans).check(eh, es, count, what)
                                assert all(first[k].tobytes() == again[k].tobytes() for k in first)
            for a, b, d in zip(inputs, before, dev_inputs):
                assert (a == b).all() and (d.cpu().numpy().view(a.dtype) == b).all(), "an input was written to"
    assert calls >= (4 if n else 1)


# ---- GPU: behind the capture kernels -------------------------------------------------------------------------------------------

def run_select(torch, t, device, text, offs, flags, need_final, cap, positions, hits=True, spans=True, stream=None, dev_text=None, out=None):
    """pire_hip_capture_run_select; positions: the caller has out_state_idx / out_final / out_begin / out_end (poisoned first)"""
    n = len(offs) - 1
    out = out or Lists(torch, device, cap, hits, spans)
    pos = None
    if positions:
        pos = {"idx": np.full(n, 0xA5A5A5A5, dtype=np.uint32), "final": np.full(n, POISON, dtype=np.uint8),
               "begin": np.full(n, -77, dtype=np.int64), "end": np.full(n, -77, dtype=np.int64)}
        if device:
            pos = {k: torch.as_tensor(v, device="cuda") for k, v in pos.items()}
    p = (lambda k: None) if pos is None else (lambda k: pos[k].data_ptr() if device else pos[k].ctypes.data)
    if device:
        d_text, d_offs = dev_text if dev_text else (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))
        tp, op = d_text.data_ptr(), d_offs.data_ptr()
    else:
        tp, op = text.ctypes.data, offs.ctypes.data
    rc = pb.lib().pire_hip_capture_run_select(t._h, tp, op, n, flags | (pb.FLAG_ON_DEVICE if device else 0), need_final, p("idx"), p("final"),
                                              p("begin"), p("end"), out.ptr("hits"), out.ptr("spans"), cap, out.ptr("count"), stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    if pos is not None and device:
        torch.cuda.synchronize()
        pos = {k: v.cpu().numpy() for k, v in pos.items()}
    return out, pos


def test_the_fixtures_between_them_reach_every_kind_of_capture_kernel():
    """What test_behind_the_capture_kernels runs behind: the ragged kernel with actions, a dense per-lane kernel, and the
    letter + transition kernel (every fixture, under PIRE_HIP_RUN_GENERIC)"""
    assert {OWN_CHOICE[n] for n in SHAPES if n in OWN_CHOICE} == {"ragged_capture", "capture_dense", "capture"}


@gpu
@pytest.mark.parametrize("name", SHAPES)
def test_behind_the_capture_kernels(torch_cuda, cfg, name):
    torch = torch_cuda
    t = pb.CountingTable(H.load_blob(case_of(name)["blob"]), 0)
    reached = set()
    for flags in FLAGS:
        text, offs, fin, b, e = oracle_capture(name, flags)
        text, offs = text.copy(), offs.copy()
        n = len(offs) - 1
        dev_text = (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))
        for extra in (0, pb.FLAG_GENERIC):
            t.capture(text, offs, flags=flags | extra)
            alone = pb.last_kernel()                      # what pire_hip_capture_run alone reports for this call
            reached.add(alone)
            for need_final in (0, 1):
                eh, es, count = restate_capture_select(offs, b, e, fin, flags & 1, need_final)
                for device in (True, False):
                    for positions in (True, False):
                        for cap in (n,) if (positions or need_final) else (n, max(count - 1, 0)):
                            what = (name, flags, extra, need_final, "device" if device else "host", positions, cap)
                            out, pos = run_select(torch, t, device, text, offs, flags | extra, need_final, cap, positions, dev_text=dev_text)
                            out.check(eh, es, count, what)
                            assert pb.last_kernel() == alone, (what, pb.last_kernel(), alone)
                            if positions:
                                assert (pos["begin"] == b).all() and (pos["end"] == e).all() and ((pos["final"] != 0) == (fin != 0)).all(), what
            # spans without hits, the library keeping every position to itself
            eh, es, count = restate_capture_select(offs, b, e, fin, flags & 1, 0)
            run_select(torch, t, True, text, offs, flags | extra, 0, n, False, hits=False, dev_text=dev_text)[0].check(eh, es, count)
        assert (dev_text[0].cpu().numpy() == text).all() and (dev_text[1].cpu().numpy().view(np.uint64) == offs).all()
    # the library's own choice for 5 700 strings (tests/test_capture_shapes.py pins it per fixture) and, under
    # PIRE_HIP_RUN_GENERIC, `capture`: a table without a dense form (capture_dotgap) has that one kernel both ways
    own = {OWN_CHOICE[name]} if name in OWN_CHOICE else {"ragged_capture", "capture_dense"}
    assert "capture" in reached and reached - {"capture"} <= own and (reached != {"capture"} or own == {"capture"}), (reached, own)
    print("%s: reached %s" % (name, sorted(reached)))


# ---- GPU: lines -------------------------------------------------------------------------------------------------------------

def dev_capture_lines(torch, t, raw, flags, need_final=0, tail=-1, cap=None, text_cap=None, raw_off=0, hits=True, spans=True, gather=True):
    size = len(raw)
    cap = size if cap is None else cap
    text_cap = (size + cap if text_cap is None else text_cap) if gather else 0
    host = np.full(raw_off + size + 256, 10, dtype=np.uint8)
    host[raw_off:raw_off + size] = raw
    d = torch.as_tensor(host, device="cuda")
    assert d.data_ptr() % 256 == 0
    out = Lists(torch, True, cap, hits, spans)
    poison = int(np.uint64(POISON64).astype(np.int64))
    d_offs = torch.full((2 * GUARD + cap + 1,), poison, dtype=torch.int64, device="cuda")
    d_text = torch.full((GUARD_B + text_cap + GUARD_B,), POISON, dtype=torch.uint8, device="cuda")
    counts = torch.full((2 * GUARD + 2,), poison, dtype=torch.int64, device="cuda")
    t.capture_lines_gather_device(d.data_ptr() + raw_off if size else 0, size, flags, counts.data_ptr() + 8 * GUARD, out.ptr("count"),
                                  out_bytes_ptr=counts.data_ptr() + 8 * GUARD + 8 if gather else 0, need_final=need_final, tail=tail,
                                  out_hits_ptr=out.ptr("hits") or 0, out_spans_ptr=out.ptr("spans") or 0, hit_cap=cap,
                                  out_text_ptr=d_text.data_ptr() + GUARD_B if text_cap else 0, text_cap=text_cap,
                                  out_offsets_ptr=d_offs.data_ptr() + 8 * GUARD if gather else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == host).all(), "the input was written to"
    c, o, x = counts.cpu().numpy().view(np.uint64), d_offs.cpu().numpy().view(np.uint64), d_text.cpu().numpy()
    assert (c[:GUARD] == np.uint64(POISON64)).all() and (c[GUARD + 2:] == np.uint64(POISON64)).all()
    return out, {"lines": int(c[GUARD]), "bytes": int(c[GUARD + 1]), "offsets": o, "text": x, "text_cap": text_cap}


def check_lines(out, got, raw, exp, tail_byte, cap, gather=True, what=""):
    """exp: (lines, hits, spans, count) from the two restatements; the gather outputs against restate_spans"""
    lines, eh, es, count = exp
    assert got["lines"] == lines, what
    out.check(eh, es, count, what)
    o, x = got["offsets"], got["text"]
    k = min(count, cap)
    if not gather:
        assert (o == np.uint64(POISON64)).all() and (x == POISON).all() and got["bytes"] == POISON64, what
        return
    et, eo, total = restate_spans(raw, es[:k], tail=tail_byte)
    assert got["bytes"] == total, (what, got["bytes"], total)
    assert (o[GUARD:GUARD + k + 1] == eo).all(), what
    assert (o[:GUARD] == np.uint64(POISON64)).all() and (o[GUARD + k + 1:] == np.uint64(POISON64)).all(), (what, "out_offsets written outside entries 0..k")
    written = min(total, got["text_cap"])
    assert (x[GUARD_B:GUARD_B + written] == et[:written]).all(), what
    assert (x[:GUARD_B] == POISON).all() and (x[GUARD_B + written:] == POISON).all(), (what, "bytes around out_text written")


def expected_lines(name, raw, flags, need_final):
    """The split's restatement, the oracle on its lines, the pass's restatement with shift = 1: spans are ranges of raw"""
    text, offs, n = restate_split(raw)
    o = ob.OracleCountingScanner(H.load_blob(case_of(name)["blob"]), 0)
    if n:
        idx, fin, cap, b, e = o.capture(text, offs, flags=flags)
    else:
        fin, b, e = np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64)
    eh, es, count = restate_capture_select(offs, b, e, fin, flags & 1, need_final, shift=1)
    for (s0, s1), i in zip(es.tolist(), eh.tolist()):                             # (the shift is right: the bytes are the line's)
        assert raw[s0:s1].tobytes() == text[s0 - i:s1 - i].tobytes() and 10 not in raw[s0:s1]
    return n, eh, es, count


@gpu
@pytest.mark.parametrize("name", LINES_OF)
def test_lines_in_captured_fields_out(torch_cuda, name):
    torch = torch_cuda
    T = pb.SPLIT_TILE
    t = pb.CountingTable(H.load_blob(case_of(name)["blob"]), 0)
    strings = batch_of(name)
    assert not any(b"\n" in s for s in strings), "the fixture's alphabet holds the delimiter"
    assert b"" in strings                                                        # consecutive newlines
    raw = u8(b"\n".join(strings)).copy()                                      # no newline behind the last line
    assert raw[-1] != 10 and b"\n\n" in raw.tobytes()
    nl = np.flatnonzero(raw == 10)
    for raw_off in (0, 1, 15):                                                   # a line that straddles a tile of the split
        starts, ends = np.concatenate([[0], nl + 1]) + raw_off, np.concatenate([nl, [len(raw)]]) + raw_off
        assert ((starts // T) != ((ends - 1) // T)).any()
    for flags in (3, 0):
        for need_final in (0, 1):
            exp = expected_lines(name, raw, flags, need_final)
            count = exp[3]
            assert 0 < count < exp[0]
            for raw_off, tail, tb in ((0, -1, 10), (1, 0, 0), (15, None, None)):
                what = (name, flags, need_final, raw_off, tail)
                out, got = dev_capture_lines(torch, t, raw, flags, need_final, tail=tail, raw_off=raw_off)
                check_lines(out, got, raw, exp, tb, len(raw), what=what)
            if need_final:
                continue
            total = restate_spans(raw, exp[2], tail=10)[2]
            for text_cap in (0, 1, total - 1, total // 2):
                out, got = dev_capture_lines(torch, t, raw, flags, tail=-1, text_cap=text_cap, raw_off=1)
                check_lines(out, got, raw, exp, 10, len(raw), what=("text_cap", text_cap))
            for cap in (count - 3, 1, 0):
                out, got = dev_capture_lines(torch, t, raw, flags, tail=-1, cap=cap, raw_off=15, hits=cap % 2 == 0)
                check_lines(out, got, raw, exp, 10, cap, what=("cap", cap))
            # spans only: no gather output at all; and the library keeping both lists to itself
            out, got = dev_capture_lines(torch, t, raw, flags, gather=False, hits=False)
            check_lines(out, got, raw, exp, None, len(raw), gather=False)
            out, got = dev_capture_lines(torch, t, raw, flags, hits=False, spans=False, tail=None)
            check_lines(out, got, raw, exp, None, len(raw))
            # host pointers: the same answer
            g = t.capture_lines_gather_host(raw, flags=flags, tail=-1)
            et, eo, total = restate_spans(raw, exp[2], tail=10)
            assert (g["lines"], g["count"], g["bytes"]) == (exp[0], count, total)
            assert (g["hits"] == exp[1]).all() and (g["spans"] == exp[2]).all() and (g["offsets"] == eo).all() and (g["text"] == et).all()
            g = t.capture_lines_gather_host(raw, flags=flags, tail=None, hit_cap=5, text_cap=7)
            et, eo, total = restate_spans(raw, exp[2][:5], tail=None)
            assert (g["count"], g["bytes"]) == (count, total) and (g["spans"] == exp[2][:5]).all() and (g["text"] == et[:7]).all()
            g = t.capture_lines_gather_host(raw, flags=flags, gather=False)
            assert (g["hits"] == exp[1]).all() and (g["spans"] == exp[2]).all()
    # a trailing newline, nothing but newlines, nothing
    for other in (np.concatenate([raw[:3000], u8(b"\n")]), u8(b"\n\n\n"), np.zeros(0, dtype=np.uint8)):
        exp = expected_lines(name, other, 3, 0)
        out, got = dev_capture_lines(torch, t, other, 3, cap=8, text_cap=32)
        check_lines(out, got, other, exp, 10, 8)


@gpu
def test_the_spans_of_the_pass_fed_to_gather_spans_by_the_caller(torch_cuda):
    """pire_hip_capture_run_select on the split lines, its spans shifted by the caller, pire_hip_gather_spans: what the fused call wrote"""
    torch = torch_cuda
    name = "capture_kv"
    t = pb.CountingTable(H.load_blob(case_of(name)["blob"]), 0)
    raw = u8(b"\n".join(batch_of(name)) + b"\n").copy()
    out, fused = dev_capture_lines(torch, t, raw, 3, tail=-1)
    text, offs, n = pb.split_host(raw)
    res = t.capture_select(text, offs, flags=3, positions=True)
    hits, spans, count = pb.capture_select_host(offs, res["begin"], res["end"], res["final"], flags=pb.FLAG_BEGIN)
    assert count == res["count"] and (hits == res["hits"]).all() and (spans == res["spans"]).all()
    in_raw = spans + hits[:, None]                                               # line i lies i bytes further into raw
    g_text, g_offs, g_total = pb.gather_host(raw, spans=in_raw, tail=10)
    now = out.check(res["hits"], in_raw, count)
    assert fused["bytes"] == g_total and (fused["offsets"][GUARD:GUARD + count + 1] == g_offs).all()
    assert (fused["text"][GUARD_B:GUARD_B + g_total] == g_text).all()
    exp = expected_lines(name, raw, 3, 0)
    check_lines(out, fused, raw, exp, 10, len(raw))


# ---- GPU: enqueue-only ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("which", ("capture_select", "capture_run_select"))
def test_an_on_device_call_only_enqueues(torch_cuda, cfg, which):
    """pire_hip_capture_select / pire_hip_capture_run_select (table uploaded, 5 700 strings, every position array in the
    library's own scratch) on a side stream behind a long-running scan: back on the host before that scan has finished
    (the method of tests/test_select.py and tests/test_gather.py)."""
    torch = torch_cuda
    cfg.set(auto_adapt=1)
    big = [b for b in H.big_sets() if b["name"] == "set_a"][0]
    long_table = pb.Table(H.load_blob(big["blob"]))
    long_table.upload()
    name = "capture_kv"
    t = pb.CountingTable(H.load_blob(case_of(name)["blob"]), 0)
    text, offs, fin, b, e = oracle_capture(name, 3)
    text, offs = text.copy(), offs.copy()
    n = len(offs) - 1
    assert n >= 256
    eh, es, count = restate_capture_select(offs, b, e, fin, 1, 0)
    inputs = (offs, np.array(b), np.array(e), np.array(fin))
    dev_inputs = [torch.as_tensor(i64(a) if a.dtype != np.uint8 else a, device="cuda") for a in inputs]
    dev_text = (torch.as_tensor(text, device="cuda"), dev_inputs[0])
    side = torch.cuda.Stream()

    def call(out):
        if which == "capture_select":
            return run_pass(torch, True, inputs, dev_inputs, 1, 0, n, True, True, stream=side.cuda_stream, out=out)
        return run_select(torch, t, True, text, offs, 3, 0, n, False, dev_text=dev_text, stream=side.cuda_stream, out=out)[0]

    # first use: the table's upload and self-test, the kernels' code objects, the pool's warm-up
    call(Lists(torch, True, n)).check(eh, es, count)
    ln, llen = 64, 8 << 20
    long_text = torch.empty((ln, llen), dtype=torch.uint8, device="cuda")
    pire_amd.corpus_fill_device(long_text.data_ptr(), 5, 0, ln, llen, llen, H.plants_for(big), torch.cuda.current_stream().cuda_stream)
    lidx = torch.empty(ln, dtype=torch.int32, device="cuda")
    out = Lists(torch, True, n)               # every buffer of the call under test is there before the long scan starts
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    long_table.run_strided_device(long_text.data_ptr(), ln, llen, llen, 3 | pb.FLAG_GENERIC, lidx.data_ptr(), 0, 0, 0, side.cuda_stream)
    done.record(side)
    t0 = time.perf_counter()
    call(out)
    returned = time.perf_counter() - t0
    still_running = not done.query()
    side.synchronize()
    assert still_running, "the call came back only after the scan in front of it had finished (%.1f ms)" % (returned * 1e3)
    out.check(eh, es, count)


# ---- the C++ shim ---------------------------------------------------------------------------------------------------------------

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
SHIM_BIN = os.path.join(REF_DIR, "bin", "capture_lines_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "extra.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present (GPU box): the prebuilt binary is used there")
def test_capture_lines_program_compiles_against_reference_headers():
    """tests/cpp/capture_lines_test.cpp with the flags oracle/Makefile gives tests/cpp/shim_test.cpp, next to it in oracle/_ref/bin"""
    ob.build()
    r = H.make_shim_program("capture_lines_test")
    assert r.returncode == 0, r.stdout[-3000:]
    assert os.path.exists(SHIM_BIN)


@gpu
def test_capture_batch_runner_matches_the_reference_line_by_line():
    """CaptureBatchRunner::RunLines(...).CapturedText() against Pire::CapturingScanner run line by line through <pire/extra.h>"""
    if not os.path.exists(SHIM_BIN):
        pytest.skip("oracle/_ref/bin/capture_lines_test was not built (needs the reference tree at build time)")
    r = subprocess.run([SHIM_BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(capture lines" in r.stdout
