"""pire_hip_gather / pire_hip_gather_spans / pire_hip_run_lines_gather: the listed strings of a batch back to back, on the
device (gather.hip).

Exact equality everywhere.  The expected values come from `restate_gather` -- the formulas of include/pire_hip.h written
down with numpy -- and, where a scan is involved, from the C oracle on the lines tests/test_split.py's `restate` produces.
Nothing expected comes from the library.  Every output buffer of a call sits between poisoned guard zones, and whatever
the call had no business writing is looked at afterwards."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16384                      # PIRE_HIP_GATHER_TILE_BYTES (the CPU tests hold the header and the binding against it)
NO_TAIL = 0xFFFFFFFF
BE = pb.FLAG_BEGIN | pb.FLAG_END
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
FILL = 0x5A                    # around the source: a byte read from there and used shows up
GUARD = 8                      # poisoned words around out_offsets and out_bytes
GUARD_B = 64                   # poisoned bytes around out_text (a multiple of 16: out_off is out_text's address modulo 16)
gpu = pytest.mark.gpu


# ---- the restatement ---------------------------------------------------------------------------------------------------

def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def batch(strings):
    """text u8, offsets u64[n + 1] of a list of bytes"""
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return u8(b"".join(strings)).copy(), offs


def restate_ranges(src, ranges, tail):
    """(out_text, out_offsets, total) of the source ranges [(begin, end)] in that order, `tail` (None: no byte) behind each"""
    src = np.asarray(src, dtype=np.uint8).tobytes()
    t = b"" if tail is None else bytes([tail])
    pieces = [src[b:e] + t for b, e in ranges]
    offs = np.zeros(len(pieces) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
    return u8(b"".join(pieces)), offs, int(offs[-1])


def restate_gather(text, offsets, idx=None, count=None, cap=None, tail=None):
    """include/pire_hip.h: k = min(count, cap) strings, string j from s_j = idx[j] (idx None: j); an s_j >= n is an empty
    string (the ON_DEVICE form; the host form refuses it)."""
    n = len(offsets) - 1
    cap = (n if idx is None else len(idx)) if cap is None else cap
    k = min(cap if count is None else count, cap)
    src = [j if idx is None else int(idx[j]) for j in range(k)]
    ranges = [(int(offsets[s]), int(offsets[s + 1])) if s < n else (0, 0) for s in src]
    return restate_ranges(text, ranges, tail)


def restate_spans(raw, spans, count=None, cap=None, tail=None):
    spans = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    cap = len(spans) if cap is None else cap
    k = min(cap if count is None else count, cap)
    ranges = [(int(b), int(e)) if b <= e <= len(raw) else (0, 0) for b, e in spans[:k].tolist()]
    return restate_ranges(raw, ranges, tail)


# ---- CPU -----------------------------------------------------------------------------------------------------------------

def test_restatement_on_hand_written_cases():
    for tail, t in ((None, b""), (10, b"\n"), (0, b"\0")):
        for strings in ([], [b""], [b"a"], [b"", b"", b"x", b""]):
            text, offs = batch(strings)
            out, oo, total = restate_gather(text, offs, tail=tail)               # idx = None: every string, in order
            assert out.tobytes() == b"".join(s + t for s in strings) and total == len(out)
            assert oo.tolist() == [sum(len(s) + len(t) for s in strings[:j]) for j in range(len(strings) + 1)]
        strings = [b"ab", b"", b"cde", b"f"]
        text, offs = batch(strings)
        for idx in ([3, 2, 1, 0], [2, 2, 0, 2], [1], []):                            # descending, duplicates
            out, oo, total = restate_gather(text, offs, idx=idx, tail=tail)
            assert out.tobytes() == b"".join(strings[i] + t for i in idx) and int(oo[-1]) == total == len(out) and len(oo) == len(idx) + 1
        out, oo, total = restate_gather(text, offs, idx=[0, 9, 2], tail=tail)         # out of range: an empty string and its tail
        assert out.tobytes() == b"ab" + t + t + b"cde" + t
        out, oo, total = restate_gather(text, offs, idx=[0, 2, 3], count=2, tail=tail)
        assert out.tobytes() == b"ab" + t + b"cde" + t and len(oo) == 3
        out, oo, total = restate_gather(text, offs, idx=[0, 2, 3], count=7, cap=1, tail=tail)
        assert out.tobytes() == b"ab" + t and len(oo) == 2
        out, oo, total = restate_spans(u8(b"hello world"), [[6, 11], [0, 5], [5, 4], [3, 12]], tail=tail)
        assert out.tobytes() == b"world" + t + b"hello" + t + t + t


def test_the_library_exports_the_gather_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    for name in ("pire_hip_gather", "pire_hip_gather_spans", "pire_hip_run_lines_gather"):
        assert hasattr(L, name), name
        assert name in {n for n, _, _ in pb.ABI}
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        src = f.read()
    assert int(re.search(r"#define PIRE_HIP_GATHER_TILE_BYTES (\d+)u", src).group(1)) == pb.GATHER_TILE == T == 16384
    assert re.search(r"#define PIRE_HIP_GATHER_NO_TAIL \(~0u\)", src) and pb.NO_TAIL == NO_TAIL


def _poisoned():
    text = np.full(64, POISON, dtype=np.uint8)
    offs = np.full(16, POISON64, dtype=np.uint64)
    total = C.c_uint64(77)
    return text, offs, total


def test_gather_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    src, so = batch([b"ab", b"cd", b"", b"efg"])
    src, so = src.copy(), so.copy()
    idx = np.array([3, 0, 1], dtype=np.uint64)
    cnt = C.c_uint64(3)
    text, offs, total = _poisoned()
    s, o, i, c, tp, op, bp = src.ctypes.data, so.ctypes.data, idx.ctypes.data, C.addressof(cnt), text.ctypes.data, offs.ctypes.data, C.addressof(total)
    cases = {
        "null out_bytes": (s, o, 4, i, c, 3, 10, tp, 64, op, None),
        "tail > 255": (s, o, 4, i, c, 3, 256, tp, 64, op, bp),
        "idx_cap > 0 with null offsets": (s, None, 4, i, c, 3, 10, tp, 64, op, bp),
        "idx_cap > 0 with null out_offsets": (s, o, 4, i, c, 3, 10, tp, 64, None, bp),
        "text_cap > 0 with null out_text": (s, o, 4, i, c, 3, 10, None, 64, op, bp),
        "idx_cap > n without idx": (s, o, 4, None, c, 5, 10, tp, 64, op, bp),
        "2^32 strings or more": (s, o, 4, i, c, 1 << 32, 10, tp, 64, op, bp),
    }
    for what, (a_s, a_o, n, a_i, a_c, cap, tail, a_t, tcap, a_oo, a_b) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_gather(a_s, a_o, n, a_i, a_c, cap, tail, flags, a_t, tcap, a_oo, a_b, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    # host pointers: an index out of range, and an out_text inside the source -- the text at addresses nobody owns (the
    # call must not touch it; the offsets are the host's to read)
    bad = np.array([0, 4, 1], dtype=np.uint64)
    assert L.pire_hip_gather(s, o, 4, bad.ctypes.data, c, 3, 10, 0, tp, 64, op, bp, None) == -1
    assert "out of range" in L.pire_hip_last_error().decode()
    wide = np.array([0, 1000, 2000, 4096], dtype=np.uint64)
    for a_s, a_t in ((0x7000000000, 0x7000000000), (0x7000000000, 0x7000000000 + 4095), (0x7000000000 + 63, 0x7000000000)):
        assert L.pire_hip_gather(a_s, wide.ctypes.data, 3, None, None, 3, NO_TAIL, 0, a_t, 64, op, bp, None) == -1
        assert "overlaps" in L.pire_hip_last_error().decode()
    assert total.value == 77 and (text == POISON).all() and (offs == np.uint64(POISON64)).all()


def test_gather_spans_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"hello world, hello gather").copy()
    spans = np.array([[0, 5], [6, 11]], dtype=np.uint64)
    cnt = C.c_uint64(2)
    text, offs, total = _poisoned()
    r, sp, c, tp, op, bp = raw.ctypes.data, spans.ctypes.data, C.addressof(cnt), text.ctypes.data, offs.ctypes.data, C.addressof(total)
    cases = {
        "null out_bytes": (r, raw.size, sp, c, 2, 10, tp, 64, op, None),
        "tail > 255": (r, raw.size, sp, c, 2, 1000, tp, 64, op, bp),
        "span_cap > 0 with null spans": (r, raw.size, None, c, 2, 10, tp, 64, op, bp),
        "idx_cap > 0 with null out_offsets": (r, raw.size, sp, c, 2, 10, tp, 64, None, bp),
        "text_cap > 0 with null out_text": (r, raw.size, sp, c, 2, 10, None, 64, op, bp),
        "2^32 strings or more": (r, raw.size, sp, c, 1 << 32, 10, tp, 64, op, bp),
        "overlaps": (r, raw.size, sp, c, 2, 10, r + raw.size - 1, 64, op, bp),
    }
    for what, (a_r, size, a_sp, a_c, cap, tail, a_t, tcap, a_oo, a_b) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_gather_spans(a_r, size, a_sp, a_c, cap, tail, flags, a_t, tcap, a_oo, a_b, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    for a_r, a_t in ((0x7000000000, 0x7000000000), (0x7000000000, 0x7000000000 + 4095), (0x7000000000 + 63, 0x7000000000)):
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_gather_spans(a_r, 4096, sp, c, 2, NO_TAIL, flags, a_t, 64, op, bp, None) == -1
            assert "overlaps" in L.pire_hip_last_error().decode()
    for bad in ([[0, 5], [7, 6]], [[0, 5], [6, raw.size + 1]]):                       # host pointers: a span out of range
        b = np.array(bad, dtype=np.uint64)
        assert L.pire_hip_gather_spans(r, raw.size, b.ctypes.data, c, 2, 10, 0, tp, 64, op, bp, None) == -1
        assert "out of range" in L.pire_hip_last_error().decode()
    assert total.value == 77 and (text == POISON).all() and (offs == np.uint64(POISON64)).all()


def test_run_lines_gather_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    t = pb.Table(H.load_blob("c2_single.blob"))
    raw = u8(b"hello  world\nabc\n").copy()
    hits = np.full(4, POISON64, dtype=np.uint64)
    text, offs, total = _poisoned()
    lines, cnt = C.c_uint64(78), C.c_uint64(79)
    r, lp, cp, h, tp, op, bp = raw.ctypes.data, C.addressof(lines), C.addressof(cnt), hits.ctypes.data, text.ctypes.data, offs.ctypes.data, C.addressof(total)
    cases = {
        "null table": (None, r, raw.size, 10, 10, lp, h, 4, cp, tp, 64, op, bp),
        "delim > 255": (t._h, r, raw.size, 300, 10, lp, h, 4, cp, tp, 64, op, bp),
        "null out_line_count": (t._h, r, raw.size, 10, 10, None, h, 4, cp, tp, 64, op, bp),
        "size > 0 with null raw": (t._h, None, raw.size, 10, 10, lp, h, 4, cp, tp, 64, op, bp),
        "null out_hit_count": (t._h, r, raw.size, 10, 10, lp, h, 4, None, tp, 64, op, bp),
        "null out_bytes": (t._h, r, raw.size, 10, 10, lp, h, 4, cp, tp, 64, op, None),
        "tail > 255": (t._h, r, raw.size, 10, 256, lp, h, 4, cp, tp, 64, op, bp),
        "idx_cap > 0 with null out_offsets": (t._h, r, raw.size, 10, 10, lp, h, 4, cp, tp, 64, None, bp),
        "text_cap > 0 with null out_text": (t._h, r, raw.size, 10, 10, lp, h, 4, cp, None, 64, op, bp),
        "overlaps": (t._h, r, raw.size, 10, 10, lp, h, 4, cp, r + 3, 64, op, bp),
    }
    for what, (th, a_r, size, delim, tail, a_l, a_h, cap, a_c, a_t, tcap, a_oo, a_b) in cases.items():
        for flags in (BE, BE | pb.FLAG_ON_DEVICE):
            assert L.pire_hip_run_lines_gather(th, a_r, size, delim, flags, None, tail, a_l, a_h, cap, a_c, a_t, tcap, a_oo, a_b, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    for flags in (BE, BE | pb.FLAG_ON_DEVICE):
        assert L.pire_hip_run_lines_gather(t._h, 0x7000000000, 4096, 10, flags, None, 10, lp, h, 4, cp, 0x7000000000 + 4095, 64, op, bp, None) == -1
        assert "overlaps" in L.pire_hip_last_error().decode()
    assert (lines.value, cnt.value, total.value) == (78, 79, 77)
    assert (text == POISON).all() and (offs == np.uint64(POISON64)).all() and (hits == np.uint64(POISON64)).all()
    # an empty buffer is answered without a device
    assert L.pire_hip_run_lines_gather(t._h, None, 0, 10, BE, None, 10, lp, h, 4, cp, tp, 64, op, bp, None) == 0
    assert (lines.value, cnt.value, total.value) == (0, 0, 0) and offs.tolist() == [0] + [POISON64] * 15 and (text == POISON).all()


def test_an_empty_list_is_answered_without_a_device():
    L = pb.lib()
    src, so = batch([b"ab", b"cd"])
    src, so = src.copy(), so.copy()
    idx = np.array([1, 0], dtype=np.uint64)
    spans = np.array([[0, 2], [2, 4]], dtype=np.uint64)
    zero = C.c_uint64(0)
    for cap, count in ((0, None), (2, C.addressof(zero)), (0, C.addressof(zero))):
        for tail in (NO_TAIL, 10):
            text, offs, total = _poisoned()
            assert L.pire_hip_gather(src.ctypes.data, so.ctypes.data, 2, idx.ctypes.data, count, cap, tail, 0, text.ctypes.data, 64,
                                     offs.ctypes.data, C.byref(total), None) == 0
            assert total.value == 0 and offs.tolist() == [0] + [POISON64] * 15 and (text == POISON).all()
            text, offs, total = _poisoned()
            assert L.pire_hip_gather_spans(src.ctypes.data, 4, spans.ctypes.data, count, cap, tail, 0, text.ctypes.data, 64,
                                           offs.ctypes.data, C.byref(total), None) == 0
            assert total.value == 0 and offs.tolist() == [0] + [POISON64] * 15 and (text == POISON).all()
    total = C.c_uint64(5)
    assert L.pire_hip_gather(None, None, 0, None, None, 0, NO_TAIL, 0, None, 0, None, C.byref(total), None) == 0 and total.value == 0


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_gather_unit_passes_the_build_audit():
    """gather.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "gather.hip" in ba.NO_SCRATCH and "gather.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        assert f.read().count("gather.hip") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("gather.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Gather" in k for k in seen), seen


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class Call:
    """One pire_hip_gather / pire_hip_gather_spans call, with host pointers or on the device.  The source sits src_off bytes
    into an aligned allocation among FILL bytes, out_text GUARD_B + out_off bytes into a poisoned one with GUARD_B poisoned
    bytes behind its text_cap bytes, out_offsets and out_bytes between GUARD poisoned words.  run() gives the return code;
    check() compares everything -- outputs, guards, the inputs -- with what the restatement says."""

    def __init__(self, torch, mode, src, offsets=None, idx=None, spans=None, count=None, cap=None, tail=None, text_cap=0,
                 src_off=0, out_off=0):
        self.torch, self.mode, self.device = torch, mode, mode == "device"
        src = np.asarray(src, dtype=np.uint8)
        self.size, self.src_off, self.out_off, self.text_cap, self.tail = len(src), src_off, out_off, text_cap, tail
        self.n = 0 if offsets is None else len(offsets) - 1
        self.is_spans = spans is not None
        self.cap = (len(spans) if self.is_spans else self.n if idx is None else len(idx)) if cap is None else cap
        img = np.full(src_off + self.size + 64, FILL, dtype=np.uint8)
        img[src_off:src_off + self.size] = src
        self.host = {"src": img,
                     "out": np.full(GUARD_B + out_off + text_cap + GUARD_B, POISON, dtype=np.uint8),
                     "offs": np.full(GUARD + self.cap + 1 + GUARD, POISON64, dtype=np.uint64),
                     "bytes": np.full(2 * GUARD + 1, POISON64, dtype=np.uint64)}
        if offsets is not None:
            self.host["offsets"] = np.ascontiguousarray(offsets, dtype=np.uint64)
        if idx is not None:
            self.host["idx"] = np.ascontiguousarray(idx, dtype=np.uint64)
        if spans is not None:
            self.host["spans"] = np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
        if count is not None:
            self.host["count"] = np.array([count], dtype=np.uint64)
        self.before = {k: v.copy() for k, v in self.host.items()}
        self.dev = {}
        if self.device:
            for k, v in self.host.items():
                if v.size:
                    self.dev[k] = torch.as_tensor(v.view(np.uint8), device="cuda")
                    assert self.dev[k].data_ptr() % 256 == 0

    def ptr(self, name, byte_off=0):
        a = self.host.get(name)
        if a is None or a.size == 0:
            return None
        return (self.dev[name].data_ptr() if self.device else a.ctypes.data) + byte_off

    def run(self, stream=None):
        flags = pb.FLAG_ON_DEVICE if self.device else 0
        tail = NO_TAIL if self.tail is None else self.tail
        outs = (self.ptr("out", GUARD_B + self.out_off) if self.text_cap else None, self.text_cap, self.ptr("offs", 8 * GUARD),
                self.ptr("bytes", 8 * GUARD), stream)
        src = self.ptr("src", self.src_off) if self.size else None
        if self.is_spans:
            return pb.lib().pire_hip_gather_spans(src, self.size, self.ptr("spans"), self.ptr("count"), self.cap, tail, flags, *outs)
        return pb.lib().pire_hip_gather(src, self.ptr("offsets"), self.n, self.ptr("idx"), self.ptr("count"), self.cap, tail, flags, *outs)

    def fetch(self):
        """Every buffer of the call as it is now, outputs and inputs (for bit-identity of two calls)"""
        if self.device:
            self.torch.cuda.synchronize()
            return {k: v.cpu().numpy().view(self.host[k].dtype) for k, v in self.dev.items()}
        return self.host

    def check(self, exp_text, exp_offs, total, refused=False):
        now = self.fetch()
        for k in ("src", "offsets", "idx", "spans", "count"):
            if k in now:
                assert (now[k] == self.before[k]).all(), "the input %s was written to" % k
        if refused:
            for k in ("out", "offs", "bytes"):
                assert (now[k] == self.before[k]).all(), "%s written by a refused call" % k
            return
        b = now["bytes"]
        assert int(b[GUARD]) == total, (int(b[GUARD]), total)
        assert (np.delete(b, GUARD) == np.uint64(POISON64)).all(), "words around out_bytes written"
        k = len(exp_offs) - 1
        o = now["offs"]
        got = o[GUARD:GUARD + k + 1]
        assert (got == exp_offs).all(), ("out_offsets", np.flatnonzero(got != exp_offs)[:5], got[:8], exp_offs[:8])
        assert (o[:GUARD] == np.uint64(POISON64)).all() and (o[GUARD + k + 1:] == np.uint64(POISON64)).all(), "out_offsets written outside entries 0..k"
        t = now["out"]
        first = GUARD_B + self.out_off
        written = min(total, self.text_cap)
        got = t[first:first + written]
        assert (got == exp_text[:written]).all(), ("out_text", np.flatnonzero(got != exp_text[:written])[:5], written)
        assert (t[:first] == POISON).all() and (t[first + written:] == POISON).all(), "bytes around out_text[0, min(total, text_cap)) written"


def check_gather(torch, strings_or_batch, idx=None, count=None, cap=None, tail=None, text_cap=None, modes=("host", "device"),
                 src_off=0, out_off=0):
    text, offs = batch(strings_or_batch) if isinstance(strings_or_batch, list) else strings_or_batch
    et, eo, total = restate_gather(text, offs, idx, count, cap, tail)
    for mode in modes:
        c = Call(torch, mode, text, offsets=offs, idx=idx, count=count, cap=cap, tail=tail, text_cap=total if text_cap is None else text_cap,
                 src_off=src_off, out_off=out_off)
        assert c.run() == 0, (mode, pb.lib().pire_hip_last_error())
        try:
            c.check(et, eo, total)
        except AssertionError as e:
            raise AssertionError("%s, tail %s, src_off %d, out_off %d: %s" % (mode, tail, src_off, out_off, e))
    return total


def plain(rng, size):
    return rng.randint(32, 127, size=size).astype(np.uint8)


def strings_of(rng, lens):
    flat = plain(rng, int(np.sum(lens)))
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [flat[cuts[i]:cuts[i + 1]].tobytes() for i in range(len(lens))]


TAILS = (None, 10, 0, 255)


# ---- GPU: pire_hip_gather --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("tail", TAILS)
def test_hand_written_batches(torch_cuda, tail):
    strings = [b"", b"", b"alpha", b"", b"be", b"\n", b"gamma delta", b"", b"", b"", b"e", b"zeta\x00\xff", b""]
    n = len(strings)
    lists = [None, list(range(n)), [], [4], [0], [n - 1], [2, 2, 2], [6, 6, 0, 6], list(range(n - 1, -1, -1)), [0, 1, 3, 7, 8, 9, 12],
             [0, 1, 2], [10, 11, 12], [12, 12, 11, 0, 0, 2, 9, 8, 7]]
    for idx in lists:
        check_gather(torch_cuda, strings, idx=idx, tail=tail)
    check_gather(torch_cuda, [b""] * 5, tail=tail)
    check_gather(torch_cuda, [b"x"], tail=tail)
    check_gather(torch_cuda, [], tail=tail)            # n = 0, idx = NULL: nothing but *out_bytes and out_offsets[0]


def lens_summing_to(rng, total, tail, top=70):
    """Random lengths 0..top whose strings, with their tails, fill exactly `total` output bytes"""
    a = 0 if tail is None else 1
    lens = []
    left = total
    while left > 0:
        ln = int(min(rng.randint(0, top + 1), left - a))
        if ln < 0:
            break
        lens.append(ln)
        left -= ln + a
    assert sum(lens) + a * len(lens) == total
    return lens


@gpu
@pytest.mark.parametrize("tail", (None, 10))
def test_tile_edges(torch_cuda, tail):
    rng = np.random.RandomState(7)
    a = 0 if tail is None else 1
    for total in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        assert check_gather(torch_cuda, strings_of(rng, lens_summing_to(rng, total, tail)), tail=tail) == total
        assert check_gather(torch_cuda, strings_of(rng, [total - a]), tail=tail) == total      # one string
    # one string of 2T + 5 bytes between short ones: a block's tile lies wholly inside a string
    check_gather(torch_cuda, strings_of(rng, [3, 0, 40, 2 * T + 5, 7, 0, 1]), tail=tail)
    check_gather(torch_cuda, strings_of(rng, [3, 0, 40, 2 * T + 5, 7, 0, 1]), idx=[3, 0, 3, 6], tail=tail, out_off=5)
    # a string that ends exactly at a tile boundary: with a tail, the tail is the first byte of the next tile
    check_gather(torch_cuda, strings_of(rng, [100, T - 100, 50, 9]), tail=tail)
    check_gather(torch_cuda, strings_of(rng, [100, T - 100 - a, 50, 9]), tail=tail)
    # 200 empty strings (with a tail: 200 one-byte strings) on a tile boundary, in front of byte 0, and behind the last byte
    for front in ([T - 7 * a], [T - 100 * a], [T - 200 * a], [T - 57, 57 - 13 * a], []):
        check_gather(torch_cuda, strings_of(rng, front + [0] * 200 + [33, T, 5]), tail=tail)
    check_gather(torch_cuda, strings_of(rng, [0] * 200 + [T + 3] + [0] * 200), tail=tail)
    check_gather(torch_cuda, strings_of(rng, [0] * 200), tail=tail)
    # more strings in one tile than the copy pass stages (2 048): short strings, runs of empty ones
    check_gather(torch_cuda, strings_of(rng, rng.randint(0, 4, size=9000).tolist()), tail=tail)
    check_gather(torch_cuda, strings_of(rng, [5] + [0] * 3000 + [T + 9] + [0] * 2500 + [1]), tail=tail)


@gpu
@pytest.mark.parametrize("src_off", range(16))
def test_every_pair_of_source_and_output_alignment(torch_cuda, src_off):
    """About 2.5 T output bytes of strings of 0..70 bytes, the source src_off bytes and out_text 0..15 bytes behind a
    16-byte boundary: all 16 x 16 pairs."""
    rng = np.random.RandomState(100 + src_off)
    lens = rng.randint(0, 71, size=1170)
    text, offs = batch(strings_of(rng, lens))
    idx = rng.permutation(len(lens)).astype(np.uint64)
    assert 2.3 * T < offs[-1] < 2.7 * T
    for out_off in range(16):
        tail = (None, 10)[(src_off + out_off) & 1]
        check_gather(torch_cuda, (text, offs), idx=None if out_off & 2 else idx, tail=tail, src_off=src_off, out_off=out_off)


@gpu
def test_lengths_around_the_group_size_at_every_source_residue(torch_cuda):
    """Strings of 15, 16, 17, 31, 32, 33 bytes, each beginning at every residue modulo 16 of the source (filler strings of
    1..16 bytes in between move them there), gathered without the fillers."""
    rng = np.random.RandomState(3)
    lens, pick, pos = [], [], 0
    for ln in (15, 16, 17, 31, 32, 33):
        for res in range(16):
            fill = (res - pos) % 16 or 16
            lens += [fill, ln]
            pos += fill + ln
            assert (pos - ln) % 16 == res
            pick.append(len(lens) - 1)
    text, offs = batch(strings_of(rng, lens))
    for tail in (None, 255):
        for src_off, out_off in ((0, 0), (0, 9), (5, 0), (11, 3)):
            check_gather(torch_cuda, (text, offs), idx=pick, tail=tail, src_off=src_off, out_off=out_off)
        check_gather(torch_cuda, (text, offs), idx=pick[::-1], tail=tail)


@gpu
def test_caps(torch_cuda):
    rng = np.random.RandomState(5)
    lens = rng.randint(0, 90, size=700)
    lens[350] = 500
    strings = strings_of(rng, lens)
    text, offs = batch(strings)
    idx = rng.randint(0, 700, size=600).astype(np.uint64)
    idx[300] = 350
    for tail in (None, 10):
        et, eo, total = restate_gather(text, offs, idx, tail=tail)
        middle = int(eo[300]) + 250                                      # inside the long string
        for text_cap in (0, 1, total - 1, total, middle, total + 100):
            assert check_gather(torch_cuda, (text, offs), idx=idx, tail=tail, text_cap=text_cap) == total
        check_gather(torch_cuda, (text, offs), idx=idx, count=600, cap=411, tail=tail)      # idx_cap < *idx_count: k = idx_cap
        check_gather(torch_cuda, (text, offs), idx=idx, count=123, cap=600, tail=tail)      # *idx_count < idx_cap: the rest stays poison
        check_gather(torch_cuda, (text, offs), idx=idx, count=0, cap=600, tail=tail)
        check_gather(torch_cuda, (text, offs), idx=idx, count=None, cap=600, tail=tail)     # idx_count = NULL
        check_gather(torch_cuda, (text, offs), idx=None, count=650, cap=700, tail=tail)
        check_gather(torch_cuda, (text, offs), idx=idx, count=1 << 40, cap=77, tail=tail, text_cap=1000)


@gpu
def test_an_index_or_span_out_of_range(torch_cuda):
    torch = torch_cuda
    rng = np.random.RandomState(6)
    strings = strings_of(rng, rng.randint(0, 50, size=40))
    text, offs = batch(strings)
    n = len(strings)
    for tail in (None, 10):
        for idx in ([3, n, 5], [n + 1000], [0, 1, 1 << 63, 2], [7, 8, (1 << 64) - 1]):
            et, eo, total = restate_gather(text, offs, idx, tail=tail)      # an empty string and its tail at that place
            c = Call(torch, "device", text, offsets=offs, idx=idx, tail=tail, text_cap=total)
            assert c.run() == 0
            c.check(et, eo, total)
            c = Call(torch, "host", text, offsets=offs, idx=idx, tail=tail, text_cap=total)
            assert c.run() == -1 and "out of range" in pb.lib().pire_hip_last_error().decode()
            c.check(et, eo, total, refused=True)
        for spans in ([[0, 5], [9, 8], [5, 10]], [[0, 5], [3, len(text) + 1]], [[len(text) + 5, len(text) + 9]], [[4, 2], [0, 1 << 63]]):
            et, eo, total = restate_spans(text, spans, tail=tail)
            c = Call(torch, "device", text, spans=spans, tail=tail, text_cap=total)
            assert c.run() == 0
            c.check(et, eo, total)
            c = Call(torch, "host", text, spans=spans, tail=tail, text_cap=total)
            assert c.run() == -1 and "out of range" in pb.lib().pire_hip_last_error().decode()
            c.check(et, eo, total, refused=True)


# ---- GPU: the spans form, the inverse of the split ---------------------------------------------------------------------------

@gpu
def test_the_64_bit_carry_of_the_scan_over_more_than_1024_tiles_of_strings(torch_cuda):
    """(1 << 20) + 1025 strings of 0-3 bytes are 1 026 tiles of strings: the scan of the tile sums takes a second step and
    carries the 64-bit total of the first into it.  Device pointers, the identity for idx, a tail byte; numpy says what
    out_offsets and out_text have to be."""
    torch = torch_cuda
    rng = np.random.RandomState(41)
    k, tail = (1 << 20) + 1025, 10
    lens = rng.randint(0, 4, size=k).astype(np.uint64)
    offs = np.zeros(k + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    size = int(offs[-1])
    text = rng.randint(97, 123, size=size).astype(np.uint8)
    exp_offs = np.zeros(k + 1, dtype=np.uint64)
    exp_offs[1:] = np.cumsum(lens + np.uint64(1))
    total = int(exp_offs[-1])
    exp_text = np.full(total, tail, dtype=np.uint8)
    exp_text[np.arange(size) + np.repeat(np.arange(k), lens.astype(np.int64))] = text   # byte p of string j moves j tails further
    d_text = torch.as_tensor(text, device="cuda")
    d_offs = torch.as_tensor(offs.view(np.int64), device="cuda")
    out_text = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out_offs = torch.full((k + 1 + 8,), -1, dtype=torch.int64, device="cuda")
    out_bytes = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    pb.gather_device(d_text.data_ptr(), d_offs.data_ptr(), k, out_bytes.data_ptr(), idx_cap=k, tail=tail, out_text_ptr=out_text.data_ptr(),
                     text_cap=total, out_offsets_ptr=out_offs.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(out_bytes.cpu()[0]) == total
    got_offs = out_offs.cpu().numpy().view(np.uint64)
    assert (got_offs[:k + 1] == exp_offs).all() and (got_offs[k + 1:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    got_text = out_text.cpu().numpy()
    assert (got_text[:total] == exp_text).all() and (got_text[total:] == 0xEE).all()


def log_like_raw(rng, lines, last_terminated=True):
    words = [b"GET", b"POST", b"/index.html", b"/api/v1/items", b"200", b"404", b"hello  world", b"hello world", b"-", b"\"Mozilla/5.0\""]
    out = []
    for i in range(lines):
        k = rng.randint(0, 7)
        line = b" ".join(words[j] for j in rng.randint(0, len(words), size=k))
        if i % 3 == 0:
            line = words[6 + i % 2]
        out.append(line + (b"\r\n" if i % 5 == 0 else b"\n"))
    out[3] = b"\n"
    out[4] = b"\n"
    raw = b"".join(out)
    return u8(raw if last_terminated else raw[:-1]).copy()


@gpu
def test_the_spans_of_run_lines_select(torch_cuda):
    big = [b for b in H.big_sets() if b["name"] == "c2_single"][0]
    t = pb.Table(H.load_blob(big["blob"]))
    rng = np.random.RandomState(8)
    raw = log_like_raw(rng, 400, last_terminated=False)
    got = t.run_lines_select_host(raw)
    spans = got["spans"]
    assert 10 < got["count"] < 390 and len(spans) == got["count"]
    for extra in (spans, np.concatenate([spans, [[0, 0], [len(raw), len(raw)], [0, len(raw)]]]).astype(np.uint64), spans[::-1]):
        for tail in (None, 10):
            et, eo, total = restate_spans(raw, extra, tail=tail)
            assert et.tobytes() == b"".join(raw[int(b):int(e)].tobytes() + (b"" if tail is None else b"\n") for b, e in extra)
            for mode in ("host", "device"):
                c = Call(torch_cuda, mode, raw, spans=extra, tail=tail, text_cap=total, src_off=3, out_off=7)
                assert c.run() == 0, pb.lib().pire_hip_last_error()
                c.check(et, eo, total)
            ht, ho, hb = pb.gather_host(raw, spans=extra, tail=tail)                # the binding's wrapper: the same answer
            assert hb == total and (ht == et).all() and (ho == eo).all()


@gpu
@pytest.mark.parametrize("delim", [10, 0, 255])
def test_the_gather_is_the_inverse_of_the_split(torch_cuda, delim):
    from tests.test_split import restate

    torch = torch_cuda
    rng = np.random.RandomState(delim + 1)
    for size in (T - 5, T, 3 * T + 1):
        for terminated in (True, False):
            raw = rng.randint(0, 256, size=size).astype(np.uint8)
            raw[rng.rand(size) < 1 / 40] = delim
            raw[-1] = delim if terminated else (delim ^ 1)
            text, offs, n = restate(raw, delim)
            whole = raw if terminated else np.concatenate([raw, np.array([delim], dtype=np.uint8)])
            keep = restate(whole, delim, keep=True)[1]
            # on the device: split into text + offsets, gather everything with the delimiter as the tail
            d_raw = torch.as_tensor(raw, device="cuda")
            d_text = torch.zeros(size + 16, dtype=torch.uint8, device="cuda")
            d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            pb.split_device(d_raw.data_ptr(), size, d_n.data_ptr(), delim, d_text.data_ptr(), d_offs.data_ptr(), n, stream)
            out = torch.full((GUARD_B + len(whole) + GUARD_B,), POISON, dtype=torch.uint8, device="cuda")
            oo = torch.full((n + 1 + GUARD,), int(np.uint64(POISON64).astype(np.int64)), dtype=torch.int64, device="cuda")
            total = torch.zeros(1, dtype=torch.int64, device="cuda")
            pb.gather_device(d_text.data_ptr(), d_offs.data_ptr(), n, total.data_ptr(), idx_count_ptr=d_n.data_ptr(), idx_cap=n, tail=delim,
                             out_text_ptr=out.data_ptr() + GUARD_B, text_cap=len(whole), out_offsets_ptr=oo.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert int(total.cpu()[0]) == len(whole) and (got[GUARD_B:GUARD_B + len(whole)] == whole).all()
            assert (got[:GUARD_B] == POISON).all() and (got[GUARD_B + len(whole):] == POISON).all()
            o = oo.cpu().numpy().view(np.uint64)
            assert (o[:n + 1] == keep).all() and (o[n + 1:] == np.uint64(POISON64)).all()
            # host pointers: the same two calls
            ht, ho, hn = pb.split_host(raw, delim)
            gt, go, gb = pb.gather_host(ht, ho, tail=delim)
            assert gb == len(whole) and (gt == whole).all() and (go == keep).all()


# ---- GPU: pire_hip_run_lines_gather ------------------------------------------------------------------------------------------

def dev_run_lines_gather(torch, t, raw, flags, want=None, tail=-1, cap=None, text_cap=None, raw_off=0, out_off=0, hits=True):
    size = len(raw)
    cap = size if cap is None else cap
    text_cap = size + cap if text_cap is None else text_cap
    host = np.full(raw_off + size + 256, 10, dtype=np.uint8)
    host[raw_off:raw_off + size] = raw
    d = torch.as_tensor(host, device="cuda")
    poison = int(np.uint64(POISON64).astype(np.int64))
    d_hits = torch.full((cap + GUARD,), poison, dtype=torch.int64, device="cuda")
    d_offs = torch.full((cap + 1 + GUARD,), poison, dtype=torch.int64, device="cuda")
    d_text = torch.full((GUARD_B + out_off + text_cap + GUARD_B,), POISON, dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), poison, dtype=torch.int64, device="cuda")
    wm = t.want_mask(want)
    dw = None if wm is None else torch.as_tensor(wm.view(np.int64), device="cuda")
    t.run_lines_gather_device(d.data_ptr() + raw_off if size else 0, size, flags, counts.data_ptr(), counts.data_ptr() + 8,
                              counts.data_ptr() + 16, tail=tail, want_ptr=0 if dw is None else dw.data_ptr(),
                              out_hits_ptr=d_hits.data_ptr() if hits and cap else 0, hit_cap=cap,
                              out_text_ptr=d_text.data_ptr() + GUARD_B + out_off if text_cap else 0, text_cap=text_cap,
                              out_offsets_ptr=d_offs.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == host).all(), "the input was written to"
    c = counts.cpu().numpy().view(np.uint64)
    k = min(int(c[1]), cap)
    h, o, x = d_hits.cpu().numpy().view(np.uint64), d_offs.cpu().numpy().view(np.uint64), d_text.cpu().numpy()
    assert (h[k if hits else 0:] == np.uint64(POISON64)).all() and (o[k + 1:] == np.uint64(POISON64)).all()
    first, written = GUARD_B + out_off, min(int(c[2]), text_cap)
    assert (x[:first] == POISON).all() and (x[first + written:] == POISON).all(), "bytes around out_text written"
    return {"lines": int(c[0]), "count": int(c[1]), "bytes": int(c[2]), "hits": h[:k] if hits else None, "offsets": o[:k + 1],
            "text": x[first:first + written]}


def check_lines_gather(got, exp, tail_byte, cap=None, text_cap=None):
    """exp: tests/test_split.py's expected_lines_select (the restatement and the oracle)"""
    assert got["lines"] == exp["lines"] and got["count"] == exp["count"]
    k = exp["count"] if cap is None else min(cap, exp["count"])
    if got["hits"] is not None:
        assert len(got["hits"]) == k and (got["hits"] == exp["hits"][:k]).all()
    t = b"" if tail_byte is None else bytes([tail_byte])
    pieces = [b + t for b in exp["bytes"][:k]]                                    # the host join of the oracle's hits
    whole = b"".join(pieces)
    assert got["bytes"] == len(whole)
    want_offs = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
    assert (got["offsets"] == want_offs).all()
    written = len(whole) if text_cap is None else min(text_cap, len(whole))
    assert got["text"].tobytes() == whole[:written]


@gpu
@pytest.mark.parametrize("name", ["set_a", "c2_single"])     # set_a: eight regexps glued into one scanner
def test_run_lines_gather_against_oracle_and_restatement(torch_cuda, name):
    from tests.test_split import LINES, expected_lines_select, planted_raw, dev_run_lines_select

    big = [b for b in H.big_sets() if b["name"] == name][0]
    blob = H.load_blob(big["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    raw = planted_raw(big, seed=77, lines=LINES // 2, last_terminated=False)
    want = [0] if name == "set_a" else None
    exp = expected_lines_select(name, t, o, raw, BE, want)
    assert exp["lines"] == LINES // 2 and 50 < exp["count"] < LINES // 2 - 50, exp["count"]
    # an unterminated last line that matches: the bytes of a line that did, once more, without a delimiter behind them
    raw = np.concatenate([raw, u8(b"\n"), u8([b for b in exp["bytes"] if b][0])])
    exp = expected_lines_select(name, t, o, raw, BE, want)
    assert exp["hits"][-1] == exp["lines"] - 1 and raw[-1] != 10
    ref = dev_run_lines_select(torch_cuda, t, raw, BE, want)
    for tail, tb in ((-1, 10), (None, None), (0, 0)):
        got = dev_run_lines_gather(torch_cuda, t, raw, BE, want, tail=tail, raw_off=3, out_off=5)
        check_lines_gather(got, exp, tb)
        assert (got["lines"], got["count"]) == (ref["lines"], ref["count"]) and (got["hits"] == ref["hits"]).all()
    assert pb.last_kernel() not in ("", None) and "gather" not in pb.last_kernel().lower()
    select_kernel = pb.last_kernel()
    dev_run_lines_select(torch_cuda, t, raw, BE, want)
    assert pb.last_kernel() == select_kernel                                      # the scan kernel is the one the call names
    # with tail = delim: what grep prints for the buffer
    grep = b"".join(b + b"\n" for b in exp["bytes"])
    assert dev_run_lines_gather(torch_cuda, t, raw, BE, want)["text"].tobytes() == grep
    # the library keeps the hit list to itself
    check_lines_gather(dev_run_lines_gather(torch_cuda, t, raw, BE, want, hits=False), exp, 10)
    # room for fewer hits than there are: the count whole, the first hit_cap strings; room for fewer bytes
    for cap in (exp["count"] - 3, 1, 0):
        check_lines_gather(dev_run_lines_gather(torch_cuda, t, raw, BE, want, cap=cap), exp, 10, cap=cap)
    for text_cap in (0, 1, len(grep) - 1, len(grep) // 2):
        check_lines_gather(dev_run_lines_gather(torch_cuda, t, raw, BE, want, text_cap=text_cap), exp, 10, text_cap=text_cap)
    # host pointers: the same answer
    got = t.run_lines_gather_host(raw, want=want)
    check_lines_gather(got, exp, 10)
    got = t.run_lines_gather_host(raw, want=want, tail=None, hit_cap=5, text_cap=40)
    check_lines_gather(got, exp, None, cap=5, text_cap=40)
    # no line at all, no hit at all
    for empty in (np.zeros(0, dtype=np.uint8), u8(b"\n\n\n")):
        e = expected_lines_select(name, t, o, empty, BE, want)
        assert e["count"] == 0
        check_lines_gather(dev_run_lines_gather(torch_cuda, t, empty, BE, want, cap=4, text_cap=16), e, 10, cap=4)
        check_lines_gather(t.run_lines_gather_host(empty, want=want, hit_cap=4, text_cap=16), e, 10, cap=4)


# ---- GPU: a cascade of two scanners, on the device ---------------------------------------------------------------------------

@gpu
def test_cascade_of_two_scanners_without_a_host_round_trip(torch_cuda):
    torch = torch_cuda
    sets = {b["name"]: b for b in H.big_sets()}
    big_a, big_b = sets["set_a"], sets["c2_single"]
    ta, oa = pb.Table(H.load_blob(big_a["blob"])), ob.OracleScanner(H.load_blob(big_a["blob"]))
    tb, o_b = pb.Table(H.load_blob(big_b["blob"])), ob.OracleScanner(H.load_blob(big_b["blob"]))
    n, top = 3000, 300
    rng = np.random.RandomState(21)
    rec = ob.corpus_fill(31, 0, n, top, H.plants_for(big_a), threads=4)
    lens = rng.randint(0, top + 1, size=n)
    lens[rng.rand(n) < 0.05] = 0
    strings = [rec[i, top - lens[i]:].tobytes() for i in range(n)]
    long = ob.corpus_fill(32, 0, 1, 40 << 10, H.plants_for(big_a), threads=1)[0].tobytes()
    strings[1500] = long
    text, offs = batch(strings)
    # what the oracles say: A on everything, B on exactly the strings A selects
    ia = oa.run(text, offs, flags=BE, threads=4)[0]
    sel = np.array([ta.Final(int(s)) for s in ia])
    hits = np.flatnonzero(sel)
    assert 100 < len(hits) < n - 100
    gt, go, gtotal = restate_gather(text, offs, idx=hits)
    ib = o_b.run(gt, go, flags=BE, threads=4)[0]
    # the device: run_select(A) -> gather(hits, count on the device) -> run(B), all enqueued, one synchronise at the end
    ta.upload()
    tb.upload()
    stream = torch.cuda.current_stream().cuda_stream
    d_text, d_offs = torch.as_tensor(text, device="cuda"), torch.as_tensor(offs.view(np.int64), device="cuda")
    d_hits = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    g_text = torch.full((len(text) + 64,), POISON, dtype=torch.uint8, device="cuda")
    g_offs = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    g_bytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    out_b = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ta.run_select_device(d_text.data_ptr(), d_offs.data_ptr(), n, BE | pb.FLAG_NO_PEEK, d_count.data_ptr(), out_hits_ptr=d_hits.data_ptr(),
                         hit_cap=n, stream=stream)
    pb.gather_device(d_text.data_ptr(), d_offs.data_ptr(), n, g_bytes.data_ptr(), idx_ptr=d_hits.data_ptr(), idx_count_ptr=d_count.data_ptr(),
                     idx_cap=n, out_text_ptr=g_text.data_ptr(), text_cap=len(text), out_offsets_ptr=g_offs.data_ptr(), stream=stream)
    k = len(hits)   # (how many strings B is given: the oracle's count, nothing is read back from the device)
    tb.run_device(g_text.data_ptr(), g_offs.data_ptr(), k, BE | pb.FLAG_NO_PEEK, out_idx_ptr=out_b.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert int(d_count.cpu()[0]) == k and (d_hits.cpu().numpy()[:k].view(np.uint64) == hits.astype(np.uint64)).all()
    assert int(g_bytes.cpu()[0]) == gtotal and (g_text.cpu().numpy()[:gtotal] == gt).all()
    assert (g_offs.cpu().numpy()[:k + 1].view(np.uint64) == go).all()
    got = out_b.cpu().numpy().view(np.uint32)
    assert (got[:k] == ib).all(), np.flatnonzero(got[:k] != ib)[:5]


# ---- GPU: enqueue-only, determinism ------------------------------------------------------------------------------------------

@gpu
def test_an_on_device_call_only_enqueues(torch_cuda, cfg):
    """pire_hip_gather and pire_hip_gather_spans on a side stream behind a long-running scan: back on the host before that
    scan has finished, right after the synchronise (the method of tests/test_select.py)."""
    torch = torch_cuda
    cfg.set(auto_adapt=1)
    big = [b for b in H.big_sets() if b["name"] == "set_a"][0]
    t = pb.Table(H.load_blob(big["blob"]))
    t.upload()
    rng = np.random.RandomState(17)
    strings = strings_of(rng, rng.randint(0, 200, size=3000))
    text, offs = batch(strings)
    idx = rng.permutation(3000)[:2000].astype(np.uint64)
    spans = np.stack([offs[idx], offs[idx + np.uint64(1)]], axis=1)
    et, eo, total = restate_gather(text, offs, idx, tail=10)
    side = torch.cuda.Stream()
    warm = Call(torch, "device", text, offsets=offs, idx=idx, count=2000, tail=10, text_cap=total)
    assert warm.run() == 0                     # first use: the kernels' code objects
    warm.check(et, eo, total)
    ln, llen = 64, 8 << 20
    long_text = torch.empty((ln, llen), dtype=torch.uint8, device="cuda")
    pire_amd.corpus_fill_device(long_text.data_ptr(), 5, 0, ln, llen, llen, H.plants_for(big), torch.cuda.current_stream().cuda_stream)
    lidx = torch.empty(ln, dtype=torch.int32, device="cuda")
    # every buffer of the calls under test is there before the long scan starts
    a = Call(torch, "device", text, offsets=offs, idx=idx, count=2000, tail=10, text_cap=total, out_off=3)
    b = Call(torch, "device", text, spans=spans, count=2000, tail=10, text_cap=total, src_off=5)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    t.run_strided_device(long_text.data_ptr(), ln, llen, llen, BE | pb.FLAG_GENERIC, lidx.data_ptr(), 0, 0, 0, side.cuda_stream)
    done.record(side)
    t0 = time.perf_counter()
    ra = a.run(side.cuda_stream)
    running_after_gather = not done.query()
    rb = b.run(side.cuda_stream)          # right behind the first call, behind the same scan
    returned = time.perf_counter() - t0
    still_running = not done.query()
    side.synchronize()
    assert ra == 0 and rb == 0
    assert running_after_gather and still_running, \
        "the calls came back only after the scan in front of them had finished (%.1f ms)" % (returned * 1e3)
    a.check(et, eo, total)
    b.check(et, eo, total)


@gpu
def test_two_device_calls_are_bit_identical(torch_cuda):
    rng = np.random.RandomState(13)
    lens = rng.randint(0, 300, size=30000)
    lens[777] = 5 * T + 3
    text, offs = batch(strings_of(rng, lens))
    idx = rng.randint(0, 30000, size=20000).astype(np.uint64)
    idx[5] = 777
    et, eo, total = restate_gather(text, offs, idx, count=19000, tail=10)
    runs = []
    for _ in range(2):
        c = Call(torch_cuda, "device", text, offsets=offs, idx=idx, count=19000, tail=10, text_cap=total - 100, src_off=1, out_off=3)
        assert c.run() == 0
        runs.append({k: v.tobytes() for k, v in c.fetch().items()})
        c.check(et, eo, total)
    assert runs[0] == runs[1]
