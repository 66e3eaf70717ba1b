"""pire_hip_splice and pire_hip_search_lines_splice: the matches of a resident buffer replaced, the rest kept (splice.hip) --
`sed 's/re/repl/g'`, deletion, redaction and `grep --color` without leaving the device.

Exact equality everywhere.  The expected values come from `model_splice`, the formulas of include/pire_hip.h in plain Python, over
span lists written by hand or by tests/test_search_all.py's `model_all` / tests/test_search.py's `model_search`; the model is
itself held against `re.sub`.  Nothing expected comes from the library.  Every output sits between poisoned guard bytes, and the
input is compared with what went in.  The scanner pairs are tests/golden/search/*."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pire_amd
from pire_amd import binding as pb
from tests import helpers as H
from tests import test_search as TS
from tests import test_search_all as TA

ROOT = TS.ROOT
POISON, GUARD, EINVAL = TS.POISON, TS.GUARD, TS.EINVAL
S, B, E = TS.S, TS.B, TS.E
KEEP, FIRST = pb.SPLICE_KEEP, pb.SPLICE_FIRST
gpu = pytest.mark.gpu
u8 = TS.u8
NAMES = ("pire_hip_splice", "pire_hip_search_lines_splice")
TILE = 16384


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_splice(raw, spans, head=b"", tail=b"", mode=0, offsets=None):
    """include/pire_hip.h, line by line: {"text", "bytes", "pos", "offsets"}"""
    raw = bytes(raw)
    out, pos, D, at = [], [], [0], 0
    for b, e in spans:                                              # [b_j, e_j) = [spans[2j], spans[2j+1])
        b, e = int(b), int(e)
        assert at <= b <= e <= len(raw)                             # b_j <= e_j <= size,  e_{j-1} <= b_j
        piece = head + (raw[b:e] if mode & KEEP else b"") + tail    # piece_j = head ++ (KEEP ? raw[b_j, e_j) : "") ++ tail
        out += [raw[at:b], piece]                                   # out = raw[0, b_0) ++ piece_0 ++ raw[e_0, b_1) ++ ...
        pos.append(b + D[-1])                                       # out_pos[j] = b_j + D(j)
        D.append(D[-1] + len(piece) - (e - b))                      # D(j) = sum over i < j of (P_i - (e_i - b_i))
        at = e
    out.append(raw[at:])                                            # ... ++ raw[e_{k-1}, size)
    res = {"text": b"".join(out), "bytes": (len(raw) + D[-1]) % (1 << 64), "pos": np.array(pos, dtype=np.uint64), "offsets": None}
    assert len(res["text"]) == res["bytes"]                         # *out_bytes = size + D(k)
    if offsets is not None:                                         # out_offsets[i] = offsets[i] + D(first j with b_j >= offsets[i])
        begins = [int(b) for b, _ in spans]
        first = lambda o: next((j for j, b in enumerate(begins) if b >= o), len(begins))
        res["offsets"] = np.array([int(o) + D[first(int(o))] for o in offsets], dtype=np.uint64)
    return res


FORMULAS = """
 *   k = min(span_count ? *span_count : span_cap, span_cap)
 *   [b_j, e_j) = [spans[2j], spans[2j+1])                      span j of raw, 0 <= j < k
 *   b_j <= e_j <= size,  e_{j-1} <= b_j                        ascending and disjoint; b_j == e_j: an insertion point
 *   piece_j = head ++ (KEEP ? raw[b_j, e_j) : "") ++ tail      P_j = |piece_j|
 *   out = raw[0, b_0) ++ piece_0 ++ raw[e_0, b_1) ++ piece_1 ++ ... ++ piece_{k-1} ++ raw[e_{k-1}, size)
 *   D(j) = sum over i < j of (P_i - (e_i - b_i))               64-bit, wrap-around
 *   *out_bytes = size + D(k)
 *   out_pos[j] = b_j + D(j)                                    where piece j begins in out
 *   out_offsets[i] = offsets[i] + D(first j with b_j >= offsets[i])        (that j is k where there is none)
"""


# ---- CPU: the model ------------------------------------------------------------------------------------------------------------

def test_the_model_on_examples_written_by_hand():
    m = model_splice(b"a1b22c", [(1, 2), (3, 5)], b"#")
    assert (m["text"], m["bytes"], m["pos"].tolist()) == (b"a#b#c", 5, [1, 3])
    m = model_splice(b"a1b22c", [(1, 2), (3, 5)], b"<", b">", KEEP, offsets=[0, 1, 3, 3, 6])
    assert (m["text"], m["pos"].tolist(), m["offsets"].tolist()) == (b"a<1>b<22>c", [1, 5], [0, 1, 5, 5, 10])
    assert model_splice(b"abc", [(0, 3)])["text"] == b"" and model_splice(b"", [(0, 0), (0, 0)], b"x", b"y")["text"] == b"xyxy"
    # an empty span on a boundary belongs to the string that begins there: "ab" | "cd" with an insertion at 2
    m = model_splice(b"abcd", [(2, 2)], b"-", offsets=[0, 2, 4])
    assert m["text"] == b"ab-cd" and m["offsets"].tolist() == [0, 2, 5]


def test_the_model_over_every_match_is_re_sub():
    """on the drawn strings of the pairs whose pattern cannot match empty and whose matches are Python's own"""
    pairs = []
    for name in sorted(TS.DRAW):
        rx = re.compile(TS.pattern_of(name).encode(), re.S)
        if rx.fullmatch(b""):
            continue
        strings = TS.drawn_strings(name, 300, 12, 7)
        matches = TA.model_all(name, strings, 0)
        if any([m.span() for m in rx.finditer(s)] != ms for s, ms in zip(strings, matches)):
            continue                                                # (leftmost-longest is not always Python's leftmost-first)
        pairs.append(name)
        for s, ms in zip(strings, matches):
            assert model_splice(s, ms, b"<>")["text"] == rx.sub(b"<>", s), (name, s)
            assert model_splice(s, ms)["text"] == rx.sub(b"", s), (name, s)
            assert model_splice(s, ms, b"[", b"]", KEEP)["text"] == rx.sub(rb"[\g<0>]", s), (name, s)
    assert len(pairs) >= 2, pairs


# ---- CPU: the interface --------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_entry_points_and_the_header_has_the_formulas():
    L = C.CDLL(pire_amd.lib_path())
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        src = f.read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in {n for n, _, _ in pb.ABI}
        assert re.search(r"\nint %s\(" % name, src), name
    for line in FORMULAS.strip("\n").splitlines():
        assert line in src, line
    assert "#define PIRE_HIP_SPLICE_KEEP 1u" in src and "#define PIRE_HIP_SPLICE_FIRST 2u" in src
    assert "moves to string i" in src and "sed 's|x*|-|g'" in src and "every source position is clamped" in src
    assert (KEEP, FIRST, pb.SPLICE_PIECE_MAX) == (1, 2, 256)


def _guarded():
    return {"text": np.full(64, POISON, dtype=np.uint8), "pos": np.full(8 * 6, POISON, dtype=np.uint8),
            "offsets": np.full(8 * 6, POISON, dtype=np.uint8), "spans": np.full(16 * 6, POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def _but(names, ok, **kw):
    a = list(ok)
    for k, v in kw.items():
        a[names.index(k)] = v
    return a


def test_splice_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"a1b22c..").copy()
    spans = np.array([1, 2, 3, 5], dtype=np.uint64)
    offs = np.array([0, 3, 8], dtype=np.uint64)
    head, tail = C.create_string_buffer(b"x" * 300), C.create_string_buffer(b"y" * 300)
    bufs, total, cnt = _guarded(), C.c_uint64(79), C.c_uint64(2)
    names = ("raw", "size", "spans", "count", "cap", "head", "head_len", "tail", "tail_len", "mode", "offsets", "n", "text", "text_cap", "pos",
             "out_offsets", "bytes")
    ok = [raw.ctypes.data, raw.size, spans.ctypes.data, C.addressof(cnt), 2, C.addressof(head), 3, C.addressof(tail), 2, KEEP, offs.ctypes.data, 2,
          bufs["text"].ctypes.data, 32, bufs["pos"].ctypes.data, bufs["offsets"].ctypes.data, C.addressof(total)]
    but = lambda **kw: _but(names, ok, **kw)
    cases = {
        "null out_bytes": but(bytes=None),
        "head_len > 256": but(head_len=257),
        "tail_len > 256": but(tail_len=257),
        "head_len > 0 with null head": but(head=None),
        "tail_len > 0 with null tail": but(tail=None),
        "unknown bits in mode": but(mode=FIRST),
        "unknown bits in mode ": but(mode=4),
        "span_cap > 0 with null spans": but(spans=None),
        "text_cap > 0 with null out_text": but(text=None),
        "offsets and out_offsets: one without the other": but(offsets=None),
        "offsets and out_offsets: one without the other ": but(out_offsets=None),
        "size > 0 with null raw": but(raw=None),
        "2^32 spans or strings or more": but(cap=1 << 32),
        "2^32 spans or strings or more ": but(n=1 << 32),
        "out_text overlaps the source": but(text=raw.ctypes.data + 4, text_cap=4),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_splice(*a[:12], flags, *a[12:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what.strip() in msg and msg.startswith("pire_hip_splice: "), (what, rc, msg)
    # host pointers: the list and the offsets are looked at
    for bad in ([3, 5, 1, 2], [1, 4, 3, 5], [2, 1, 3, 5], [1, 2, 3, 9]):
        rc = L.pire_hip_splice(*but(spans=np.array(bad, dtype=np.uint64).ctypes.data)[:12], 0, *ok[12:], None)
        assert rc == EINVAL and "spans must ascend" in L.pire_hip_last_error().decode(), bad
    for bad in ([0, 5, 3], [0, 3, 9]):
        assert L.pire_hip_splice(*but(offsets=np.array(bad, dtype=np.uint64).ctypes.data)[:12], 0, *ok[12:], None) == EINVAL, bad
    assert total.value == 79 and _untouched(bufs) and (raw == u8(b"a1b22c..")).all()
    with pytest.raises(pb.PireHipError, match="head_len > 256"):
        pb.splice(raw, [[1, 2]], head=b"x" * 257)


def test_search_lines_splice_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"a1 \n\n22\n").copy()
    tr, tf = TS.tables_of("num")
    head, tail = C.create_string_buffer(b"x" * 300), C.create_string_buffer(b"y" * 300)
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    names = ("rev", "fwd", "opts", "raw", "size", "delim", "head", "head_len", "tail", "tail_len", "mode", "lines", "spans", "pos", "cap", "count",
             "text", "text_cap", "bytes")
    ok = [tr._h, tf._h, 0, raw.ctypes.data, raw.size, 10, C.addressof(head), 1, C.addressof(tail), 1, KEEP | FIRST, C.addressof(lines),
          bufs["spans"].ctypes.data, bufs["pos"].ctypes.data, 4, C.addressof(cnt), bufs["text"].ctypes.data, 32, C.addressof(total)]
    but = lambda **kw: _but(names, ok, **kw)
    cases = {
        "null rev": but(rev=None),
        "null fwd": but(fwd=None),
        "unknown bits in opts": but(opts=8),
        "delim > 255": but(delim=300),
        "null out_line_count": but(lines=None),
        "size > 0 with null raw": but(raw=None),
        "null out_match_count": but(count=None),
        "null out_bytes": but(bytes=None),
        "head_len > 256": but(head_len=257),
        "tail_len > 256": but(tail_len=300),
        "head_len > 0 with null head": but(head=None),
        "tail_len > 0 with null tail": but(tail=None),
        "unknown bits in mode": but(mode=4),
        "text_cap > 0 with null out_text": but(text=None),
        "2^32 spans or strings or more": but(cap=1 << 32),
        "out_text overlaps the source": but(text=raw.ctypes.data + 4, text_cap=4),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_search_lines_splice(*a[:6], flags, *a[6:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_search_lines_splice: "), (what, rc, msg)
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)
    assert (raw == u8(b"a1 \n\n22\n")).all()
    # host pointers with size == 0: zeros, no device is touched
    for mode in (0, KEEP, FIRST, KEEP | FIRST):
        cnt.value, lines.value, total.value = 77, 78, 79
        assert L.pire_hip_search_lines_splice(*but(raw=None, size=0, mode=mode)[:6], 0, *but(raw=None, size=0, mode=mode)[6:], None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0) and _untouched(bufs)
    g = pb.search_lines_splice_host(tr, tf, b"", head=b"#")
    assert (g["lines"], g["count"], g["bytes"], g["text"].size) == (0, 0, 0, 0)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """splice.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "splice.hip" in ba.NO_SCRATCH and "splice.hip" in ba.UNITS and "splice" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bsplice\.hip\b", mk)) == 2                             # NAMES and AUDIT_UNITS
    names = re.search(r"^NAMES\s*:=(.*)$", mk, re.M).group(1).split()
    units = re.search(r"^AUDIT_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "splice.hip" in names and "splice.hip" in units
    fails, seen = ba.audit("splice.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Splice" in k for k in seen), seen                # sums, scan, positions, copy


def test_the_unit_names_no_kernel_reads_no_environment_and_has_no_assembly():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "splice.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "SelfTest" not in src
    assert "asm" not in src and "s_waitcnt" not in src and "atomic" not in src.replace("no atomics", "")
    assert src.count("__global__") == 4 and len(re.findall(r"void (Splice\w+Kernel)\(", src)) == 4
    for shared in ("BlockExclusive(", "WaveOwner(", "WaveBound<"):
        assert shared in src, shared
    assert not re.search(r"__forceinline__ \w+ (BlockExclusive|WaveOwner|WaveBound)\(", src)    # used, not copied
    assert '#include "compact.h"' in src


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

torch_cuda = TS.torch_cuda
stream_of, guarded, ptr_of, payload_of = TS.stream_of, TS.guarded, TS.ptr_of, TS.payload_of


def _ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _at(torch, data, off, device):
    """`data` at address offset `off` from a 16-byte boundary, device or host: (owner, pointer)"""
    a = np.full(data.size + 48, POISON, dtype=np.uint8)
    pad = (-a.ctypes.data) % 16 if not device else 0
    a[pad + off:pad + off + data.size] = data
    own = torch.as_tensor(a, device="cuda") if device else a
    assert (_ptr(own) + pad) % 16 == 0
    return own, _ptr(own) + pad + off, pad + off


def _u64(torch, values, device):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    a = a if a.size else np.zeros(1, dtype=np.uint64)
    return torch.as_tensor(a.view(np.int64), device="cuda") if device else a


def splice_call(torch, raw, spans, head=b"", tail=b"", mode=0, raw_off=0, out_off=0, text_cap=None, offsets=None, pos=True, device=True,
                count=None, cap=None, need=None, rc_only=False):
    """pire_hip_splice between guards, `raw` and out_text at the given address offsets from a 16-byte boundary: the outputs,
    after a synchronisation; the input compared with what went in.  need: the size of the result where text_cap is None."""
    raw = u8(raw) if not isinstance(raw, np.ndarray) else raw
    spans = np.asarray(spans, dtype=np.uint64).reshape(-1, 2)
    k = spans.shape[0]
    cap = k if cap is None else cap
    room = need if text_cap is None else text_cap
    own_raw, raw_ptr, raw_at = _at(torch, raw, raw_off, device)
    d_spans = _u64(torch, spans.reshape(-1), device)
    d_count = _u64(torch, [count], device) if count is not None else None
    d_offs = _u64(torch, offsets, device) if offsets is not None else None
    n = len(offsets) - 1 if offsets is not None else 0
    g_text = guarded(torch, out_off + room + 16, device)
    base = ptr_of(g_text) + (-ptr_of(g_text)) % 16                  # (a host array is aligned by hand)
    lead = base - ptr_of(g_text) + out_off
    bufs = {"text": g_text, "lead": lead, "room": room, "pos": guarded(torch, 8 * cap, device) if pos else None,
            "offsets": guarded(torch, 8 * (n + 1), device) if offsets is not None else None, "bytes": guarded(torch, 8, device)}
    rc = pb.lib().pire_hip_splice(raw_ptr if raw.size else None, raw.size, _ptr(d_spans) if cap else None, _ptr(d_count) if d_count is not None else None,
                                  cap, head or None, len(head), tail or None, len(tail), mode, _ptr(d_offs) if d_offs is not None else None, n,
                                  pb.FLAG_ON_DEVICE if device else 0, base + out_off if room else None, room,
                                  ptr_of(bufs["pos"]) if pos and cap else None, ptr_of(bufs["offsets"]) if offsets is not None else None,
                                  ptr_of(bufs["bytes"]), stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    back = own_raw.cpu().numpy() if device else own_raw
    assert (back[raw_at:raw_at + raw.size] == raw).all() and (np.delete(back, np.s_[raw_at:raw_at + raw.size]) == POISON).all(), "the input was written to"
    return bufs


def text_of(bufs, nbytes, what=""):
    """the first nbytes of out_text; everything around them is still poison"""
    a = payload_of(bufs["text"], bufs["lead"] + nbytes, what)
    assert (a[:bufs["lead"]] == POISON).all(), ("written in front of out_text", what)
    return a[bufs["lead"]:].tobytes()


def check_splice(bufs, exp, what, k=None, text_cap=None):
    k = len(exp["pos"]) if k is None else k
    assert payload_of(bufs["bytes"], 8, what).view(np.uint64)[0] == exp["bytes"], what             # the need, whatever the capacity
    written = exp["bytes"] if text_cap is None else min(exp["bytes"], text_cap)
    got = text_of(bufs, written, what)
    if got != exp["text"][:written]:
        bad = next(i for i in range(written) if got[i] != exp["text"][i])
        raise AssertionError((what, "differs first at byte %d of %d: %r expected %r" % (bad, written, got[bad:bad + 8], exp["text"][bad:bad + 8])))
    if bufs["pos"] is not None:
        assert (payload_of(bufs["pos"], 8 * k, what).view(np.uint64) == exp["pos"][:k]).all(), what
    if bufs["offsets"] is not None:
        got = payload_of(bufs["offsets"], 8 * len(exp["offsets"]), what).view(np.uint64)
        assert (got == exp["offsets"]).all(), (what, got.tolist()[:12], exp["offsets"].tolist()[:12])


def run_and_check(torch, raw, spans, head=b"", tail=b"", mode=0, what="", offsets=None, exp=None, **kw):
    exp = exp or model_splice(raw, spans, head, tail, mode, offsets)
    bufs = splice_call(torch, raw, spans, head, tail, mode, offsets=offsets, need=exp["bytes"], **kw)
    check_splice(bufs, exp, what)
    return exp


def some_bytes(size, seed=3):
    return np.random.RandomState(seed).randint(97, 123, size=size).astype(np.uint8).tobytes()


# ---- GPU: sizes, alignments, placements -----------------------------------------------------------------------------------------

SIZES = (0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
ALIGN = (0, 1, 7, 15)
PIECES = ((b"#", b"", 0), (b"", b"", 0), (b"<b>", b"</b>", KEEP), (b"0123456789abcdefg", b"", 0), (b"", b"xyz", KEEP), (b"", b"", KEEP))


def placements(size, out_off):
    """the span lists of the issue for a buffer of `size` bytes whose result lies out_off bytes behind a 16-byte boundary"""
    q = (16 - out_off) % 16 + 16                                    # a 16-byte boundary of the OUTPUT (nothing in front of it changes length)
    every = [(i, i + 1) for i in range(0, size, 2)]
    all_ = {"none": [], "first": [(0, 1)], "last": [(size - 1, size)], "whole": [(0, size)], "adjacent": [(1, 3), (3, 4)],
            "empty_at_0": [(0, 0)], "empty_at_size": [(size, size)], "two_empties": [(size // 2, size // 2)] * 2,
            "before": [(q - 1, q + 2)], "on": [(q, q + 3)], "after": [(q + 1, q + 4)], "every_second": every}
    return {k: v for k, v in all_.items() if all(0 <= b <= e <= size for b, e in v) and (v or k == "none")}


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_sizes_alignments_and_placements(torch_cuda, size):
    torch = torch_cuda
    raw = some_bytes(size, size)
    seen, turn = set(), 0
    for out_off in ALIGN:
        for kind, spans in placements(size, out_off).items():
            seen.add(kind)
            for raw_off in ALIGN:
                head, tail, mode = PIECES[turn % len(PIECES)]
                turn += 1
                run_and_check(torch, raw, spans, head, tail, mode, (size, kind, raw_off, out_off, head, tail, mode), raw_off=raw_off, out_off=out_off)
    want = {"none", "whole", "empty_at_0", "empty_at_size", "two_empties"}
    if size >= 1:
        want |= {"first", "last"}
    if size >= 17:                                                  # (the sizes that have room for them; size == 16: `adjacent` alone)
        want |= {"adjacent", "every_second"}
    if size >= TILE - 1:
        want |= {"before", "on", "after"}
    assert want <= seen, want - seen


@gpu
def test_host_pointers_at_every_size(torch_cuda):
    torch = torch_cuda
    for size in SIZES:
        raw = some_bytes(size, size + 1)
        for kind, spans in placements(size, 7).items():
            run_and_check(torch, raw, spans, b"<<", b">", KEEP if len(spans) % 2 else 0, (size, kind, "host"), raw_off=1, out_off=7, device=False)


# ---- GPU: the pieces ---------------------------------------------------------------------------------------------------------------

@gpu
def test_head_and_tail_lengths_with_and_without_keep(torch_cuda):
    torch = torch_cuda
    size = TILE + 1
    raw = some_bytes(size, 11)
    rng = np.random.RandomState(12)
    cuts = sorted(set(rng.randint(0, size, size=90).tolist()))
    spans = [(a, min(a + int(rng.randint(0, 40)), b)) for a, b in zip(cuts, cuts[1:] + [size])]
    spans[3] = (spans[3][0], spans[4][0])                           # two adjacent ones among them
    long_head, long_tail = some_bytes(256, 13).upper(), some_bytes(256, 14).upper()
    turn = 0
    for hl in (0, 1, 15, 16, 17, 40, 256):
        for tl in (0, 3, 256):
            for mode in (0, KEEP):
                off = ALIGN[turn % 4], ALIGN[(turn // 4) % 4]
                turn += 1
                run_and_check(torch, raw, spans, long_head[:hl], long_tail[256 - tl:], mode, (hl, tl, mode, off), raw_off=off[0], out_off=off[1])
                run_and_check(torch, raw, [(0, size)], long_head[:hl], long_tail[256 - tl:], mode, (hl, tl, mode, "whole"), out_off=off[1])
    exp = run_and_check(torch, raw, [(0, size)], what="the whole buffer deleted")
    assert exp["bytes"] == 0 and exp["text"] == b""


@gpu
def test_a_piece_of_512_bytes_for_every_byte_of_a_kib(torch_cuda):
    torch = torch_cuda
    raw = some_bytes(1024, 15)
    head, tail = some_bytes(256, 16).upper(), some_bytes(256, 17).upper()
    spans = [(i, i + 1) for i in range(1024)]
    for mode in (0, KEEP):
        exp = run_and_check(torch, raw, spans, head, tail, mode, ("expansion", mode), raw_off=7, out_off=1)
        assert exp["bytes"] == 1024 * (512 + (1 if mode else 0)) > 30 * TILE


# ---- GPU: span counts across the scan's tiles, more pieces in a tile than the stage holds ------------------------------------------

@gpu
@pytest.mark.parametrize("k", (1023, 1024, 1025, 2049))
def test_span_counts_across_the_tiles_of_the_scan(torch_cuda, k):
    torch = torch_cuda
    raw = some_bytes(3 * k + 2, k)
    spans = [(3 * j + 1, 3 * j + 2 + (j % 2)) for j in range(k)]   # 1 or 2 bytes, 1 or 2 kept bytes between them
    offsets = [0, 0, 1, 2] + list(range(4, 3 * k, 5)) + [3 * k + 2, 3 * k + 2]
    for head, tail, mode in ((b"-", b"", 0), (b"", b"", 0), (b"(", b")", KEEP)):
        run_and_check(torch, raw, spans, head, tail, mode, (k, head, tail, mode), offsets=offsets, out_off=7)
        run_and_check(torch, raw, spans, head, tail, mode, (k, head, tail, mode, "no offsets"), raw_off=15)


@gpu
def test_more_pieces_in_a_tile_than_the_stage_holds(torch_cuda):
    """spans of 1 byte replaced by nothing, one kept byte between them: 16 384 pieces in every output tile of 16 KiB, the
    stage holds 1 024 -- the copy reads positions and spans from global memory"""
    torch = torch_cuda
    size = 5 * TILE + 77
    raw = some_bytes(size, 21)
    spans = [(i, i + 1) for i in range(0, size, 2)]
    exp = run_and_check(torch, raw, spans, what="deleted", raw_off=1, out_off=15)
    assert exp["text"] == raw[1::2] and len(spans) > 2 * TILE
    run_and_check(torch, raw, spans, b"", b"", KEEP, what="a copy, piece by piece")
    run_and_check(torch, raw, spans + [(size, size)], b"", b"!", what="one tail at the end", out_off=7)


# ---- GPU: truncation, the span count ------------------------------------------------------------------------------------------------

@gpu
def test_text_cap_below_the_need_and_span_count_around_span_cap(torch_cuda):
    torch = torch_cuda
    size = 2 * TILE + 100
    raw = some_bytes(size, 31)
    spans = [(i, i + 3) for i in range(5, size - 8, 97)]
    k = len(spans)
    for head, tail, mode in ((b"0123456789abcdefghij", b"", 0), (b"", b"", 0), (b"[", b"]", KEEP)):
        exp = model_splice(raw, spans, head, tail, mode)
        need = exp["bytes"]
        for device in (True, False):
            for cap in (need, need - 1, need - 17, 0):
                bufs = splice_call(torch, raw, spans, head, tail, mode, text_cap=cap, out_off=1, device=device)
                check_splice(bufs, exp, (head, mode, device, "text_cap", cap), text_cap=cap)
            # span_count below, at and above span_cap: k = min(*span_count, span_cap)
            for count, span_cap in ((k - 5, k), (k, k), (k + 9, k), (k, k - 5), (0, k)):
                used = min(count, span_cap)
                e = model_splice(raw, spans[:used], head, tail, mode)
                bufs = splice_call(torch, raw, spans, head, tail, mode, count=count, cap=span_cap, need=e["bytes"], device=device)
                check_splice(bufs, e, (head, mode, device, "span_count", count, span_cap), k=used)


# ---- GPU: offsets and positions -------------------------------------------------------------------------------------------------------

@gpu
def test_offsets_of_a_batch_and_positions(torch_cuda):
    torch = torch_cuda
    strings = [b"", b"abc", b"", b"", b"defgh", b"i", b"", b"jklmnopqrstuvwxyz0123456789", b"AB", b""]
    text, offs = H.pack(strings)
    raw, o = text.tobytes(), [int(x) for x in offs]
    lists = {
        "first and last byte of strings": [(o[1], o[1] + 1), (o[2] - 1, o[2]), (o[4], o[4] + 1), (o[5] - 1, o[5]), (o[5], o[6]), (o[8], o[8] + 1), (o[9] - 1, o[9])],
        "an empty span on a boundary": [(o[1], o[1]), (o[4], o[4]), (o[5], o[5]), (o[7], o[7]), (o[8], o[8]), (o[10], o[10])],
        "whole strings": [(o[1], o[2]), (o[4], o[5]), (o[7], o[8])],
        "none": [],
        "mixed": [(0, 0), (0, 1), (1, 1), (2, 3), (3, 3), (3, 3), (5, 8), (9, 9), (9, 12), (len(raw), len(raw))],
    }
    for what, spans in lists.items():
        for head, tail, mode in ((b"<<", b">", KEEP), (b"", b"", 0), (b"#", b"", 0)):
            for device in (True, False):
                for pos in (True, False):
                    run_and_check(torch, raw, spans, head, tail, mode, (what, head, mode, device, pos), offsets=o, pos=pos, device=device, out_off=1)
    # the odd case of the header: the insertion at the end of "abc" is the next string's
    m = model_splice(raw, [(o[2], o[2])], b"-", offsets=o)
    assert m["offsets"].tolist()[:5] == [0, 0, 3, 3, 3] and m["offsets"].tolist()[5] == o[5] + 1


# ---- GPU: host and device pointers, two calls back to back ------------------------------------------------------------------------------

@gpu
def test_host_pointers_and_device_pointers_give_the_same_bytes(torch_cuda):
    torch = torch_cuda
    raw = u8(b"\n".join(TS.log_lines(400))).copy()
    parts = TS.py_lines(raw)
    offs = H.pack(parts)[1]
    for name in ("num", "alt"):
        spans = TA.lists_of(TA.model_all(name, parts, 0), offs, shift=1)["spans"]
        assert len(spans) > 50
        for head, tail, mode in ((b"#", b"", 0), (b"\x1b[1m", b"\x1b[0m", KEEP)):
            exp = model_splice(raw.tobytes(), spans.tolist(), head, tail, mode)
            got = {}
            for device in (True, False):
                bufs = splice_call(torch, raw, spans, head, tail, mode, need=exp["bytes"], device=device, out_off=7)
                check_splice(bufs, exp, (name, head, device))
                got[device] = text_of(bufs, exp["bytes"])
            assert got[True] == got[False]
            w = pb.splice(raw, spans, head, tail, mode)
            assert w["text"].tobytes() == exp["text"] and w["bytes"] == exp["bytes"] and (w["pos"] == exp["pos"]).all()


@gpu
def test_two_device_calls_back_to_back_leave_nothing_stale(torch_cuda):
    """out_pos is null: both calls keep their positions in stream-ordered scratch, the second gets the first one's block"""
    torch = torch_cuda
    size = 3 * TILE
    raw = some_bytes(size, 41)
    first = [(i, i + 2) for i in range(0, size - 2, 5)]
    second = [(i, i + 1) for i in range(3, size - 2, 7)]
    e1, e2 = model_splice(raw, first, b"12345"), model_splice(raw, second, b"", b"!", KEEP)
    d_raw = torch.as_tensor(u8(raw).copy(), device="cuda")
    d1, d2 = _u64(torch, np.array(first).reshape(-1), True), _u64(torch, np.array(second).reshape(-1), True)
    for _ in range(2):
        t1, t2 = guarded(torch, e1["bytes"]), guarded(torch, e2["bytes"])
        b1, b2 = guarded(torch, 8), guarded(torch, 8)
        stream = stream_of(torch) or 0
        pb.splice_device(d_raw.data_ptr(), size, d1.data_ptr(), len(first), ptr_of(b1), head=b"12345", out_text_ptr=ptr_of(t1),
                         text_cap=e1["bytes"], stream=stream)
        pb.splice_device(d_raw.data_ptr(), size, d2.data_ptr(), len(second), ptr_of(b2), tail=b"!", mode=KEEP, out_text_ptr=ptr_of(t2),
                         text_cap=e2["bytes"], stream=stream)
        torch.cuda.synchronize()
        assert payload_of(t1, e1["bytes"]).tobytes() == e1["text"] and payload_of(t2, e2["bytes"]).tobytes() == e2["text"]
        assert payload_of(b1, 8).view(np.uint64)[0] == e1["bytes"] and payload_of(b2, 8).view(np.uint64)[0] == e2["bytes"]
    assert (d_raw.cpu().numpy() == u8(raw)).all()


@gpu
def test_a_shuffled_list_on_device_pointers_stays_inside_its_buffers(torch_cuda):
    """the list breaks the promise: the call returns 0, the guards and the input are intact, nothing else is asserted"""
    torch = torch_cuda
    size = 2 * TILE + 9
    raw = some_bytes(size, 51)
    spans = np.array([(i, i + 4) for i in range(0, size - 4, 11)], dtype=np.uint64)
    rng = np.random.RandomState(52)
    shuffled = spans[rng.permutation(len(spans))]
    shuffled[::7] = shuffled[::7][:, ::-1]                          # some of them end in front of their begin
    shuffled[5] = (size - 2, size + 40)                             # ... and one leaves the buffer
    shuffled[9] = (1 << 40, (1 << 40) + 3)
    offsets = [0, 100, 50, size]
    for head, tail, mode in ((b"0123456789", b"", 0), (b"", b"", 0), (b"<", b">", KEEP)):
        for cap in (size, size + 20 * len(spans)):
            bufs = splice_call(torch, raw, shuffled, head, tail, mode, text_cap=cap, offsets=offsets, raw_off=1, out_off=7)
            payload_of(bufs["text"], bufs["lead"] + cap), payload_of(bufs["pos"], 8 * len(spans))
            payload_of(bufs["offsets"], 8 * len(offsets)), payload_of(bufs["bytes"], 8)


# ---- GPU: lines in, rewritten lines out --------------------------------------------------------------------------------------------------

def expected_lines(name, raw, opts, mode):
    """Python's split, the model on the lines: (lines, the spans counted in raw, the matches found)"""
    parts = TS.py_lines(raw)
    offs = H.pack(parts)[1]
    if mode & FIRST:
        begin, end, _, _ = TS.model_search(name, parts, opts)
        spans = TS.model_select(begin, end, offs, shift=1)["spans"]
    else:
        spans = TA.lists_of(TA.model_all(name, parts, opts), offs, shift=1)["spans"]
    return len(parts), spans


def lines_call(torch, name, raw, opts, head, tail, mode, cap, text_cap, device, lists=True):
    tr, tf = TS.tables_of(name)
    keep = torch.as_tensor(raw, device="cuda") if device else raw
    bufs = {"lines": guarded(torch, 8, device), "count": guarded(torch, 8, device), "bytes": guarded(torch, 8, device),
            "spans": guarded(torch, 16 * cap, device) if lists else None, "pos": guarded(torch, 8 * cap, device) if lists else None,
            "text": guarded(torch, text_cap, device), "lead": 0, "offsets": None}
    p = {k: (ptr_of(v) if v is not None and k != "lead" else None) for k, v in bufs.items()}
    rc = pb.lib().pire_hip_search_lines_splice(tr._h, tf._h, opts, _ptr(keep), len(raw), 10, pb.FLAG_ON_DEVICE if device else 0, head or None,
                                               len(head), tail or None, len(tail), mode, p["lines"], p["spans"], p["pos"], cap, p["count"],
                                               p["text"] if text_cap else None, text_cap, p["bytes"], stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device:
        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
    return bufs


def check_lines(bufs, nlines, spans, exp, cap, what):
    k = min(len(spans), cap)
    assert payload_of(bufs["lines"], 8, what).view(np.uint64)[0] == nlines, what
    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == len(spans), what               # the need
    if bufs["spans"] is not None:
        assert (payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2) == spans[:k]).all(), what
    check_splice(bufs, exp, what, k=k)


PROBE_RAW = u8(b"\n".join(TA.PROBES)).copy()


@gpu
@pytest.mark.parametrize("name,opts", (("num", 0), ("ipv4", 0), ("alt", 0), ("blanks_star", 0), ("bol", B)))
def test_lines_in_rewritten_lines_out(torch_cuda, name, opts):
    torch = torch_cuda
    raw = PROBE_RAW
    for mode in (0, KEEP, FIRST, KEEP | FIRST):
        nlines, spans = expected_lines(name, raw, opts, mode)
        assert len(spans) > 3, (name, mode)
        if mode & FIRST and name == "blanks_star":
            assert (spans[:, 0] == spans[:, 1]).any()                   # an empty first match is an insertion
        if not mode & FIRST:
            assert (spans[:, 0] < spans[:, 1]).all()                    # the list form never reports an empty match
        for head, tail in ((b"#", b""), (b"<b>", b"</b>"), (b"", b"")):
            full = model_splice(raw.tobytes(), spans.tolist(), head, tail, mode)
            room = len(raw) + (len(spans) + 2) * (len(head) + len(tail))
            for device in (True, False):
                for lists in (True, False):
                    bufs = lines_call(torch, name, raw, opts, head, tail, mode, len(spans) + 2, room, device, lists)
                    check_lines(bufs, nlines, spans, full, len(spans) + 2, (name, mode, head, device, lists))
                # match_cap below the need: the first match_cap matches are replaced, the rest is copied; the count is the need
                cap = len(spans) - 2
                part = model_splice(raw.tobytes(), spans[:cap].tolist(), head, tail, mode)
                bufs = lines_call(torch, name, raw, opts, head, tail, mode, cap, room, device)
                check_lines(bufs, nlines, spans, part, cap, (name, mode, head, device, "match_cap below the need"))
    # the wrapper
    nlines, spans = expected_lines(name, raw, opts, 0)
    g = pb.search_lines_splice_host(*TS.tables_of(name), raw, head=b"#", opts=opts)
    assert g["lines"] == nlines and g["count"] == len(spans) and (g["spans"] == spans).all()
    assert g["text"].tobytes() == model_splice(raw.tobytes(), spans.tolist(), b"#")["text"]


@gpu
def test_the_output_is_a_buffer_of_lines_again(torch_cuda):
    """num -> "#" on a log, every pointer the device's: the result is split again and scanned -- as many lines, no number left"""
    torch = torch_cuda
    tr, tf = TS.tables_of("num")
    raw = u8(b"\n".join(TS.log_lines()) + b"\n").copy()
    nlines, spans = expected_lines("num", raw, 0, 0)
    exp = model_splice(raw.tobytes(), spans.tolist(), b"#")
    assert nlines == 1000 and len(spans) > 300
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(raw, device="cuda")
    words = torch.full((5,), -1, dtype=torch.int64, device="cuda")      # lines, matches, bytes | lines again, matches again
    d_out = torch.full((len(raw) + 16,), POISON, dtype=torch.uint8, device="cuda")
    pb.search_lines_splice_device(tr, tf, d_raw.data_ptr(), len(raw), words.data_ptr(), words[1:].data_ptr(), words[2:].data_ptr(), head=b"#",
                                  match_cap=len(raw), out_text_ptr=d_out.data_ptr(), text_cap=len(raw), stream=stream)
    torch.cuda.synchronize()
    assert words[:3].cpu().tolist() == [nlines, len(spans), exp["bytes"]]
    got = d_out.cpu().numpy()
    assert got[:exp["bytes"]].tobytes() == exp["text"] and (got[exp["bytes"]:] == POISON).all()
    d_text = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(nlines + 1, dtype=torch.int64, device="cuda")
    pb.split_device(d_out.data_ptr(), exp["bytes"], words[3:].data_ptr(), out_text_ptr=d_text.data_ptr(), out_offsets_ptr=d_offs.data_ptr(),
                    offsets_cap=nlines, stream=stream)
    pb.search_all_device(tr, tf, d_text.data_ptr(), len(raw), d_offs.data_ptr(), nlines, words[4:].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert words[3:].cpu().tolist() == [nlines, 0]
    again = TS.py_lines(exp["text"])
    assert len(again) == nlines and (d_offs.cpu().numpy() == H.pack(again)[1].view(np.int64)).all()
