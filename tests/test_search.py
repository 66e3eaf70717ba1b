"""pire_hip_search, pire_hip_search_run_select and pire_hip_search_lines_gather: where the leftmost-longest match of a regexp
lies inside every string (line) of a batch -- on the device, both legs in one launch (search.hip).

Exact equality everywhere.  The expected values come from `model_search` -- the formulas of include/pire_hip.h written down over
the C oracle's LongestSuffix and LongestPrefix / ShortestPrefix (oracle.binding.OracleScanner.suffix / .prefix) --, which is
itself held against what the unmodified reference recorded in tests/golden/search/cases.json and against a brute-force
leftmost-longest search.  Python's `re.search` is leftmost-FIRST and is no model: `abc|abcabc|b+` on `abcabc` is [0, 6) here.
Nothing expected comes from the library.  Outputs sit between poisoned guard bytes.

The scanner pairs are tests/golden/search/* (tests/golden/make_search_inputs.py wrote them through the reference): `re` with
option n (F) and `(re).*` with options nr (R), neither Surround()ed."""
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
SEARCH = os.path.join(H.GOLDEN, "search")
POISON = 0xA5
GUARD = 64
EINVAL = -1
S, B, E = pb.SEARCH_SHORTEST, pb.SEARCH_THROUGH_BEGIN, pb.SEARCH_THROUGH_END
gpu = pytest.mark.gpu
NAMES = ("pire_hip_search", "pire_hip_search_run_select", "pire_hip_search_lines_gather")

with open(os.path.join(SEARCH, "cases.json")) as _f:
    CASES = json.load(_f)
PROBES = [bytes.fromhex(h) for h in CASES["probes_hex"]]
PAIRS = {c["name"]: c for c in CASES["pairs"]}
WORDS = [w.encode() for w in PAIRS["words"]["words"]]
_oracles, _tables = {}, {}


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def pattern_of(name):
    c = PAIRS[name]
    return c["pattern"] if c["pattern"] is not None else "|".join(c["words"])


def blobs_of(name):
    """(R, F): the blobs of the reversed `(re).*` and of `re`"""
    return H.load_blob(os.path.join("search", PAIRS[name]["rev"])), H.load_blob(os.path.join("search", PAIRS[name]["fwd"]))


def oracles_of(name):
    if name not in _oracles:
        r, f = blobs_of(name)
        _oracles[name] = (ob.OracleScanner(r), ob.OracleScanner(f))
    return _oracles[name]


def tables_of(name):
    if name not in _tables:
        r, f = blobs_of(name)
        _tables[name] = (pb.Table(r), pb.Table(f))
    return _tables[name]


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_search(name, strings, opts):
    """include/pire_hip.h, line by line: (begin i64[n], end i64[n], t i64[n], h i64[n]).  The tails are repacked as a batch of
    their own; two prefix calls cover B, picked per string by b_i == 0."""
    R, F = oracles_of(name)
    n = len(strings)
    text, offs = H.pack(strings)
    lens = np.array([len(s) for s in strings], dtype=np.int64)
    t = R.suffix(text, offs, True, bool(opts & E), bool(opts & B)) if n else np.zeros(0, np.int64)     # t_i
    b = lens - t                                                                                       # b_i (where t_i >= 0)
    cut = [s[int(bi):] if ti >= 0 else b"" for s, bi, ti in zip(strings, b, t)]
    ctext, coffs = H.pack(cut)
    if n:
        plain = F.prefix(ctext, coffs, not (opts & S), False, bool(opts & E))
        marked = F.prefix(ctext, coffs, not (opts & S), True, bool(opts & E)) if opts & B else plain
    else:
        plain = marked = np.zeros(0, np.int64)
    h = np.where(b == 0, marked, plain)                                                                # h_i
    found = (t >= 0) & (h >= 0)
    begin = np.where(found, b, -1).astype(np.int64)
    end = np.where(found, b + h, -1).astype(np.int64)
    for a in (begin, end):
        a.setflags(write=False)
    return begin, end, t, np.where(t >= 0, h, -1)


def brute_force(pattern, s):
    """leftmost-longest by definition: re.fullmatch over all (b, e), smallest b, then largest e"""
    rx = re.compile(pattern.encode(), re.S)
    for b in range(len(s) + 1):
        for e in range(len(s), b - 1, -1):
            if rx.fullmatch(s, b, e):
                return b, e
    return -1, -1


def model_select(begin, end, offs, shift=0):
    """pire_hip_capture_select on the search's positions, without the BeginMark shift and without Final: hits, spans, count"""
    sel = (begin >= 0) & (end >= 0)
    hits = np.flatnonzero(sel).astype(np.uint64)
    base = np.asarray(offs[:-1], dtype=np.uint64) + np.uint64(shift) * np.arange(len(begin), dtype=np.uint64)
    spans = np.stack([base[sel] + begin[sel].astype(np.uint64), base[sel] + end[sel].astype(np.uint64)], axis=1).reshape(-1, 2)
    return {"hits": hits, "spans": spans.astype(np.uint64), "count": int(hits.size)}


def py_lines(raw, delim=b"\n"):
    parts = bytes(raw).split(delim)
    if parts and parts[-1] == b"":
        parts.pop()
    return parts


# ---- CPU: the model against the reference's records and against brute force ----------------------------------------------------

def test_the_probes_cover_what_the_issue_lists():
    assert b"" in PROBES and any(len(p) == 1 for p in PROBES)
    for name in ("num", "stamp", "alt", "arrow", "gap"):
        c = PAIRS[name]
        rows = [(len(p), len(p) - t, len(p) - t + l) for p, t, l in zip(PROBES, c["tail"], c["longest"]) if t >= 0 and l >= 0]
        assert any(b == 0 and e < n for n, b, e in rows), name              # at 0
        assert any(b > 0 and e == n for n, b, e in rows), name              # at the end
        assert any(b == 0 and e == n and n for n, b, e in rows), name       # the whole string
        assert any(t < 0 for t in c["tail"]), name                          # none
    assert PAIRS["words"]["fwd_states"] > 255 and PAIRS["words"]["rev_states"] > 255
    assert PAIRS["eol"]["opts"] == E and PAIRS["bol"]["opts"] == B


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_the_model_against_what_the_reference_recorded(name):
    c = PAIRS[name]
    for shortest in (False, True):
        begin, end, t, h = model_search(name, PROBES, c["opts"] | (S if shortest else 0))
        assert t.tolist() == c["tail"], name
        assert h.tolist() == c["shortest" if shortest else "longest"], (name, shortest)
        lens = np.array([len(p) for p in PROBES])
        found = (np.array(c["tail"]) >= 0) & (h >= 0)
        assert (begin == np.where(found, lens - t, -1)).all() and (end == np.where(found, lens - t + h, -1)).all()
    if name == "alt":
        i = PROBES.index(b"abcabc")
        assert (model_search(name, PROBES, 0)[0][i], model_search(name, PROBES, 0)[1][i]) == (0, 6)
        assert re.search(pattern_of(name).encode(), b"abcabc").span() == (0, 3)      # leftmost-first: not a model
    if name == "blanks_star":
        begin, end, _, _ = model_search(name, PROBES, 0)
        assert (begin >= 0).all() and ((begin == 0) & (end == 0)).sum() > 10         # an empty match is a match


DRAW = {   # name -> (alphabet, planted samples)
    "num": (b"0123456789ab ", [b"7", b"42"]),
    "stamp": (b"0123456789-x", [b"2024-01-02", b"1999-12-31"]),
    "alt": (b"abcx", [b"abcabc", b"bb"]),
    "blanks_star": (b" \tab", [b"  "]),
    "arrow": (b"->x", [b"-->"]),
    "gap": (b"abxy", [b"ab"]),
    "words": (b"abcdefghij", WORDS[:40]),
}


def drawn_strings(name, n, max_len, seed):
    rng = np.random.RandomState(seed)
    alphabet, samples = DRAW[name]
    out = H.random_strings(rng, n, max_len, alphabet)
    for i in range(0, n, 2):                                # every other string: a sample planted somewhere
        s, w = out[i], samples[int(rng.randint(len(samples)))]
        at = int(rng.randint(0, len(s) + 1))
        out[i] = (s[:at] + w + s[at:])[:max_len]
    return out + [b""]


@pytest.mark.parametrize("name", sorted(DRAW))
def test_the_model_against_a_brute_force_leftmost_longest_search(name):
    strings = drawn_strings(name, 300, 12, 5)
    begin, end, _, _ = model_search(name, strings, 0)
    want = [brute_force(pattern_of(name), s) for s in strings]
    assert list(zip(begin.tolist(), end.tolist())) == want
    assert 20 < (begin >= 0).sum() and ((begin < 0).sum() > 20 or name in ("blanks_star", "alt", "gap", "num"))


# ---- CPU: the interface --------------------------------------------------------------------------------------------------------

FORMULAS = """
 *   t_i   = LongestSuffix(R, string i, throughEndMark = E, throughBeginMark = B)     length, or -1          run.h:313-341
 *   b_i   = len_i - t_i                                                              the leftmost start
 *   h_i   = S ? ShortestPrefix(F, string i from b_i, throughBeginMark = B && b_i == 0, throughEndMark = E)
 *             : LongestPrefix (F, string i from b_i, ...the same...)                 length, or -1          run.h:277-311
 *   found(i) = t_i >= 0 && h_i >= 0
 *   begin[i] = found ? b_i : -1        end[i] = found ? b_i + h_i : -1              positions inside the string
"""


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
    for macro, value in (("SHORTEST", S), ("THROUGH_BEGIN", B), ("THROUGH_END", E)):
        assert int(re.search(r"#define PIRE_HIP_SEARCH_%s (\d+)u" % macro, src).group(1)) == value
    for line in FORMULAS.strip("\n").splitlines():
        assert line in src, line
    assert "pire_hip_last_kernel() is not changed by the search" in src


def _guarded(cap=4):
    return {"hits": np.full(8 * (cap + 2), POISON, dtype=np.uint8), "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8),
            "begin": np.full(64, POISON, dtype=np.uint8), "end": np.full(64, POISON, dtype=np.uint8),
            "text": np.full(64, POISON, dtype=np.uint8), "offsets": np.full(8 * (cap + 3), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_search_refuses_before_any_device_is_touched():
    L = pb.lib()
    tr, tf = tables_of("num")
    text, offs = H.pack([b"a1", b"", b"22"])
    text = text.copy()
    bufs = _guarded()
    x, o, bp, ep = text.ctypes.data, offs.ctypes.data, bufs["begin"].ctypes.data, bufs["end"].ctypes.data
    cases = {
        "null rev": (None, tf._h, 0, x, o, 3, bp, ep),
        "null fwd": (tr._h, None, 0, x, o, 3, bp, ep),
        "unknown bits in opts": (tr._h, tf._h, 8, x, o, 3, bp, ep),
        "unknown bits in opts ": (tr._h, tf._h, 0x80000001, x, o, 3, bp, ep),
        "n > 0 with null text or offsets": (tr._h, tf._h, 0, None, o, 3, bp, ep),
        "n > 0 with null text or offsets ": (tr._h, tf._h, 0, x, None, 3, bp, ep),
        "null out_begin or out_end": (tr._h, tf._h, 0, x, o, 3, None, ep),
        "null out_begin or out_end ": (tr._h, tf._h, 0, x, o, 3, bp, None),
        "2^32 strings or more": (tr._h, tf._h, 0, x, o, 1 << 32, bp, ep),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_search(*a[:6], flags, *a[6:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what.strip() in msg and msg.startswith("pire_hip_search: "), (what, rc, msg)
    assert _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="unknown bits in opts"):
        pb.search(tr, tf, text, offs, opts=16)


def test_search_run_select_refuses_before_any_device_is_touched():
    L = pb.lib()
    tr, tf = tables_of("num")
    text, offs = H.pack([b"a1", b"", b"22"])
    text = text.copy()
    bufs, cnt = _guarded(), C.c_uint64(77)
    x, o, h, s, c = text.ctypes.data, offs.ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    # (rev, fwd, opts, text, offsets, n, out_hits, out_spans, hit_cap, out_hit_count)
    cases = {
        "null rev": (None, tf._h, 0, x, o, 3, h, s, 4, c),
        "null fwd": (tr._h, None, 0, x, o, 3, h, s, 4, c),
        "unknown bits in opts": (tr._h, tf._h, 0x10, x, o, 3, h, s, 4, c),
        "n > 0 with null text or offsets": (tr._h, tf._h, 0, None, o, 3, h, s, 4, c),
        "n > 0 with null text or offsets ": (tr._h, tf._h, 0, x, None, 3, h, s, 4, c),
        "null out_hit_count": (tr._h, tf._h, 0, x, o, 3, h, s, 4, None),
        "hit_cap > 0 with null out_hits and null out_spans": (tr._h, tf._h, 0, x, o, 3, None, None, 4, c),
        "2^32 strings or more": (tr._h, tf._h, 0, x, o, 1 << 32, h, s, 4, c),
    }
    bp, ep = bufs["begin"].ctypes.data, bufs["end"].ctypes.data
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            for positions in ((bp, ep), (None, None)):
                rc = L.pire_hip_search_run_select(*a[:6], flags, *positions, *a[6:], None)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what.strip() in msg and msg.startswith("pire_hip_search_run_select: "), (what, rc, msg)
    # host pointers: offsets that decrease (the scans' refusal, before any device)
    bad = np.array([0, 5, 3, 8], dtype=np.uint64)
    assert L.pire_hip_search_run_select(tr._h, tf._h, 0, x, bad.ctypes.data, 3, 0, None, None, h, s, 4, c, None) == EINVAL
    assert L.pire_hip_search(tr._h, tf._h, 0, x, bad.ctypes.data, 3, 0, bp, ep, None) == EINVAL
    assert cnt.value == 77 and _untouched(bufs)


def test_search_lines_gather_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"a1 \n\n22\n").copy()
    tr, tf = tables_of("num")
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    r, lp, h, s, c = raw.ctypes.data, C.addressof(lines), bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    x, xo, bp = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data, C.addressof(total)
    names = ("rev", "fwd", "opts", "raw", "size", "delim", "tail_byte", "lines", "hits", "spans", "cap", "count", "text", "text_cap", "offsets",
             "bytes")
    ok = [tr._h, tf._h, 0, r, raw.size, 10, 10, lp, h, s, 4, c, x, 32, xo, bp]

    def but(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    cases = {
        "null rev": but(rev=None),
        "null fwd": but(fwd=None),
        "unknown bits in opts": but(opts=8),
        "null out_hit_count": but(count=None),
        "hit_cap > 0 with null out_hits and null out_spans": but(hits=None, spans=None, text=None, text_cap=0, offsets=None, bytes=None),
        "delim > 255": but(delim=300),
        "null out_line_count": but(lines=None),
        "size > 0 with null raw": but(raw=None),
        "null out_bytes": but(bytes=None),
        "tail > 255": but(tail_byte=256),
        "idx_cap > 0 with null out_offsets (idx_cap = hit_cap)": but(offsets=None),
        "text_cap > 0 with null out_text": but(text=None),
        "out_text overlaps the source": but(text=r + 4, text_cap=4),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_search_lines_gather(*a[:6], flags, *a[6:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_search_lines_gather: "), (what, rc, msg)
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)
    assert (raw == u8(b"a1 \n\n22\n")).all()


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    tr, tf = tables_of("num")
    offs0 = np.zeros(1, dtype=np.uint64)
    for opts in (0, S, B | E):
        bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
        h, s, c, lp = bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt), C.addressof(lines)
        bp, ep = bufs["begin"].ctypes.data, bufs["end"].ctypes.data
        for o in (None, offs0.ctypes.data):
            assert L.pire_hip_search(tr._h, tf._h, opts, None, o, 0, 0, bp, ep, None) == 0, L.pire_hip_last_error()
            cnt.value = 77
            assert L.pire_hip_search_run_select(tr._h, tf._h, opts, None, o, 0, 0, bp, ep, h, s, 4, c, None) == 0, L.pire_hip_last_error()
            assert cnt.value == 0
        cnt.value = 77
        assert L.pire_hip_search_lines_gather(tr._h, tf._h, opts, None, 0, 10, 0, 10, lp, h, s, 4, c, None, 0, None, None, None) == 0   # spans only
        assert (cnt.value, lines.value) == (0, 0)
        assert _untouched(bufs)
        cnt.value, lines.value = 77, 78
        assert L.pire_hip_search_lines_gather(tr._h, tf._h, opts, None, 0, 10, 0, 10, lp, h, s, 4, c, bufs["text"].ctypes.data, 32,
                                              bufs["offsets"].ctypes.data, C.addressof(total), None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0)
        assert bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
        bufs["offsets"][:8] = POISON
        assert _untouched(bufs)
    # the wrappers on nothing
    begin, end = pb.search(tr, tf, np.zeros(0, np.uint8), offs0)
    assert begin.size == 0 and end.size == 0
    got = pb.search_run_select(tr, tf, np.zeros(0, np.uint8), offs0)
    assert got["count"] == 0 and got["hits"].size == 0 and got["spans"].shape == (0, 2) and got["begin"].size == 0
    gg = pb.search_lines_gather_host(tr, tf, b"")
    assert gg["lines"] == 0 and gg["count"] == 0 and gg["bytes"] == 0 and gg["text"].size == 0 and gg["offsets"].tolist() == [0]
    assert pb.search_opts() == 0 and pb.search_opts(shortest=True, through_begin=True, through_end=True) == S | B | E


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """search.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "search.hip" in ba.NO_SCRATCH and "search.hip" in ba.UNITS and "search" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bsearch\.hip\b", mk)) == 2                             # NAMES and AUDIT_UNITS
    names = re.search(r"^NAMES\s*:=(.*)$", mk, re.M).group(1).split()
    units = re.search(r"^AUDIT_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "search.hip" in names and "search.hip" in units
    fails, seen = ba.audit("search.hip")
    assert not fails, fails
    assert len(seen) == 1 and "SearchKernel" in seen[0], seen                       # one kernel, both legs


def test_the_unit_names_no_kernel_reads_no_environment_and_shares_the_walks():
    csrc = os.path.join(ROOT, "pire_amd", "csrc")
    with open(os.path.join(csrc, "search.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "SelfTest" not in src
    assert "asm" not in src and "s_waitcnt" not in src                              # plain HIP, compiler-placed waits
    assert src.count("__global__") == 1 and src.count("hipLaunchKernelGGL") == 1     # one kernel, one launch
    for shared in ("SuffixWalk(", "PrefixWalk(", "LoadTableToLds(", "MakeLayout("):
        assert shared in src, shared
    # the walks are exact.hip's own, moved, not copied: one definition, used by both units
    with open(os.path.join(csrc, "device_common.h")) as f:
        common = f.read()
    with open(os.path.join(csrc, "exact.hip")) as f:
        exact = f.read()
    for walk in ("SuffixWalk", "PrefixWalk"):
        assert len(re.findall(r"long long %s\(" % walk, common)) == 1 and walk + "(" in exact
        assert not re.search(r"long long %s\(" % walk, src) and not re.search(r"long long %s\(" % walk, exact)
    assert "alignbit" not in src and "WalkBlocks" not in src and "DenseChunk" not in src


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream or None


def guarded(torch, nbytes, device=True):
    a = np.full(2 * GUARD + nbytes, POISON, dtype=np.uint8)
    return torch.as_tensor(a, device="cuda") if device else a


def ptr_of(buf):
    return (buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data) + GUARD


def payload_of(buf, nbytes, what=""):
    """the bytes between the guards, after checking that the guards -- and everything behind nbytes -- are still poison"""
    a = buf.cpu().numpy() if hasattr(buf, "cpu") else buf
    assert (a[:GUARD] == POISON).all() and (a[GUARD + nbytes:] == POISON).all(), ("written outside its output", what)
    return a[GUARD:GUARD + nbytes].copy()


class Batch:
    """strings packed back to back inside a larger device buffer: `lead` in front of the first, `trail` behind the last"""

    def __init__(self, torch, strings, lead=b"", trail=b""):
        self.strings, self.n, self.lead = strings, len(strings), len(lead)
        text, offs = H.pack(strings)
        self.offs = offs + np.uint64(len(lead))
        self.host = u8(lead + text.tobytes() + trail).copy()
        self.d_text = torch.as_tensor(self.host if self.host.size else np.zeros(16, np.uint8), device="cuda")
        self.d_offs = torch.as_tensor(self.offs.view(np.int64), device="cuda")
        assert self.d_text.data_ptr() % 16 == 0                # a position in the buffer says where the 16-byte blocks lie


def device_search(torch, name, batch, opts, what=""):
    """pire_hip_search on device pointers: (begin, end), the guards checked, the text compared with what went in"""
    tr, tf = tables_of(name)
    n = batch.n
    d_b, d_e = guarded(torch, 8 * n), guarded(torch, 8 * n)
    pb.search_device(tr, tf, batch.d_text.data_ptr(), batch.d_offs.data_ptr(), n, ptr_of(d_b), ptr_of(d_e), opts, stream_of(torch) or 0)
    torch.cuda.synchronize()
    begin, end = payload_of(d_b, 8 * n, what).view(np.int64), payload_of(d_e, 8 * n, what).view(np.int64)
    if batch.host.size:
        assert (batch.d_text.cpu().numpy() == batch.host).all(), "the input was written to"
    return begin, end


def same(got, exp, strings, what):
    begin, end = got
    bad = np.flatnonzero((begin != exp[0]) | (end != exp[1]))
    assert bad.size == 0, (what, "%d of %d differ, first: string %d %r got [%d, %d) expected [%d, %d)" % (
        bad.size, len(begin), bad[0], strings[bad[0]][:80], begin[bad[0]], end[bad[0]], exp[0][bad[0]], exp[1][bad[0]]))


# ---- GPU: block edges of both legs ------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 100, 257)
EDGE = {   # name -> (filler alphabet: no byte of it starts or ends a match, the matches placed)
    "num": (b"xyz ", [b"7", b"2024", b"12345678901234567"]),
    "stamp": (b"xyz ", [b"2024-01-02"]),
    "alt": (b"xyz ", [b"abcabc", b"abc", b"bbbbb"]),
    "arrow": (b"xy >", [b"-->"]),
    "gap": (b"xyz ", [b"ab", b"axxxxxxxxxxxxxxxxxxb"]),
}


def edge_strings(name, lead):
    """every length crossed with every placement that fits in it; the strings go back to back behind `lead` bytes, so that their
    first bytes fall on every residue mod 16 and a placement can aim at the 16-byte blocks of the text's address"""
    alphabet, samples = EDGE[name]
    rng = np.random.RandomState(11)
    out, kinds, pos = [], [], lead
    for rnd in range(3):
        for L in sorted(set(LENGTHS) | {len(m) for m in samples}):   # (and the samples' own lengths: the whole string)
            for m in samples:
                k = len(m)
                q = (pos // 16 + 1) * 16 - pos                  # the first 16-byte boundary behind the string's first byte, inside it
                places = {"none": None, "at0": 0, "end": L - k, "whole": 0 if L == k else None, "straddle": q - max(k // 2, 1),
                          "before": q - 1 - k, "after": q + 1 - k, "straddle2": q + 16 - 1, "two": 1}
                for kind, at in places.items():
                    if kind != "none" and (at is None or at < 0 or at + k > L):
                        continue
                    s = bytearray(bytes(rng.choice(u8(alphabet), size=L)))
                    if kind != "none":
                        s[at:at + k] = m
                    if kind == "two":
                        if at + 2 * k + 1 > L:
                            continue
                        s[L - k:] = m                            # a second match at the end: the first must be reported
                    out.append(bytes(s))
                    kinds.append(kind)
                    pos += L
    return out, kinds


@gpu
@pytest.mark.parametrize("name", sorted(EDGE))
def test_block_edges_of_both_legs(torch_cuda, name):
    torch = torch_cuda
    strings, kinds = edge_strings(name, 0)
    assert {"none", "at0", "end", "whole", "straddle", "before", "after", "two"} <= set(kinds)
    starts = np.cumsum([0] + [len(s) for s in strings[:-1]])
    assert len({int(p) % 16 for p in starts}) == 16            # every residue mod 16
    batch = Batch(torch, strings)
    for opts in (0, S):
        exp = model_search(name, strings, opts)
        assert (exp[0] >= 0).sum() > len(strings) // 2 and (exp[0] < 0).sum() >= len(LENGTHS)
        same(device_search(torch, name, batch, opts), exp, strings, (name, opts))
    exp = model_search(name, strings, 0)
    two = [i for i, k in enumerate(kinds) if k == "two"]
    assert two and all(exp[0][i] == 1 for i in two)            # the first of two matches
    if name == "alt":
        # leftmost-LONGEST: on the abcabc rows `end` is not what a leftmost-first engine says
        rows = [i for i, s in enumerate(strings) if b"abcabc" in s and b"abcabc" == s[exp[0][i]:exp[0][i] + 6]]
        assert len(rows) > 20
        got = device_search(torch, name, batch, 0)
        for i in rows:
            first = re.search(pattern_of(name).encode(), strings[i])
            assert first.start() == got[0][i] and first.end() == got[0][i] + 3 and got[1][i] == got[0][i] + 6


# ---- GPU: empty matches and marks -----------------------------------------------------------------------------------------

def mixed_strings(seed, n=700):
    rng = np.random.RandomState(seed)
    out = H.random_strings(rng, n, 70, b"abcxyz \t09-")
    for i in range(0, n, 5):
        out[i] = b""
    for i in range(1, n, 5):
        out[i] = b" \t " + out[i]
    for i in range(2, n, 5):
        out[i] = out[i] + b" tail"
    return out


@gpu
def test_empty_matches_and_marks(torch_cuda):
    torch = torch_cuda
    strings = mixed_strings(3)
    batch = Batch(torch, strings)
    # blanks_star: every string is found, many at [0, 0), the strings of length 0 among them
    exp = model_search("blanks_star", strings, 0)
    got = device_search(torch, "blanks_star", batch, 0)
    same(got, exp, strings, "blanks_star")
    empty = np.array([len(s) == 0 for s in strings])
    assert (got[0] >= 0).all() and ((got[0] == 0) & (got[1] == 0)).sum() > 200 and ((got[0] == 0) & (got[1] == 0))[empty].all()
    assert (got[1] > got[0]).sum() > 100
    # the marks: with their bit, and without it -- nothing is found
    for name, bit in (("eol", E), ("bol", B)):
        for opts in (bit, bit | S, 0, B | E):
            exp = model_search(name, strings, opts)
            got = device_search(torch, name, batch, opts)
            same(got, exp, strings, (name, opts))
            if opts in (bit, bit | S):
                assert 100 < (got[0] >= 0).sum() < len(strings)
            elif opts == 0:
                assert (got[0] < 0).all() and (got[1] < 0).all()
    bol = device_search(torch, "bol", batch, B)
    assert (bol[0][bol[0] >= 0] == 0).all()                     # ^: only at the string's first byte
    eol = device_search(torch, "eol", batch, E)
    lens = np.array([len(s) for s in strings])
    assert (eol[1][eol[0] >= 0] == lens[eol[0] >= 0]).all()     # $: only up to its last
    # num with SHORTEST: the first digit alone
    exp = model_search("num", strings, S)
    got = device_search(torch, "num", batch, S)
    same(got, exp, strings, "num shortest")
    found = got[0] >= 0
    assert found.sum() > 100 and (got[1][found] == got[0][found] + 1).all()
    longest = device_search(torch, "num", batch, 0)
    assert (longest[0] == got[0]).all() and (longest[1][found] > got[1][found]).sum() > 20


# ---- GPU: outside the dense rows ------------------------------------------------------------------------------------------

@gpu
def test_both_legs_outside_the_dense_rows(torch_cuda):
    """`words`: more than 255 states in both forms -- the walks leave the dense rows and step through the table in memory"""
    torch = torch_cuda
    rng = np.random.RandomState(23)
    strings = []
    for i in range(1500):
        parts = []
        for _ in range(int(rng.randint(0, 5))):
            parts.append(bytes(rng.choice(u8(b"abcdefghijxyz "), size=int(rng.randint(0, 30)))))
            w = WORDS[int(rng.randint(len(WORDS)))]
            parts.append(w if rng.rand() < 0.7 else w[:-1])
        strings.append(b"".join(parts))
    exp = model_search("words", strings, 0)
    assert 500 < (exp[0] >= 0).sum() < len(strings)
    for opts in (0, S):
        same(device_search(torch, "words", Batch(torch, strings), opts), model_search("words", strings, opts), strings, ("words", opts))
    # a control batch on which nothing matches
    control = H.random_strings(rng, 1500, 120, b"klmnopqrstuvwxyz ")
    got = device_search(torch, "words", Batch(torch, control), 0)
    same(got, model_search("words", control, 0), control, "control")
    assert (got[0] < 0).all() and (got[1] < 0).all()


# ---- GPU: wave, block and grid edges ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025))
def test_wave_and_block_edges(torch_cuda, n):
    torch = torch_cuda
    strings = H.random_strings(np.random.RandomState(n), n, 7, b"0123456789ab ")
    same(device_search(torch, "num", Batch(torch, strings), 0), model_search("num", strings, 0), strings, n)


@gpu
def test_the_grid_stride_loop_past_its_first_trip(torch_cuda):
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 1024 + 1025
    rng = np.random.RandomState(41)
    lens = rng.randint(0, 8, size=n)
    flat = rng.choice(u8(b"0123456789ab "), size=int(lens.sum())).tobytes()
    ends = np.cumsum(lens)
    strings = [flat[e - k:e] for e, k in zip(ends.tolist(), lens.tolist())]
    exp = model_search("num", strings, 0)
    got = device_search(torch, "num", Batch(torch, strings), 0)
    same(got, exp, strings, n)
    assert (got[0][-1025:] >= 0).sum() > 300 and (got[0][-1025:] < 0).sum() > 50     # the last trip's strings among them


# ---- GPU: poisoned surroundings, both call forms --------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("lead", (1, 16, 37))
def test_poisoned_surroundings(torch_cuda, lead):
    """the bytes in front of the first string and behind the last one are digits: read as part of a string they would match"""
    torch = torch_cuda
    rng = np.random.RandomState(lead)
    strings = [b"xy", b""] + H.random_strings(rng, 200, 40, b"0123456789abc ") + [b"", b"ab"]
    batch = Batch(torch, strings, lead=b"7" * lead, trail=b"9" * 64)
    for opts in (0, S):
        exp = model_search("num", strings, opts)
        got = device_search(torch, "num", batch, opts)
        same(got, exp, strings, (lead, opts))
        assert got[0][0] == -1 and got[0][1] == -1 and got[0][-1] == -1 and got[0][-2] == -1


@gpu
def test_host_pointers_and_device_pointers_give_the_same_bits(torch_cuda):
    torch = torch_cuda
    for name, opts in (("num", 0), ("alt", 0), ("gap", S), ("eol", E), ("bol", B), ("words", 0)):
        strings = mixed_strings(9, 400) + [w + b" " for w in WORDS[:50]]
        exp = model_search(name, strings, opts)
        batch = Batch(torch, strings)
        one, two = device_search(torch, name, batch, opts), device_search(torch, name, batch, opts)
        assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
        text, offs = H.pack(strings)
        host = pb.search(*tables_of(name), text, offs, opts)
        assert host[0].tobytes() == one[0].tobytes() and host[1].tobytes() == one[1].tobytes()
        same(host, exp, strings, name)
    # the same table twice is legal (a pair that does not belong together: only what the header promises)
    tr, tf = tables_of("num")
    text, offs = H.pack([b"a1", b"22", b""])
    begin, end = pb.search(tf, tf, text, offs)
    assert ((begin >= 0) == (end >= 0)).all() and (begin <= end).all()
    assert pb.last_kernel() != "search"


# ---- GPU: the pass behind the search ------------------------------------------------------------------------------------------

def run_select_call(torch, name, batch, opts, cap, device, positions=True, hits=True, spans=True):
    tr, tf = tables_of(name)
    n = batch.n
    text, offs = H.pack(batch.strings)
    bufs = {"begin": guarded(torch, 8 * n, device) if positions else None, "end": guarded(torch, 8 * n, device) if positions else None,
            "hits": guarded(torch, 8 * cap, device) if hits and cap else None, "spans": guarded(torch, 16 * cap, device) if spans and cap else None,
            "count": guarded(torch, 8, device)}
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    tp, op = (batch.d_text.data_ptr(), batch.d_offs.data_ptr()) if device else (text.ctypes.data if text.size else None, offs.ctypes.data)
    rc = pb.lib().pire_hip_search_run_select(tr._h, tf._h, opts, tp, op, n, pb.FLAG_ON_DEVICE if device else 0, p["begin"], p["end"], p["hits"],
                                             p["spans"], cap, p["count"], stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    return bufs


@gpu
def test_run_select_below_at_and_above_the_count(torch_cuda):
    torch = torch_cuda
    strings = mixed_strings(13, 1500)
    batch = Batch(torch, strings, lead=b"5" * 21)
    _, offs = H.pack(strings)
    for name, opts in (("num", 0), ("gap", 0), ("eol", E | S)):
        begin, end, _, _ = model_search(name, strings, opts)
        count = int((begin >= 0).sum())
        assert 100 < count < len(strings)
        for device in (True, False):
            exp = model_select(begin, end, batch.offs if device else offs)
            # ... which is pire_hip_capture_select fed with the search's own begin / end
            got_b, got_e = device_search(torch, name, batch, opts)
            ch, cs, cc = pb.capture_select_host(batch.offs if device else offs, got_b, got_e, flags=0)
            assert cc == count and (ch == exp["hits"]).all() and (cs == exp["spans"]).all()
            for cap in (count - 1, count, count + 5, 0):
                for positions, hits, spans in ((True, True, True), (False, True, False), (False, False, True)):
                    what = (name, device, cap, positions, hits, spans)
                    bufs = run_select_call(torch, name, batch, opts, cap, device, positions, hits, spans)
                    k = min(count, cap)
                    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == count, what        # the whole total
                    if bufs["hits"] is not None:
                        assert (payload_of(bufs["hits"], 8 * k, what).view(np.uint64) == exp["hits"][:k]).all(), what
                    if bufs["spans"] is not None:
                        assert (payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2) == exp["spans"][:k]).all(), what
                    if positions:
                        assert (payload_of(bufs["begin"], 8 * batch.n, what).view(np.int64) == begin).all(), what
                        assert (payload_of(bufs["end"], 8 * batch.n, what).view(np.int64) == end).all(), what
    # the wrapper
    text, offs = H.pack(strings)
    begin, end, _, _ = model_search("num", strings, 0)
    got = pb.search_run_select(*tables_of("num"), text, offs)
    exp = model_select(begin, end, offs)
    assert got["count"] == exp["count"] and (got["hits"] == exp["hits"]).all() and (got["spans"] == exp["spans"]).all()
    assert (got["begin"] == begin).all() and (got["end"] == end).all()
    # n == 0 on the device: the count zeroed on the stream
    cnt = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    pb.search_run_select_device(*tables_of("num"), 0, batch.d_offs.data_ptr(), 0, cnt.data_ptr(), stream=stream_of(torch) or 0)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0]


# ---- GPU: lines in, matches out ---------------------------------------------------------------------------------------------

def log_lines(n=1000):
    rng = np.random.RandomState(29)
    out = H.random_strings(rng, n, 90, b"abcxyz .:-")
    for i in range(n):
        if i % 3 == 0:
            at = int(rng.randint(0, len(out[i]) + 1))
            out[i] = out[i][:at] + b"%d" % rng.randint(0, 10 ** int(rng.randint(1, 9))) + out[i][at:]
        if i % 7 == 0:
            out[i] = out[i] + b" 2024-01-%02d" % (i % 28 + 1) + b" and 1999-12-31"
        if i % 50 == 0:
            out[i] = b""
    return out


def expected_lines(name, raw, delim, opts):
    """Python's split, the model on the lines: the spans counted in raw, and the matches"""
    parts = py_lines(raw, bytes([delim]))
    begin, end, _, _ = model_search(name, parts, opts)
    exp = model_select(begin, end, H.pack(parts)[1], shift=1)
    texts = [parts[i][begin[i]:end[i]] for i in exp["hits"].tolist()]
    for (b, e), t in zip(exp["spans"].tolist(), texts):
        assert bytes(raw[b:e]) == t
    return len(parts), exp, texts


def lines_call(torch, name, raw, delim, opts, cap, device, gather=None, lists=True):
    """gather: None -- spans only --, or (tail_byte, text_cap)"""
    tr, tf = tables_of(name)
    keep = torch.as_tensor(raw, device="cuda") if device else raw
    tail_byte, text_cap = gather if gather else (0, 0)
    bufs = {"lines": guarded(torch, 8, device), "count": guarded(torch, 8, device),
            "hits": guarded(torch, 8 * cap, device) if lists else None, "spans": guarded(torch, 16 * cap, device) if lists else None,
            "text": guarded(torch, text_cap, device) if gather else None, "offsets": guarded(torch, 8 * (cap + 1), device) if gather else None,
            "bytes": guarded(torch, 8, device) if gather else None}
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    rc = pb.lib().pire_hip_search_lines_gather(tr._h, tf._h, opts, keep.data_ptr() if device else keep.ctypes.data, len(raw), delim,
                                               pb.FLAG_ON_DEVICE if device else 0, tail_byte, p["lines"], p["hits"], p["spans"], cap, p["count"],
                                               p["text"], text_cap, p["offsets"], p["bytes"], stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device:
        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
    return bufs


def check_lines(bufs, nlines, exp, cap, what, want=None, texts=None):
    k = min(exp["count"], cap)
    assert payload_of(bufs["lines"], 8, what).view(np.uint64)[0] == nlines, what
    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == exp["count"], what
    if bufs["hits"] is not None:
        assert (payload_of(bufs["hits"], 8 * k, what).view(np.uint64) == exp["hits"][:k]).all(), what
        assert (payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2) == exp["spans"][:k]).all(), what
    if want is not None:
        assert payload_of(bufs["bytes"], 8, what).view(np.uint64)[0] == len(want), what
        assert payload_of(bufs["text"], len(want), what).tobytes() == want, what
        ends = np.cumsum([0] + [len(t) + 1 for t in texts[:k]]).astype(np.uint64)
        assert (payload_of(bufs["offsets"], 8 * (k + 1), what).view(np.uint64) == ends).all(), what


@gpu
@pytest.mark.parametrize("name,opts", (("num", 0), ("stamp", 0), ("eol", E)))
def test_lines_in_first_matches_out(torch_cuda, name, opts):
    """`grep -o` for the first match of each line: 1 000 lines with \\n and a last line without one; a second delimiter"""
    torch = torch_cuda
    lines = log_lines()
    assert len(lines) == 1000 and lines[-1] != b""
    for raw, delim in ((u8(b"\n".join(lines)).copy(), 10), (u8(b"|".join(lines) + b"|").copy(), ord("|"))):
        nlines, exp, texts = expected_lines(name, raw, delim, opts)
        assert nlines == 1000 and 100 < exp["count"] < 1000
        for device in (True, False):
            for cap in (nlines, exp["count"] - 1):
                what = (name, delim, device, cap)
                k = min(exp["count"], cap)
                check_lines(lines_call(torch, name, raw, delim, opts, cap, device), nlines, exp, cap, what + ("spans only",))
                want = b"".join(t + bytes([delim]) for t in texts[:k])
                for lists in (True, False):
                    bufs = lines_call(torch, name, raw, delim, opts, cap, device, gather=(delim, len(raw) + cap), lists=lists)
                    check_lines(bufs, nlines, exp, cap, what + (lists,), want, texts)
    # the wrappers
    raw = u8(b"\n".join(lines)).copy()
    nlines, exp, texts = expected_lines(name, raw, 10, opts)
    g = pb.search_lines_gather_host(*tables_of(name), raw, opts=opts)
    assert g["lines"] == nlines and g["count"] == exp["count"] and (g["hits"] == exp["hits"]).all() and (g["spans"] == exp["spans"]).all()
    assert g["text"].tobytes() == b"".join(t + b"\n" for t in texts)
    g = pb.search_lines_gather_host(*tables_of(name), raw, opts=opts, gather=False, hit_cap=7)
    assert g["count"] == exp["count"] and (g["spans"] == exp["spans"][:7]).all() and "text" not in g


@gpu
def test_the_chain_by_hand_on_device_pointers(torch_cuda):
    """pire_hip_split -> pire_hip_search_run_select -> pire_hip_gather_spans, every pointer the device's and nothing read back in
    between: the bytes of the fused call"""
    torch = torch_cuda
    name = "num"
    tr, tf = tables_of(name)
    lines = log_lines()
    raw = u8(b"\n".join(lines) + b"\n").copy()
    nlines, exp, texts = expected_lines(name, raw, 10, 0)
    want = b"".join(t + b"\n" for t in texts)
    n = nlines
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(raw, device="cuda")
    d_text = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int64, device="cuda")   # n, the hit count, the bytes
    d_spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    d_out = torch.full((len(raw) + n,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    pb.split_device(d_raw.data_ptr(), len(raw), words.data_ptr(), out_text_ptr=d_text.data_ptr(), out_offsets_ptr=d_offs.data_ptr(),
                    offsets_cap=n, stream=stream)
    pb.search_run_select_device(tr, tf, d_text.data_ptr(), d_offs.data_ptr(), n, words[1:].data_ptr(), out_spans_ptr=d_spans.data_ptr(),
                                hit_cap=n, stream=stream)
    rc = pb.lib().pire_hip_gather_spans(d_text.data_ptr(), len(raw), d_spans.data_ptr(), words[1:].data_ptr(), n, 10, pb.FLAG_ON_DEVICE,
                                        d_out.data_ptr(), len(raw) + n, d_ends.data_ptr(), words[2:].data_ptr(), stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [n, exp["count"], len(want)]
    got = d_out.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()
    # ... which is what the fused call wrote
    bufs = lines_call(torch, name, raw, 10, 0, n, True, gather=(10, len(raw) + n))
    check_lines(bufs, n, exp, n, "fused", want, texts)
