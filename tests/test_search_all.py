"""pire_hip_search_all and pire_hip_search_all_lines_gather: EVERY leftmost-longest match of every string (line) of a batch -- on
the device, one backward pass that writes a mark bit per byte, then the forward leg over the marks (search_all.hip).

Exact equality everywhere.  The expected values come from `model_all` -- the loop of include/pire_hip.h written down over the C
oracle's LongestSuffix and LongestPrefix / ShortestPrefix, one call per round over all the strings that are still walking --,
which is itself held against what the unmodified reference recorded in tests/golden/search_all/cases.json
(tests/golden/make_search_all_inputs.py), against a brute-force iterated leftmost-longest search, against the mark formulation
the kernel uses, and against tests/test_search.py's model of the first match.  Nothing expected comes from the library.
Outputs sit between poisoned guard bytes.  The scanner pairs are tests/golden/search/*."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H
from tests import test_search as TS

ROOT = TS.ROOT
POISON, GUARD, EINVAL = TS.POISON, TS.GUARD, TS.EINVAL
S, B, E = TS.S, TS.B, TS.E
gpu = pytest.mark.gpu
u8 = TS.u8
NAMES = ("pire_hip_search_all", "pire_hip_search_all_lines_gather")

with open(os.path.join(H.GOLDEN, "search_all", "cases.json")) as _f:
    CASES = json.load(_f)
PROBES = [bytes.fromhex(h) for h in CASES["probes_hex"]]
RECORDS = {c["name"]: c for c in CASES["pairs"]}
_models = {}


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_all(name, strings, opts):
    """include/pire_hip.h, line by line, for all strings at once: [[(begin, end), ...] per string] (cached: computed once)"""
    key = (name, opts, hash(tuple(strings)), len(strings))
    if key in _models:
        return _models[key]
    R, F = TS.oracles_of(name)
    n = len(strings)
    p = [0] * n
    out = [[] for _ in range(n)]
    live = [i for i in range(n) if len(strings[i]) > 0]
    while live:                                                                 # while p < len
        text, offs = H.pack([strings[i][p[i]:] for i in live])
        plain = R.suffix(text, offs, True, bool(opts & E), False)
        marked = R.suffix(text, offs, True, bool(opts & E), True) if opts & B else plain
        t = [int(marked[k] if p[i] == 0 else plain[k]) for k, i in enumerate(live)]
        b = [len(strings[i]) - tk for i, tk in zip(live, t) if tk > 0]
        live = [i for i, tk in zip(live, t) if tk > 0]                          # t <= 0: stop
        if not live:
            break
        text, offs = H.pack([strings[i][bi:] for i, bi in zip(live, b)])
        plain = F.prefix(text, offs, not (opts & S), False, bool(opts & E))
        marked = F.prefix(text, offs, not (opts & S), True, bool(opts & E)) if opts & B else plain
        nxt = []
        for k, (i, bi) in enumerate(zip(live, b)):
            h = int(marked[k] if bi == 0 else plain[k])
            if h < 0:                                                           # h < 0: stop
                continue
            if h > 0:
                out[i].append((bi, bi + h))
            p[i] = bi + max(h, 1)
            if p[i] < len(strings[i]):
                nxt.append(i)
        live = nxt
    _models[key] = out
    return out


def lists_of(matches, offs, shift=0):
    """what the entry point writes: rows u64[n + 1], owners u64[m], spans u64[m, 2]"""
    counts = [len(m) for m in matches]
    rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    owners = np.repeat(np.arange(len(matches), dtype=np.uint64), counts)
    spans = np.array([(int(offs[i]) + shift * i + b, int(offs[i]) + shift * i + e) for i, m in enumerate(matches) for b, e in m],
                     dtype=np.uint64).reshape(-1, 2)
    return {"rows": rows, "owners": owners, "spans": spans, "count": int(rows[-1])}


def marks_model(name, s, opts):
    """the mark formulation of the header: one backward walk through R, then the forward leg from the next mark >= p"""
    R, F = TS.oracles_of(name)
    st = R.initial
    if opts & E:
        st = R.next(st, ob.END_MARK)
    marks, j = [False] * len(s), len(s)
    while j > 0 and not R.dead(st):
        st = R.next(st, s[j - 1])
        j -= 1
        marks[j] = R.final(st)
    if j == 0 and s and opts & B and R.final(R.next(st, ob.BEGIN_MARK)):
        marks[0] = True
    out, p = [], 0
    while p < len(s):
        b = next((k for k in range(p, len(s)) if marks[k]), None)
        if b is None:
            break
        text, offs = H.pack([s[b:]])
        h = int(F.prefix(text, offs, not (opts & S), bool(opts & B) and b == 0, bool(opts & E))[0])
        if h < 0:
            break
        if h > 0:
            out.append((b, b + h))
        p = b + max(h, 1)
    return out


def brute_force_all(pattern, s):
    """iterated leftmost-longest by definition; an empty match is dropped and stepped over"""
    rx = re.compile(pattern.encode(), re.S)
    out, p = [], 0
    while p < len(s):
        hit = next(((b, e) for b in range(p, len(s) + 1) for e in range(len(s), b - 1, -1) if rx.fullmatch(s, b, e)), None)
        if hit is None or hit[0] >= len(s):
            break
        if hit[1] > hit[0]:
            out.append(hit)
        p = hit[0] + max(hit[1] - hit[0], 1)
    return out


# ---- CPU: the model against the reference's records, brute force, the marks and the first match ----------------------------------

def test_the_records_cover_what_the_issue_lists():
    assert len(PROBES) == CASES["base_probes"] + 9 and PROBES[:CASES["base_probes"]] == TS.PROBES
    assert sorted(RECORDS) == sorted(TS.PAIRS)
    rec = lambda name, probe, key="matches": [tuple(m) for m in RECORDS[name][key][PROBES.index(probe)]]
    assert rec("num", b"a1b22c333") == [(1, 2), (3, 5), (6, 9)]
    assert rec("alt", b"abcabcabc bb abc") == [(0, 6), (6, 9), (10, 12), (13, 16)]
    assert rec("blanks_star", b"x  y \t") == [(1, 3), (4, 6)]
    assert rec("gap", b"a b a b") == [(0, 7)]
    assert rec("arrow", b"-->-->x-->") == [(0, 3), (3, 6), (7, 10)]
    assert len(rec("num", b" ".join(b"%d" % i for i in range(1, 41)))) == 40
    assert len(rec("stamp", PROBES[CASES["base_probes"] + 5])) == 3 and len(rec("ipv4", b"10.0.0.1 10.0.0.2, 192.168.1.254")) == 3
    assert len(rec("words", PROBES[-2])) == 8 and len(rec("words", PROBES[-1])) >= 4
    many = sum(len(m) > 1 for c in RECORDS.values() for key in ("matches", "matches_shortest") for m in c[key])
    assert many > 50


@pytest.mark.parametrize("name", sorted(TS.PAIRS))
def test_the_model_against_what_the_reference_recorded(name):
    c = RECORDS[name]
    assert c["opts"] == TS.PAIRS[name]["opts"]
    for key, opts in (("matches", c["opts"]), ("matches_shortest", c["opts"] | S)):
        got = model_all(name, PROBES, opts)
        assert [[list(m) for m in ms] for ms in got] == c[key], (name, key)
        for s, ms in zip(PROBES, got):                          # ascending, disjoint, not empty, inside the string
            flat = [x for m in ms for x in m]
            assert flat == sorted(flat) and all(b < e <= len(s) for b, e in ms)


def test_bol_matches_at_byte_0_only():
    s = [b"  lead  x"]
    assert model_all("bol", s, B) == [[(0, 2)]] and model_all("bol", s, 0) == [[]]


@pytest.mark.parametrize("name", sorted(TS.DRAW))
def test_the_model_against_a_brute_force_iterated_search(name):
    strings = TS.drawn_strings(name, 300, 12, 7)
    got = model_all(name, strings, 0)
    assert got == [brute_force_all(TS.pattern_of(name), s) for s in strings]
    if name in ("num", "alt", "blanks_star", "arrow"):          # (12 bytes hold one stamp, few words, and `a.*b` takes all there is)
        assert sum(len(m) > 1 for m in got) > 5


@pytest.mark.parametrize("name", sorted(TS.PAIRS))
def test_the_model_against_the_mark_formulation(name):
    own = TS.PAIRS[name]["opts"]
    strings = PROBES + (TS.drawn_strings(name, 60, 20, 3) if name in TS.DRAW else [])
    for opts in (own, own | S, 0):
        got = model_all(name, strings, opts)
        assert got == [marks_model(name, s, opts) for s in strings], (name, opts)


@pytest.mark.parametrize("name", sorted(TS.PAIRS))
def test_the_first_match_is_the_search_s_where_that_is_not_empty(name):
    own = TS.PAIRS[name]["opts"]
    for opts in (own, own | S):
        begin, end, _, _ = TS.model_search(name, PROBES, opts)
        for i, ms in enumerate(model_all(name, PROBES, opts)):
            if end[i] > begin[i]:
                assert ms and ms[0] == (begin[i], end[i]), (name, opts, PROBES[i])


# ---- CPU: the interface --------------------------------------------------------------------------------------------------------

FORMULAS = """
 *   p = 0, k = 0
 *   while p < len:
 *       t = LongestSuffix(R, s[p, len), throughEndMark = E, throughBeginMark = B && p == 0)      run.h:313-341
 *       if t <= 0: stop                      (t == 0: only the empty match at len is left)
 *       b = len - t
 *       h = S ? ShortestPrefix(F, s[b, len), throughBeginMark = B && b == 0, throughEndMark = E)
 *             : LongestPrefix (F, ...the same...)                                                 run.h:277-311
 *       if h < 0: stop                       (two tables that do not belong together)
 *       if h > 0: match k of the string = [b, b + h);  k += 1
 *       p = b + max(h, 1)
 *   LongestSuffix(R, s[p, len)) = len - min{ j >= p : mark(j) }
 *   mark(j) = Final(state after byte j) || (j == 0 && B && Final(Step(that state, BeginMark)))
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
    for line in FORMULAS.strip("\n").splitlines():
        assert line in src, line
    assert "Strings that OVERLAP in text" in src and "costs len steps per match" in src


def _guarded(n=3, cap=4):
    return {"rows": np.full(8 * (n + 3), POISON, dtype=np.uint8), "owners": np.full(8 * (cap + 2), POISON, dtype=np.uint8),
            "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8), "text": np.full(64, POISON, dtype=np.uint8),
            "offsets": np.full(8 * (cap + 3), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_search_all_refuses_before_any_device_is_touched():
    L = pb.lib()
    tr, tf = TS.tables_of("num")
    text, offs = H.pack([b"a1", b"", b"22"])
    text = text.copy()
    bufs, cnt = _guarded(), C.c_uint64(77)
    x, o, c = text.ctypes.data, offs.ctypes.data, C.addressof(cnt)
    r, w, s = bufs["rows"].ctypes.data, bufs["owners"].ctypes.data, bufs["spans"].ctypes.data
    # (rev, fwd, opts, text, text_bytes, offsets, n | rows, owners, spans, cap, count)
    cases = {
        "null rev": (None, tf._h, 0, x, 4, o, 3, r, w, s, 4, c),
        "null fwd": (tr._h, None, 0, x, 4, o, 3, r, w, s, 4, c),
        "unknown bits in opts": (tr._h, tf._h, 8, x, 4, o, 3, r, w, s, 4, c),
        "n > 0 with null text or offsets": (tr._h, tf._h, 0, None, 4, o, 3, r, w, s, 4, c),
        "n > 0 with null text or offsets ": (tr._h, tf._h, 0, x, 4, None, 3, r, w, s, 4, c),
        "2^32 strings or more": (tr._h, tf._h, 0, x, 4, o, 1 << 32, r, w, s, 4, c),
        "null out_match_count": (tr._h, tf._h, 0, x, 4, o, 3, r, w, s, 4, None),
        "match_cap > 0 with null out_owners and null out_spans": (tr._h, tf._h, 0, x, 4, o, 3, r, None, None, 4, c),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_search_all(*a[:7], flags, *a[7:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what.strip() in msg and msg.startswith("pire_hip_search_all: "), (what, rc, msg)
    # host pointers: offsets that decrease, an offset beyond text_bytes
    bad = np.array([0, 5, 3, 8], dtype=np.uint64)
    assert L.pire_hip_search_all(tr._h, tf._h, 0, x, 8, bad.ctypes.data, 3, 0, r, w, s, 4, c, None) == EINVAL
    assert L.pire_hip_search_all(tr._h, tf._h, 0, x, 3, o, 3, 0, r, w, s, 4, c, None) == EINVAL
    assert "an offset exceeds text_bytes" in L.pire_hip_last_error().decode()
    assert cnt.value == 77 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="unknown bits in opts"):
        pb.search_all(tr, tf, text, offs, opts=16)


def test_search_all_lines_gather_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"a1 \n\n22\n").copy()
    tr, tf = TS.tables_of("num")
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    r, lp, h, s, c = raw.ctypes.data, C.addressof(lines), bufs["owners"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    x, xo, bp = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data, C.addressof(total)
    names = ("rev", "fwd", "opts", "raw", "size", "delim", "tail_byte", "lines", "owners", "spans", "cap", "count", "text", "text_cap",
             "offsets", "bytes")
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
        "null out_match_count": but(count=None),
        "match_cap > 0 with null out_owners and null out_spans": but(owners=None, spans=None, text=None, text_cap=0, offsets=None, bytes=None),
        "delim > 255": but(delim=300),
        "null out_line_count": but(lines=None),
        "size > 0 with null raw": but(raw=None),
        "null out_bytes": but(bytes=None),
        "tail > 255": but(tail_byte=256),
        "idx_cap > 0 with null out_offsets (idx_cap = match_cap)": but(offsets=None),
        "text_cap > 0 with null out_text": but(text=None),
        "out_text overlaps the source": but(text=r + 4, text_cap=4),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_search_all_lines_gather(*a[:6], flags, *a[6:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_search_all_lines_gather: "), (what, rc, msg)
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)
    assert (raw == u8(b"a1 \n\n22\n")).all()


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    tr, tf = TS.tables_of("num")
    offs0 = np.zeros(1, dtype=np.uint64)
    for opts in (0, S, B | E):
        bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
        w, s, c, lp = bufs["owners"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt), C.addressof(lines)
        for o in (None, offs0.ctypes.data):
            cnt.value = 77
            assert L.pire_hip_search_all(tr._h, tf._h, opts, None, 0, o, 0, 0, None, w, s, 4, c, None) == 0, L.pire_hip_last_error()
            assert cnt.value == 0 and _untouched(bufs)
            cnt.value = 77
            assert L.pire_hip_search_all(tr._h, tf._h, opts, None, 0, o, 0, 0, bufs["rows"].ctypes.data, w, s, 4, c, None) == 0
            assert cnt.value == 0 and bufs["rows"].view(np.uint64)[0] == 0 and (bufs["rows"][8:] == POISON).all()
            bufs["rows"][:8] = POISON
        cnt.value = 77
        assert L.pire_hip_search_all_lines_gather(tr._h, tf._h, opts, None, 0, 10, 0, 10, lp, w, s, 4, c, None, 0, None, None, None) == 0
        assert (cnt.value, lines.value) == (0, 0) and _untouched(bufs)
        cnt.value, lines.value = 77, 78
        assert L.pire_hip_search_all_lines_gather(tr._h, tf._h, opts, None, 0, 10, 0, 10, lp, w, s, 4, c, bufs["text"].ctypes.data, 32,
                                                  bufs["offsets"].ctypes.data, C.addressof(total), None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0)
        assert bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
        bufs["offsets"][:8] = POISON
        assert _untouched(bufs)
    got = pb.search_all(tr, tf, np.zeros(0, np.uint8), offs0)
    assert got["count"] == 0 and got["rows"].tolist() == [0] and got["owners"] is None and got["spans"] is None
    gg = pb.search_all_lines_gather_host(tr, tf, b"")
    assert gg["lines"] == 0 and gg["count"] == 0 and gg["bytes"] == 0 and gg["text"].size == 0 and gg["offsets"].tolist() == [0]


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """search_all.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "search_all.hip" in ba.NO_SCRATCH and "search_all.hip" in ba.UNITS and "search_all" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bsearch_all\.hip\b", mk)) == 2                         # NAMES and AUDIT_UNITS
    names = re.search(r"^NAMES\s*:=(.*)$", mk, re.M).group(1).split()
    units = re.search(r"^AUDIT_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "search_all.hip" in names and "search_all.hip" in units
    fails, seen = ba.audit("search_all.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("SearchAll" in k for k in seen), seen             # marks + counts, two scans, the fill


def test_the_unit_names_no_kernel_reads_no_environment_and_has_no_assembly():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "search_all.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "SelfTest" not in src
    assert "asm" not in src and "s_waitcnt" not in src and "atomic" not in src.replace("no atomics", "")
    assert src.count("__global__") == 4
    for shared in ("PrefixWalk(", "LoadTableToLds(", "MakeLayout(", "BlockExclusive("):
        assert shared in src, shared
    assert not re.search(r"long long (Suffix|Prefix)Walk\(", src)                   # the shared walks are not copied


def test_the_search_s_own_units_are_what_the_parent_commit_has():
    """the new kernels live in a unit of their own: search.hip, exact.hip and device_common.h are untouched"""
    if not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("no history here")
    log = subprocess.run(["git", "-C", ROOT, "log", "--format=%H", "--", "pire_amd/csrc/search_all.hip"], stdout=subprocess.PIPE,
                         stderr=subprocess.DEVNULL, text=True)
    first = log.stdout.split()[-1] if log.returncode == 0 and log.stdout.split() else None     # the commit that added the unit ...
    base = first + "~" if first else "HEAD"                                                    # ... or, before it: the work tree's parent
    for unit in ("search.hip", "exact.hip", "device_common.h"):
        old = subprocess.run(["git", "-C", ROOT, "show", "%s:pire_amd/csrc/%s" % (base, unit)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        if old.returncode != 0:
            pytest.skip("no history here")
        with open(os.path.join(ROOT, "pire_amd", "csrc", unit), "rb") as f:
            assert f.read() == old.stdout, unit


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

torch_cuda = TS.torch_cuda
stream_of, guarded, ptr_of, payload_of, Batch = TS.stream_of, TS.guarded, TS.ptr_of, TS.payload_of, TS.Batch


def all_call(torch, name, batch, opts, cap, device=True, rows=True, owners=True, spans=True, text_bytes=None, n=None):
    """pire_hip_search_all between guards: the buffers, after a synchronisation; the input compared with what went in"""
    tr, tf = TS.tables_of(name)
    n = batch.n if n is None else n
    bufs = {"rows": guarded(torch, 8 * (n + 1), device) if rows else None, "owners": guarded(torch, 8 * cap, device) if owners else None,
            "spans": guarded(torch, 16 * cap, device) if spans else None, "count": guarded(torch, 8, device)}
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    if device:
        tp, op, size = batch.d_text.data_ptr(), batch.d_offs.data_ptr(), batch.host.size
    else:
        tp, op, size = (batch.host.ctypes.data if batch.host.size else None), batch.offs.ctypes.data, batch.host.size
    rc = pb.lib().pire_hip_search_all(tr._h, tf._h, opts, tp, size if text_bytes is None else text_bytes, op, n,
                                      pb.FLAG_ON_DEVICE if device else 0, p["rows"], p["owners"], p["spans"], cap, p["count"],
                                      stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device and batch.host.size:
        assert (batch.d_text.cpu().numpy() == batch.host).all(), "the input was written to"
    return bufs


def check_all(bufs, exp, cap, what):
    n = len(exp["rows"]) - 1
    k = min(exp["count"], cap)
    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == exp["count"], what           # the need, whatever the capacity
    if bufs["rows"] is not None:
        got = payload_of(bufs["rows"], 8 * (n + 1), what).view(np.uint64)
        bad = np.flatnonzero(got != exp["rows"])
        assert bad.size == 0, (what, "rows differ first at %d: %d expected %d" % (bad[0] if bad.size else -1, got[bad[0]] if bad.size else 0,
                                                                              exp["rows"][bad[0]] if bad.size else 0))
    if bufs["owners"] is not None:
        assert (payload_of(bufs["owners"], 8 * k, what).view(np.uint64) == exp["owners"][:k]).all(), what
    if bufs["spans"] is not None:
        got = payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2)
        bad = np.flatnonzero((got != exp["spans"][:k]).any(axis=1))
        assert bad.size == 0, (what, "%d spans of %d differ, first: match %d of string %d" % (bad.size, k, bad[0] if bad.size else -1,
                                                                                          exp["owners"][bad[0]] if bad.size else -1))


def device_all(torch, name, strings, opts, what="", batch=None):
    """device pointers, room for every match: checked against the model"""
    batch = batch or Batch(torch, strings)
    exp = lists_of(model_all(name, strings, opts), batch.offs)
    check_all(all_call(torch, name, batch, opts, exp["count"] + 3), exp, exp["count"] + 3, (name, opts, what))
    return exp


# ---- GPU: block edges --------------------------------------------------------------------------------------------------------

def edge_strings(name):
    """every length, three rounds back to back -- the starts fall on every residue mod 16 --, crossed with every placement
    that fits: aimed at the 16-byte blocks of the text's address"""
    alphabet, samples = TS.EDGE[name]
    rng = np.random.RandomState(17)
    out, kinds, pos = [], [], 0
    for rnd in range(3):
        for L in TS.LENGTHS:
            m = samples[(rnd + L) % len(samples)]
            k = len(m)
            q = (pos // 16 + 1) * 16 - pos                      # the first 16-byte boundary behind the string's first byte
            places = {"none": [], "at0": [0], "end": [L - k], "whole": [0] if L == k else None, "straddle": [q - max(k // 2, 1)],
                      "before": [q - 1 - k], "after": [q + 1 - k], "ends_on": [q - k], "back2back": [q - k, q],
                      "three": [0, (L - k) // 2, L - k] if 3 * k + 2 <= L else None,
                      "every": list(range((q - 1) % 16, L - k + 1, 16)) if k < 15 else None}
            for kind, ats in places.items():
                if ats is None or any(at < 0 or at + k > L for at in ats) or (kind != "none" and not ats):
                    continue
                s = bytearray(bytes(rng.choice(u8(alphabet), size=L)))
                for at in ats:
                    s[at:at + k] = m
                out.append(bytes(s))
                kinds.append(kind)
                pos += L
    return out, kinds


@gpu
@pytest.mark.parametrize("name", sorted(TS.EDGE))
def test_block_edges(torch_cuda, name):
    torch = torch_cuda
    strings, kinds = edge_strings(name)
    assert {"none", "at0", "end", "straddle", "before", "after", "ends_on", "back2back", "three", "every"} <= set(kinds)
    starts = np.cumsum([0] + [len(s) for s in strings[:-1]])
    assert len({int(p) % 16 for p in starts}) == 16            # every residue mod 16
    batch = Batch(torch, strings)
    for opts in (0, S):
        counts = np.array([len(m) for m in model_all(name, strings, opts)])
        if name != "gap" or opts == S:                          # (`a.*b` takes everything between the first a and the last b)
            assert (counts >= 3).sum() * 10 >= len(strings), (name, opts, (counts >= 3).sum(), len(strings))
        assert (counts > 0).sum() * 2 > len(strings) and (counts == 0).sum() >= 15
        device_all(torch, name, strings, opts, "edges", batch)


# ---- GPU: many strings in one block, many matches in one string --------------------------------------------------------------------

@gpu
def test_many_strings_in_one_block(torch_cuda):
    """2 000 strings of 0-3 bytes: neighbours share their mark blocks, runs of empty strings among them"""
    torch = torch_cuda
    rng = np.random.RandomState(5)
    strings = H.random_strings(rng, 2000, 3, b"1a ")
    for i in range(100, 140):
        strings[i] = b""
    exp = device_all(torch, "num", strings, 0)
    assert exp["count"] > 700 and sum(len(s) == 0 for s in strings) > 400
    device_all(torch, "num", strings, S)


@gpu
def test_many_matches_in_one_string(torch_cuda):
    torch = torch_cuda
    long = b"7 " * 4096
    exp = device_all(torch, "num", [long], 0)
    assert exp["count"] == 4096 and exp["spans"][:, 0].tolist() == list(range(0, 8192, 2))
    rng = np.random.RandomState(6)
    short = H.random_strings(rng, 100, 9, b"0123456789ab ")
    strings = short[:37] + [long] + short[37:]
    exp = device_all(torch, "num", strings, 0)
    assert exp["rows"][38] - exp["rows"][37] == 4096 and exp["count"] > 4096 + 50


# ---- GPU: marks and empties, stale marks ---------------------------------------------------------------------------------------------

@gpu
def test_marks_and_empty_matches(torch_cuda):
    torch = torch_cuda
    strings = TS.mixed_strings(3)
    batch = Batch(torch, strings)
    exp = device_all(torch, "blanks_star", strings, 0, batch=batch)     # every position is marked; the empty matches are dropped
    assert (exp["spans"][:, 1] > exp["spans"][:, 0]).all() and exp["count"] > 700
    for name, bit in (("eol", E), ("bol", B)):
        for opts in (bit, bit | S, 0, B | E):
            exp = device_all(torch, name, strings, opts, batch=batch)
            if opts in (bit, bit | S):
                assert 100 < exp["count"] < len(strings)
            elif opts == 0:
                assert exp["count"] == 0
    bol = lists_of(model_all("bol", strings, B), batch.offs)
    assert (bol["spans"][:, 0] == batch.offs[:-1][bol["owners"].astype(np.int64)]).all()       # ^: only at the string's first byte


@gpu
def test_stale_marks(torch_cuda):
    """blanks_star marks every position; `eol` directly behind it, same shapes, same stream, the same scratch: none of those
    marks may be read -- eol's backward walk dies at the first byte that is no letter and writes no marks below it"""
    torch = torch_cuda
    first = TS.mixed_strings(3)
    rng = np.random.RandomState(8)
    second = [bytes(rng.choice(u8(b"abc xyz.9 "), size=len(s))) for s in first]
    b1, b2 = Batch(torch, first), Batch(torch, second)
    e1 = lists_of(model_all("blanks_star", first, 0), b1.offs)
    e2 = lists_of(model_all("eol", second, E), b2.offs)
    assert e2["count"] > 100 and e1["count"] > 700
    for _ in range(2):
        got1 = all_call(torch, "blanks_star", b1, 0, e1["count"])
        got2 = all_call(torch, "eol", b2, E, e2["count"])
        check_all(got1, e1, e1["count"], "blanks_star")
        check_all(got2, e2, e2["count"], "eol behind blanks_star")


# ---- GPU: outside the dense rows -----------------------------------------------------------------------------------------------

@gpu
def test_both_legs_outside_the_dense_rows(torch_cuda):
    torch = torch_cuda
    rng = np.random.RandomState(23)
    strings = []
    for i in range(600):
        parts = []
        for _ in range(int(rng.randint(0, 5))):
            parts.append(bytes(rng.choice(u8(b"abcdefghijxyz "), size=int(rng.randint(0, 30)))))
            w = TS.WORDS[int(rng.randint(len(TS.WORDS)))]
            parts.append(w if rng.rand() < 0.7 else w[:-1])
        strings.append(b"".join(parts))
    exp = device_all(torch, "words", strings, 0)
    assert sum(1 for i in range(600) if exp["rows"][i + 1] - exp["rows"][i] > 1) > 100
    device_all(torch, "words", strings, S)


# ---- GPU: wave, block and grid edges ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_wave_block_and_tile_edges(torch_cuda, n):
    torch = torch_cuda
    strings = H.random_strings(np.random.RandomState(n), n, 9, b"0123456789ab ")
    device_all(torch, "num", strings, 0, n)


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
    exp = device_all(torch, "num", strings, 0, n)
    assert exp["rows"][-1] - exp["rows"][-1026] > 300          # the last trip's strings among them


# ---- GPU: capacity, pointer forms, clamping --------------------------------------------------------------------------------------------

@gpu
def test_capacity_below_at_and_above_the_count(torch_cuda):
    torch = torch_cuda
    strings = TS.mixed_strings(13, 1500)
    batch = Batch(torch, strings, lead=b"5" * 21, trail=b"9" * 40)
    for name, opts in (("num", 0), ("eol", E | S)):
        matches = model_all(name, strings, opts)
        for device in (True, False):
            exp = lists_of(matches, batch.offs)
            count = exp["count"]
            assert count > 300
            for cap in (count - 1, count, count + 5, 0, 1):
                for rows, owners, spans in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
                    what = (name, device, cap, rows, owners, spans)
                    check_all(all_call(torch, name, batch, opts, cap, device, rows, owners and cap > 0, spans and cap > 0), exp, cap, what)
            check_all(all_call(torch, name, batch, opts, 0, device, True, False, False), exp, 0, (name, device, "rows alone"))
            check_all(all_call(torch, name, batch, opts, 0, device, False, False, False), exp, 0, (name, device, "the count alone"))
    # n == 0 on the device: the count (and rows[0]) zeroed on the stream
    bufs = all_call(torch, "num", batch, 0, 4, True, n=0)
    assert payload_of(bufs["count"], 8).view(np.uint64)[0] == 0 and payload_of(bufs["rows"], 8).view(np.uint64)[0] == 0
    payload_of(bufs["owners"], 0), payload_of(bufs["spans"], 0)


@gpu
def test_host_pointers_and_device_pointers_give_the_same_bits(torch_cuda):
    torch = torch_cuda
    for name, opts in (("num", 0), ("alt", 0), ("gap", S), ("eol", E), ("bol", B), ("words", 0)):
        strings = TS.mixed_strings(9, 400) + [w + b" " + w for w in TS.WORDS[:50]]
        text, offs = H.pack(strings)
        exp = lists_of(model_all(name, strings, opts), offs)
        batch = Batch(torch, strings)
        cap = exp["count"] + 2
        one, two = all_call(torch, name, batch, opts, cap), all_call(torch, name, batch, opts, cap)
        for key, size in (("rows", 8 * (batch.n + 1)), ("owners", 8 * exp["count"]), ("spans", 16 * exp["count"]), ("count", 8)):
            assert payload_of(one[key], size).tobytes() == payload_of(two[key], size).tobytes(), (name, key)
        host = pb.search_all(*TS.tables_of(name), text, offs, opts)
        assert host["count"] == exp["count"] and (host["rows"] == exp["rows"]).all(), name
        assert (host["owners"] == exp["owners"]).all() and (host["spans"] == exp["spans"]).all(), name
        assert host["spans"].tobytes() == payload_of(one["spans"], 16 * exp["count"]).tobytes()
        few = pb.search_all(*TS.tables_of(name), text, offs, opts, match_cap=3, want_rows=False, want_owners=False)
        assert few["count"] == exp["count"] and (few["spans"] == exp["spans"][:3]).all() and few["rows"] is None
    assert pb.last_kernel() != "search_all"


@gpu
def test_offsets_beyond_text_bytes_are_clamped(torch_cuda):
    """the last offset lies beyond text_bytes: the last string is cut there, and the digits behind are not read as its bytes"""
    torch = torch_cuda
    rng = np.random.RandomState(12)
    strings = H.random_strings(rng, 300, 30, b"0123456789ab ") + [b"x 12 y 3456"]
    batch = Batch(torch, strings, trail=b"7" * 48)
    size = int(batch.offs[-1])
    for cut in (0, 1, 3, 11, 40):
        offs = batch.offs.copy()
        beyond = offs[-1] + np.uint64(37)
        text_bytes = size - cut
        clamped = [bytes(batch.host[min(int(a), text_bytes):min(int(b), text_bytes)]) for a, b in zip(offs[:-1], offs[1:])]
        offs[-1] = beyond
        batch.d_offs = torch.as_tensor(offs.view(np.int64), device="cuda")
        exp = lists_of(model_all("num", clamped, 0), np.minimum(offs, np.uint64(text_bytes)))
        check_all(all_call(torch, "num", batch, 0, exp["count"] + 1, text_bytes=text_bytes), exp, exp["count"] + 1, ("clamped", cut))


# ---- GPU: the first match is pire_hip_search's ---------------------------------------------------------------------------------------

@gpu
def test_the_first_match_is_what_pire_hip_search_says(torch_cuda):
    torch = torch_cuda
    strings = TS.mixed_strings(21, 600) + TS.log_lines(300)
    batch = Batch(torch, strings)
    for name, opts in (("num", 0), ("stamp", 0), ("blanks_star", 0), ("eol", E), ("bol", B), ("alt", S)):
        begin, end = TS.device_search(torch, name, batch, opts)
        matches = model_all(name, strings, opts)
        cap = sum(len(m) for m in matches)
        bufs = all_call(torch, name, batch, opts, cap)
        rows = payload_of(bufs["rows"], 8 * (batch.n + 1)).view(np.uint64)
        spans = payload_of(bufs["spans"], 16 * cap).view(np.uint64).reshape(-1, 2)
        some = 0
        for i in np.flatnonzero(end > begin).tolist():
            assert rows[i + 1] > rows[i], (name, i)
            first = spans[int(rows[i])]
            assert (int(first[0]), int(first[1])) == (int(batch.offs[i]) + begin[i], int(batch.offs[i]) + end[i]), (name, i)
            some += 1
        assert some > 30, name                                  # (42 lines carry a stamp)


# ---- GPU: lines in, every match out ---------------------------------------------------------------------------------------------

NO_TAIL = 0xFFFFFFFF


def expected_lines(name, raw, delim, opts):
    parts = TS.py_lines(raw, bytes([delim]))
    matches = model_all(name, parts, opts)
    exp = lists_of(matches, H.pack(parts)[1], shift=1)
    texts = [parts[i][b:e] for i, m in enumerate(matches) for b, e in m]
    for (b, e), t in zip(exp["spans"].tolist(), texts):
        assert bytes(raw[b:e]) == t
    return len(parts), exp, texts


def lines_call(torch, name, raw, delim, opts, cap, device, gather=None, lists=True):
    """gather: None -- spans only --, or (tail_byte, text_cap)"""
    tr, tf = TS.tables_of(name)
    keep = torch.as_tensor(raw, device="cuda") if device else raw
    tail_byte, text_cap = gather if gather else (0, 0)
    bufs = {"lines": guarded(torch, 8, device), "count": guarded(torch, 8, device),
            "owners": guarded(torch, 8 * cap, device) if lists else None, "spans": guarded(torch, 16 * cap, device) if lists else None,
            "text": guarded(torch, text_cap, device) if gather else None, "offsets": guarded(torch, 8 * (cap + 1), device) if gather else None,
            "bytes": guarded(torch, 8, device) if gather else None}
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    rc = pb.lib().pire_hip_search_all_lines_gather(tr._h, tf._h, opts, keep.data_ptr() if device else keep.ctypes.data, len(raw), delim,
                                                   pb.FLAG_ON_DEVICE if device else 0, tail_byte, p["lines"], p["owners"], p["spans"], cap,
                                                   p["count"], p["text"], text_cap, p["offsets"], p["bytes"],
                                                   stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device:
        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
    return bufs


def check_lines(bufs, nlines, exp, cap, what, tail=None, texts=None):
    k = min(exp["count"], cap)
    assert payload_of(bufs["lines"], 8, what).view(np.uint64)[0] == nlines, what
    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == exp["count"], what
    if bufs["owners"] is not None:
        assert (payload_of(bufs["owners"], 8 * k, what).view(np.uint64) == exp["owners"][:k]).all(), what
        assert (payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2) == exp["spans"][:k]).all(), what
    if texts is not None:
        want = b"".join(t + tail for t in texts[:k])
        assert payload_of(bufs["bytes"], 8, what).view(np.uint64)[0] == len(want), what
        assert payload_of(bufs["text"], len(want), what).tobytes() == want, what
        ends = np.cumsum([0] + [len(t) + len(tail) for t in texts[:k]]).astype(np.uint64)
        assert (payload_of(bufs["offsets"], 8 * (k + 1), what).view(np.uint64) == ends).all(), what


@gpu
@pytest.mark.parametrize("name,opts", (("num", 0), ("stamp", 0), ("eol", E)))
def test_lines_in_every_match_out(torch_cuda, name, opts):
    """`grep -o`: 1 000 lines with \\n and a last line without one; a second delimiter"""
    torch = torch_cuda
    lines = TS.log_lines()
    for raw, delim in ((u8(b"\n".join(lines)).copy(), 10), (u8(b"|".join(lines) + b"|").copy(), ord("|"))):
        nlines, exp, texts = expected_lines(name, raw, delim, opts)
        assert nlines == 1000 and exp["count"] > 100 and (name == "eol" or exp["count"] > len(set(exp["owners"].tolist())) + 100)
        if name in ("num", "stamp") and delim == 10:            # POSIX and Python agree on these two: `grep -o` itself
            found = [m.group() for ln in lines for m in re.finditer(TS.pattern_of(name).encode(), ln)]
            assert found == texts
        for device in (True, False):
            for cap in (exp["count"] + 7, exp["count"] - 1):
                what = (name, delim, device, cap)
                check_lines(lines_call(torch, name, raw, delim, opts, cap, device), nlines, exp, cap, what + ("spans only",))
                for tail_byte, tail in ((delim, bytes([delim])), (0, b"\0"), (NO_TAIL, b"")):
                    for lists in (True, False):
                        bufs = lines_call(torch, name, raw, delim, opts, cap, device, gather=(tail_byte, len(raw) + cap), lists=lists)
                        check_lines(bufs, nlines, exp, cap, what + (tail_byte, lists), tail, texts)
    raw = u8(b"\n".join(lines)).copy()
    nlines, exp, texts = expected_lines(name, raw, 10, opts)
    g = pb.search_all_lines_gather_host(*TS.tables_of(name), raw, opts=opts)
    assert g["lines"] == nlines and g["count"] == exp["count"] and (g["owners"] == exp["owners"]).all() and (g["spans"] == exp["spans"]).all()
    assert g["text"].tobytes() == b"".join(t + b"\n" for t in texts)
    g = pb.search_all_lines_gather_host(*TS.tables_of(name), raw, opts=opts, gather=False, match_cap=7)
    assert g["count"] == exp["count"] and (g["spans"] == exp["spans"][:7]).all() and "text" not in g


@gpu
def test_the_spans_feed_pire_hip_gather_spans(torch_cuda):
    """pire_hip_search_all -> pire_hip_gather_spans on device pointers, nothing read back in between: the bytes of the lines form"""
    torch = torch_cuda
    tr, tf = TS.tables_of("num")
    lines = TS.log_lines()
    raw = u8(b"\n".join(lines) + b"\n").copy()
    nlines, exp, texts = expected_lines("num", raw, 10, 0)
    want = b"".join(t + b"\n" for t in texts)
    batch = Batch(torch, lines)
    cap = exp["count"] + 3
    stream = torch.cuda.current_stream().cuda_stream
    words = torch.full((2,), -1, dtype=torch.int64, device="cuda")   # the match count, the bytes
    d_spans = torch.zeros((cap, 2), dtype=torch.int64, device="cuda")
    d_out = torch.full((batch.host.size + cap,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
    pb.search_all_device(tr, tf, batch.d_text.data_ptr(), batch.host.size, batch.d_offs.data_ptr(), batch.n, words.data_ptr(),
                         out_spans_ptr=d_spans.data_ptr(), match_cap=cap, stream=stream)
    rc = pb.lib().pire_hip_gather_spans(batch.d_text.data_ptr(), batch.host.size, d_spans.data_ptr(), words.data_ptr(), cap, 10,
                                        pb.FLAG_ON_DEVICE, d_out.data_ptr(), batch.host.size + cap, d_ends.data_ptr(), words[1:].data_ptr(),
                                        stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [exp["count"], len(want)]
    got = d_out.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()
    bufs = lines_call(torch, "num", raw, 10, 0, cap, True, gather=(10, len(raw) + cap))
    check_lines(bufs, nlines, exp, cap, "the lines form", b"\n", texts)
