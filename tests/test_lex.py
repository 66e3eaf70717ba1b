"""pire_hip_lex and pire_hip_lex_lines_gather: every leftmost-longest match of every string (line) WITH the regexps that accept
it, or -- PIRE_HIP_LEX_TOKENS -- the maximal-munch tokens of every string and the gaps between them (lex.hip).

Exact equality everywhere.  The expected values come from a model: the loops of include/pire_hip.h written down over the C
oracle's LongestSuffix and LongestPrefix / ShortestPrefix (search mode: tests/test_search_all.py's model_all on the set's two
tables) and its Next, Final and AcceptedRegexps for the masks.  The model is held against what the unmodified reference recorded
in tests/golden/lex/cases.json (tests/golden/make_lex_inputs.py).  Nothing expected comes from the library.  Outputs sit between
poisoned guard bytes."""
import collections
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
from tests import test_search as TS
from tests import test_search_all as TSA

ROOT = TS.ROOT
POISON, GUARD, EINVAL, EUNSUPPORTED = TS.POISON, TS.GUARD, TS.EINVAL, -5
S, B, E, T = 1, 2, 4, 8
gpu = pytest.mark.gpu
u8 = TS.u8
NAMES = ("pire_hip_lex", "pire_hip_lex_lines_gather")
NO_TAIL = 0xFFFFFFFF

with open(os.path.join(H.GOLDEN, "lex", "cases.json")) as _f:
    CASES = json.load(_f)
PROBES = [bytes.fromhex(h) for h in CASES["probes_hex"]]
SETS = {c["name"]: c for c in CASES["sets"]}
RUN = sorted(n for n in SETS if n != "r65")
WORDS = [w.encode() for w in CASES["words"]]
_oracles, _tables, _next, _cache = {}, {}, {}, {}


def oracles_of(name):
    """(R, F) of a set as C oracles; also known to tests/test_search.py under "lex/<name>", for model_all"""
    if name not in _oracles:
        c = SETS[name]
        _oracles[name] = (ob.OracleScanner(H.load_blob(os.path.join("lex", c["rev"]))), ob.OracleScanner(H.load_blob(os.path.join("lex", c["fwd"]))))
        TS._oracles["lex/" + name] = _oracles[name]
    return _oracles[name]


def tables_of(name):
    if name not in _tables:
        c = SETS[name]
        rev = pb.Table(H.load_blob(os.path.join("lex", c["rev"]))) if "rev" in c else None
        _tables[name] = (rev, pb.Table(H.load_blob(os.path.join("lex", c["fwd"]))))
    return _tables[name]


# ---- the model -----------------------------------------------------------------------------------------------------------

def _step(name, F, st, ch):
    key = (name, st, ch)
    if key not in _next:
        _next[key] = F.next(st, ch)
    return _next[key]


def mask_of(name, s, b, h, opts):
    """include/pire_hip.h: q = F's state after the h bytes; AcceptedRegexps(q) if Final(q), OR those behind the EndMark"""
    _, F = oracles_of(name)
    st = F.initial
    if opts & B and b == 0:
        st = _step(name, F, st, ob.BEGIN_MARK)
    for ch in s[b:b + h]:
        st = _step(name, F, st, ch)
    mask = sum(1 << r for r in F.accepted(st)) if F.final(st) else 0
    if opts & E and b + h == len(s):
        end = _step(name, F, st, ob.END_MARK)
        if F.final(end):
            mask |= sum(1 << r for r in F.accepted(end))
    return mask


def model(name, strings, opts):
    """[[(begin, end, mask), ...] per string] for `opts` (T among them or not); computed once"""
    key = (name, opts, hash(tuple(strings)), len(strings))
    if key in _cache:
        return _cache[key]
    _, F = oracles_of(name)
    if not opts & T:
        spans = TSA.model_all("lex/" + name, strings, opts)
        out = [[(b, e, mask_of(name, s, b, e - b, opts)) for b, e in ms] for s, ms in zip(strings, spans)]
    else:
        n = len(strings)
        p, gap, out = [0] * n, [None] * n, [[] for _ in range(n)]
        live = [i for i in range(n) if strings[i]]
        while live:                                                                  # while p < len
            text, offs = H.pack([strings[i][p[i]:] for i in live])
            plain = F.prefix(text, offs, not (opts & S), False, bool(opts & E))
            marked = F.prefix(text, offs, not (opts & S), True, bool(opts & E)) if opts & B else plain
            nxt = []
            for k, i in enumerate(live):
                h = int(marked[k] if p[i] == 0 else plain[k])
                if h > 0:
                    if gap[i] is not None:
                        out[i].append((gap[i], p[i], 0))
                        gap[i] = None
                    out[i].append((p[i], p[i] + h, mask_of(name, strings[i], p[i], h, opts)))
                    p[i] += h
                else:
                    gap[i] = p[i] if gap[i] is None else gap[i]
                    p[i] += 1
                if p[i] < len(strings[i]):
                    nxt.append(i)
                elif gap[i] is not None:
                    out[i].append((gap[i], len(strings[i]), 0))
            live = nxt
    _cache[key] = out
    return out


def lowest(mask):
    return (mask & -mask).bit_length() - 1


def lists_of(name, entries, offs, shift=0):
    """what the entry point writes: rows u64[n + 1], owners u64[m], spans u64[m, 2], masks u64[m], label_counts u64[R + 1]"""
    counts = [len(m) for m in entries]
    rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    owners = np.repeat(np.arange(len(entries), dtype=np.uint64), counts)
    spans = np.array([(int(offs[i]) + shift * i + b, int(offs[i]) + shift * i + e) for i, m in enumerate(entries) for b, e, _ in m],
                     dtype=np.uint64).reshape(-1, 2)
    masks = np.array([k for m in entries for _, _, k in m], dtype=np.uint64)
    R = SETS[name]["regexps"]
    tally = collections.Counter(lowest(k) if k else R for m in entries for _, _, k in m)
    labels = np.array([tally.get(r, 0) for r in range(R + 1)], dtype=np.uint64)
    return {"rows": rows, "owners": owners, "spans": spans, "masks": masks, "labels": labels, "count": int(rows[-1])}


# ---- CPU: the model against the reference's records ------------------------------------------------------------------------------

def rec(name, probe, key):
    return [(b, e, sum(1 << r for r in ids)) for b, e, ids in SETS[name][key][PROBES.index(probe)]]


def test_the_records_hold_the_values_the_header_quotes():
    assert PROBES[:CASES["base_probes"]] == TS.PROBES and len(PROBES) > CASES["base_probes"] + 8
    assert sorted(SETS) == sorted(["lexer3", "kw", "alt3", "ipnum", "eol", "ends", "bol", "words2", "r64", "r65"])
    assert rec("kw", b"if iffy 10 else x9", "search") == [(0, 2, 3), (3, 7, 2), (11, 15, 3), (16, 17, 2)]
    assert rec("alt3", b"abcabc bb abc", "search") == [(0, 6, 2), (7, 9, 4), (10, 13, 1)]
    assert rec("ipnum", b"from 10.0.0.1:80 x 10.0.0", "search") == [(5, 13, 1), (14, 16, 2), (19, 21, 2), (22, 23, 2), (24, 25, 2)]
    assert rec("lexer3", b"  ?? a1!", "tokens") == [(0, 2, 4), (2, 4, 0), (4, 5, 4), (5, 6, 1), (6, 7, 2), (7, 8, 0)]
    assert rec("eol", b"ab 12 cd", "tokens") == [(0, 3, 0), (3, 5, 2), (5, 6, 0), (6, 8, 1)]
    assert rec("eol", b"ab 12 cd", "search") == [(6, 8, 1)]                    # search mode sees only what accepts through the EndMark
    assert rec("ends", b"ab", "search") == [(0, 2, 3)] == rec("ends", b"ab", "tokens")
    assert rec("r64", b"k00 k63k01 k6", "search") == [(0, 3, 1), (4, 7, 1 << 63), (7, 10, 2)]
    assert rec("bol", b"#ab #c", "tokens") == [(0, 1, 1), (1, 3, 2), (3, 5, 0), (5, 6, 2)]
    assert (SETS["lexer3"]["fwd_states"], SETS["r64"]["fwd_states"]) == (5, 74)
    assert SETS["words2"]["fwd_states"] > 255 and SETS["words2"]["rev_states"] > 255
    assert SETS["r65"]["regexps"] == 65 and "rev" not in SETS["r65"]
    for name in RUN:
        assert [SETS[name]["opts"]] == [{"eol": E, "ends": E, "bol": B}.get(name, 0)]
        for key in ("search", "search_shortest", "tokens", "tokens_shortest"):
            assert all(ids or key.startswith("tokens") for es in SETS[name][key] for _, _, ids in es)     # a match's mask is never 0


@pytest.mark.parametrize("name", RUN)
def test_the_model_against_what_the_reference_recorded(name):
    own = SETS[name]["opts"]
    R, F = oracles_of(name)
    assert (R.size, F.size, F.regexps) == (SETS[name]["rev_states"], SETS[name]["fwd_states"], SETS[name]["regexps"])
    for key, opts in (("search", own), ("search_shortest", own | S), ("tokens", own | T), ("tokens_shortest", own | T | S)):
        got = model(name, PROBES, opts)
        assert got == [rec(name, p, key) for p in PROBES], (name, key)


@pytest.mark.parametrize("name", RUN)
def test_search_mode_is_model_all_and_token_mode_tiles(name):
    own = SETS[name]["opts"]
    oracles_of(name)
    for opts in (own, own | S):
        search = model(name, PROBES, opts)
        assert [[(b, e) for b, e, _ in es] for es in search] == TSA.model_all("lex/" + name, PROBES, opts)
        assert all(k for es in search for _, _, k in es)
        tokens = model(name, PROBES, opts | T)
        for s, es in zip(PROBES, tokens):                       # the entries tile [0, len), gaps are maximal
            assert [b for b, _, _ in es] == [0] * bool(s) + [e for _, e, _ in es][:-1] and (not es or es[-1][1] == len(s))
            assert all(b < e for b, e, _ in es) and not any(x[2] == 0 and y[2] == 0 for x, y in zip(es, es[1:]))
        if own & E:
            continue
        # without E: token mode minus its gaps is search mode.  With B there is one exception, which the reference's records
        # show on `ab12`: where the forward leg that took the BeginMark at byte 0 answers null, search mode stops (h < 0) and
        # token mode goes on behind a gap byte.
        for s, es, ms in zip(PROBES, tokens, search):
            kept = [x for x in es if x[2]]
            assert kept == ms or (own & B and ms == [] and es[0][0] == 0 and es[0][2] == 0), (name, opts, s)
    if not own & E:                                             # ... and with no bit set, for every set without exception
        for opts in (0, S):
            assert [[x for x in es if x[2]] for es in model(name, PROBES, opts | T)] == model(name, PROBES, opts), (name, opts)


def test_lowest_is_not_only():
    es = model("kw", [b"if iffy 10 else x9"], 0)[0]
    assert [lowest(k) for _, _, k in es] == [0, 1, 0, 1] and [k for _, _, k in es] == [3, 2, 3, 2]
    assert pb.lex_labels(np.array([3, 2, 0, 1 << 63], dtype=np.uint64)).tolist() == [0, 1, pb.LEX_GAP, 63]
    exp = lists_of("kw", model("kw", [b"if iffy 10 else x9", b"", b"while"], T), [0, 18, 18, 23])
    assert exp["labels"].tolist() == [3, 2, 4] and exp["rows"].tolist() == [0, 8, 8, 9]


# ---- CPU: the interface --------------------------------------------------------------------------------------------------------

FORMULAS = """
 *   q = F's state after the h bytes of the match, from Initialize() (+ Step(BeginMark) where the leg took the mark)
 *   mask = AcceptedRegexps(q) as bits                                  if Final(q)
 *   mask |= AcceptedRegexps(Step(q, EndMark)) as bits                  if E, the match ends at len and Final(Step(q, EndMark))
 *   p = 0
 *   while p < len:
 *       h = S ? ShortestPrefix(F, s[p, len), throughBeginMark = B && p == 0, throughEndMark = E)
 *       if h > 0: an entry [p, p + h) with its mask as above;  p += h
 *       else:     byte p is a gap byte;  p += 1
 *   a maximal run of gap bytes is ONE entry with mask 0
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
    assert (pb.LEX_SHORTEST, pb.LEX_THROUGH_BEGIN, pb.LEX_THROUGH_END, pb.LEX_TOKENS) == (S, B, E, T)
    for macro, value in (("SHORTEST", 1), ("THROUGH_BEGIN", 2), ("THROUGH_END", 4), ("TOKENS", 8)):
        assert re.search(r"#define PIRE_HIP_LEX_%s %du\b" % (macro, value), src)


def _guarded(n=3, cap=4, labels=3):
    return {"rows": np.full(8 * (n + 3), POISON, dtype=np.uint8), "owners": np.full(8 * (cap + 2), POISON, dtype=np.uint8),
            "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8), "masks": np.full(8 * (cap + 2), POISON, dtype=np.uint8),
            "labels": np.full(8 * (labels + 2), POISON, dtype=np.uint8), "text": np.full(64, POISON, dtype=np.uint8),
            "offsets": np.full(8 * (cap + 3), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_lex_refuses_before_any_device_is_touched():
    L = pb.lib()
    tr, tf = tables_of("kw")
    _, big = tables_of("r65")
    text, offs = H.pack([b"if", b"", b"x9"])
    text = text.copy()
    bufs, cnt = _guarded(), C.c_uint64(77)
    x, o, c = text.ctypes.data, offs.ctypes.data, C.addressof(cnt)
    r, w, s, m, lc = (bufs[k].ctypes.data for k in ("rows", "owners", "spans", "masks", "labels"))
    # (rev, fwd, opts, text, text_bytes, offsets, n | rows, owners, spans, masks, cap, count, labels)
    cases = {
        "unknown bits in opts": (tr._h, tf._h, 16, x, 4, o, 3, r, w, s, m, 4, c, lc),
        "null fwd": (tr._h, None, 0, x, 4, o, 3, r, w, s, m, 4, c, lc),
        "null fwd ": (None, None, T, x, 4, o, 3, r, w, s, m, 4, c, lc),
        "null rev without PIRE_HIP_LEX_TOKENS": (None, tf._h, 0, x, 4, o, 3, r, w, s, m, 4, c, lc),
        "n > 0 with null text or offsets": (tr._h, tf._h, 0, None, 4, o, 3, r, w, s, m, 4, c, lc),
        "2^32 strings or more": (tr._h, tf._h, T, x, 4, o, 1 << 32, r, w, s, m, 4, c, lc),
        "null out_match_count": (tr._h, tf._h, 0, x, 4, o, 3, r, w, s, m, 4, None, lc),
        "match_cap > 0 with null out_owners, out_spans and out_masks": (tr._h, tf._h, T, x, 4, o, 3, r, None, None, None, 4, c, lc),
    }
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_lex(*a[:7], flags, *a[7:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what.strip() in msg and msg.startswith("pire_hip_lex: "), (what, rc, msg)
    for opts, rev in ((0, tr._h), (T, None)):                   # 65 regexps: no accept masks
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_lex(rev, big._h, opts, x, 4, o, 3, flags, r, w, s, m, 4, c, lc, None) == EUNSUPPORTED
            assert "65 regexps" in L.pire_hip_last_error().decode()
    # host pointers: offsets that decrease, an offset beyond text_bytes
    bad = np.array([0, 5, 3, 8], dtype=np.uint64)
    assert L.pire_hip_lex(tr._h, tf._h, 0, x, 8, bad.ctypes.data, 3, 0, r, w, s, m, 4, c, lc, None) == EINVAL
    assert L.pire_hip_lex(None, tf._h, T, x, 3, o, 3, 0, r, w, s, m, 4, c, lc, None) == EINVAL
    assert "an offset exceeds text_bytes" in L.pire_hip_last_error().decode()
    assert cnt.value == 77 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="unknown bits in opts"):
        pb.lex(tr, tf, text, offs, opts=32)


def test_lex_refuses_a_simple_scanner_table():
    L = pb.lib()
    simple = [pb.Table(H.load_blob([c for c in H.golden()["simple"] if c["name"] == "simple_hello"][0]["blob"]))]
    assert simple[0].info.scanner_type == 2
    tr, tf = tables_of("kw")
    text, offs = H.pack([b"if"])
    text, cnt = text.copy(), C.c_uint64(77)
    m = np.full(8, POISON, dtype=np.uint8)
    for rev, fwd, opts in ((tr, simple[0], 0), (simple[0], tf, 0), (None, simple[0], T)):
        rc = L.pire_hip_lex(pb._table_ptr(rev), fwd._h, opts, text.ctypes.data, 2, offs.ctypes.data, 1, 0, None, None, None, m.ctypes.data, 1,
                            C.addressof(cnt), None, None)
        assert rc == EINVAL and "a SimpleScanner table" in L.pire_hip_last_error().decode()
    assert cnt.value == 77 and (m == POISON).all()


def test_lex_lines_gather_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"if x\n\n22\n").copy()
    tr, tf = tables_of("kw")
    _, big = tables_of("r65")
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    names = ("rev", "fwd", "opts", "raw", "size", "delim", "tail_byte", "lines", "owners", "spans", "masks", "cap", "count", "labels", "text",
             "text_cap", "offsets", "bytes")
    r = raw.ctypes.data
    ok = [tr._h, tf._h, 0, r, raw.size, 10, 10, C.addressof(lines), bufs["owners"].ctypes.data, bufs["spans"].ctypes.data,
          bufs["masks"].ctypes.data, 4, C.addressof(cnt), bufs["labels"].ctypes.data, bufs["text"].ctypes.data, 32, bufs["offsets"].ctypes.data,
          C.addressof(total)]

    def but(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    cases = {
        "unknown bits in opts": but(opts=16),
        "null fwd": but(fwd=None),
        "null rev without PIRE_HIP_LEX_TOKENS": but(rev=None),
        "null out_match_count": but(count=None),
        "match_cap > 0 with null out_owners, out_spans and out_masks": but(owners=None, spans=None, masks=None, text=None, text_cap=0, offsets=None,
                                                                          bytes=None),
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
            rc = L.pire_hip_lex_lines_gather(*a[:6], flags, *a[6:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_lex_lines_gather: "), (what, rc, msg)
    a = but(fwd=big._h)
    assert L.pire_hip_lex_lines_gather(*a[:6], 0, *a[6:], None) == EUNSUPPORTED
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    tr, tf = tables_of("kw")
    offs0 = np.zeros(1, dtype=np.uint64)
    for opts, rev in ((0, tr._h), (S, tr._h), (T, None), (T | B | E, tr._h)):
        bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
        w, s, m, c, lp = bufs["owners"].ctypes.data, bufs["spans"].ctypes.data, bufs["masks"].ctypes.data, C.addressof(cnt), C.addressof(lines)
        assert L.pire_hip_lex(rev, tf._h, opts, None, 0, offs0.ctypes.data, 0, 0, None, w, s, m, 4, c, None, None) == 0, L.pire_hip_last_error()
        assert cnt.value == 0 and _untouched(bufs)
        cnt.value = 77
        assert L.pire_hip_lex(rev, tf._h, opts, None, 0, None, 0, 0, bufs["rows"].ctypes.data, w, s, m, 4, c, bufs["labels"].ctypes.data, None) == 0
        assert cnt.value == 0 and bufs["rows"].view(np.uint64)[0] == 0 and (bufs["rows"][8:] == POISON).all()
        assert (bufs["labels"].view(np.uint64)[:3] == 0).all() and (bufs["labels"][24:] == POISON).all()      # R + 1 = 3 zeros
        bufs["rows"][:8] = POISON
        bufs["labels"][:24] = POISON
        cnt.value = 77
        assert L.pire_hip_lex_lines_gather(rev, tf._h, opts, None, 0, 10, 0, 10, lp, w, s, m, 4, c, bufs["labels"].ctypes.data, bufs["text"].ctypes.data,
                                           32, bufs["offsets"].ctypes.data, C.addressof(total), None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0) and (bufs["labels"].view(np.uint64)[:3] == 0).all()
        assert bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
        bufs["offsets"][:8] = POISON
        bufs["labels"][:24] = POISON
        assert _untouched(bufs)
    got = pb.lex(None, tf, np.zeros(0, np.uint8), offs0, opts=T)
    assert got["count"] == 0 and got["rows"].tolist() == [0] and got["masks"] is None and got["label_counts"].tolist() == [0, 0, 0]
    gg = pb.lex_lines_gather_host(tr, tf, b"")
    assert gg["lines"] == 0 and gg["count"] == 0 and gg["bytes"] == 0 and gg["label_counts"].tolist() == [0, 0, 0]


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """lex.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "lex.hip" in ba.NO_SCRATCH and "lex.hip" in ba.UNITS and "/ lex /" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\blex\.hip\b", mk)) == 2                                # NAMES and AUDIT_UNITS
    names = re.search(r"^NAMES\s*:=(.*)$", mk, re.M).group(1).split()
    units = re.search(r"^AUDIT_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert names.index("lex.hip") == names.index("search_all.hip") + 1 and units.index("lex.hip") == units.index("search_all.hip") + 1
    assert "match_loop.h" in re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1)
    fails, seen = ba.audit("lex.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Lex" in k for k in seen), seen                   # count and fill, search mode and token mode


def test_the_unit_shares_the_loop_and_has_no_global_atomics_or_assembly():
    csrc = os.path.join(ROOT, "pire_amd", "csrc")
    with open(os.path.join(csrc, "lex.hip")) as f:
        src = f.read()
    with open(os.path.join(csrc, "match_loop.h")) as f:
        shared = f.read()
    with open(os.path.join(csrc, "search_all.hip")) as f:
        base = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "SelfTest" not in src and "asm" not in src and "s_waitcnt" not in src
    assert src.count("atomicAdd(") == 1 and "atomicAdd(&tally[" in src and "__shared__ unsigned long long tally[" in src       # LDS only
    for fn in ("void StringOf(", "uint64_t MarkIndex(", "void MarkWalk(", "uint64_t MatchLoop("):
        assert fn in shared and fn not in src and fn not in base, fn                # one copy, in the header
    for call in ("StringOf(", "MarkWalk(", "MatchLoop(", "LaunchSearchAllRows("):
        assert call in src and call in base, call
    assert "BlockExclusive(" not in src                                              # the row scan is search_all.hip's


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

torch_cuda = TS.torch_cuda
stream_of, guarded, ptr_of, payload_of, Batch = TS.stream_of, TS.guarded, TS.ptr_of, TS.payload_of, TS.Batch
LISTS = ("rows", "owners", "spans", "masks", "labels")


def lex_call(torch, name, batch, opts, cap, device=True, want=LISTS, text_bytes=None, n=None, rev=True, offs=None):
    """pire_hip_lex between guards: the buffers, after a synchronisation; the input compared with what went in"""
    tr, tf = tables_of(name)
    n = batch.n if n is None else n
    R = SETS[name]["regexps"]
    sizes = {"rows": 8 * (n + 1), "owners": 8 * cap, "spans": 16 * cap, "masks": 8 * cap, "labels": 8 * (R + 1)}
    bufs = {k: (guarded(torch, sizes[k], device) if k in want and (cap or k in ("rows", "labels")) else None) for k in LISTS}
    bufs["count"] = guarded(torch, 8, device)
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    if device:
        d_offs = batch.d_offs if offs is None else torch.as_tensor(offs.view(np.int64), device="cuda")
        tp, op, size = batch.d_text.data_ptr(), d_offs.data_ptr(), batch.host.size
    else:
        spare = np.zeros(16, np.uint8)                          # (n > 0 wants a text pointer, also where every string is empty)
        tp, op, size = (batch.host.ctypes.data if batch.host.size else spare.ctypes.data), batch.offs.ctypes.data, batch.host.size
    rc = pb.lib().pire_hip_lex(tr._h if rev and tr is not None else None, tf._h, opts, tp, size if text_bytes is None else text_bytes, op, n,
                               pb.FLAG_ON_DEVICE if device else 0, p["rows"], p["owners"], p["spans"], p["masks"], cap, p["count"], p["labels"],
                               stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device and batch.host.size:
        assert (batch.d_text.cpu().numpy() == batch.host).all(), "the input was written to"
    return bufs


def check_lex(bufs, exp, cap, what):
    n = len(exp["rows"]) - 1
    k = min(exp["count"], cap)
    got = int(payload_of(bufs["count"], 8, what).view(np.uint64)[0])
    assert got == exp["count"], (what, got, exp["count"])                                        # the need, whatever the capacity
    if bufs["labels"] is not None:
        got = payload_of(bufs["labels"], 8 * len(exp["labels"]), what).view(np.uint64)
        assert (got == exp["labels"]).all(), (what, got.tolist(), exp["labels"].tolist())        # uncapped too
    if bufs["rows"] is not None:
        got = payload_of(bufs["rows"], 8 * (n + 1), what).view(np.uint64)
        bad = np.flatnonzero(got != exp["rows"])
        assert bad.size == 0, (what, "rows differ first at %d" % (bad[0] if bad.size else -1))
    if bufs["owners"] is not None:
        assert (payload_of(bufs["owners"], 8 * k, what).view(np.uint64) == exp["owners"][:k]).all(), what
    if bufs["spans"] is not None:
        got = payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2)
        bad = np.flatnonzero((got != exp["spans"][:k]).any(axis=1))
        assert bad.size == 0, (what, "%d spans of %d differ, first: entry %d %s expected %s" % (
            bad.size, k, bad[0] if bad.size else -1, got[bad[0]].tolist() if bad.size else "", exp["spans"][bad[0]].tolist() if bad.size else ""))
    if bufs["masks"] is not None:
        got = payload_of(bufs["masks"], 8 * k, what).view(np.uint64)
        bad = np.flatnonzero(got != exp["masks"][:k])
        assert bad.size == 0, (what, "%d masks of %d differ, first: entry %d: %x expected %x" % (
            bad.size, k, bad[0] if bad.size else -1, got[bad[0]] if bad.size else 0, exp["masks"][bad[0]] if bad.size else 0))


def both(torch, name, strings, opts, what="", batch=None, devices=(True, False)):
    """room for every entry, device and host pointers: checked against the model"""
    batch = batch or Batch(torch, strings)
    exp = lists_of(name, model(name, strings, opts), batch.offs)
    for device in devices:
        check_lex(lex_call(torch, name, batch, opts, exp["count"] + 3, device), exp, exp["count"] + 3, (name, opts, device, what))
    return exp


# ---- GPU: every set against the model -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", RUN)
def test_every_set_against_the_model(torch_cuda, name):
    torch = torch_cuda
    own = SETS[name]["opts"]
    modes = [own, own | T] + ([own | S, own | S | T] if name in ("lexer3", "kw") else [])
    whole = Batch(torch, PROBES)
    for opts in modes:
        exp = both(torch, name, PROBES, opts, "all probes", whole)
        assert exp["count"] >= 4
        per = model(name, PROBES, opts)
        for i, probe in enumerate(PROBES):                      # n = 1: every probe alone, inside the batch's buffer
            one = lists_of(name, [per[i]], whole.offs[i:i + 2])
            one_offs = whole.offs[i:i + 2].copy()
            bufs = lex_call(torch, name, whole, opts, one["count"] + 1, True, n=1, offs=one_offs)
            check_lex(bufs, one, one["count"] + 1, (name, opts, probe))
        for probe in PROBES[::5]:                               # ... and through host pointers
            both(torch, name, [probe], opts, probe, devices=(False,))


# ---- GPU: alignment ----------------------------------------------------------------------------------------------------------------

@gpu
def test_every_length_at_every_address_mod_16(torch_cuda):
    """one lexer3 string of 0..48 bytes at each address mod 16, random bytes around it (strings of their own: checked as well)"""
    torch = torch_cuda
    rng = np.random.RandomState(31)
    alphabet = u8(b"ab1 ?\t9z")
    strings, pos, starts = [], 0, set()
    for L in range(49):
        for mod in range(16):
            fill = (mod - pos) % 16
            strings.append(bytes(rng.choice(alphabet, size=fill)))
            pos += fill
            starts.add((L, pos % 16))
            strings.append(bytes(rng.choice(alphabet, size=L)))
            pos += L
    assert len(starts) == 49 * 16
    batch = Batch(torch, strings, lead=b"a1" * 8, trail=b"1a" * 24)
    for opts in (0, T, S, T | S):
        exp = both(torch, "lexer3", strings, opts, "alignment", batch)
        assert exp["count"] > 2000
    crossing = sum(1 for es, s in zip(model("lexer3", strings, T), strings) for b, e, k in es if k == 0 and e - b > 1)
    assert crossing > 100                                       # gap runs of several bytes, many across a 16-byte boundary
    # n = 1 at every residue: the string alone in the call, its neighbours' bytes around it
    per = {opts: model("lexer3", strings, opts) for opts in (0, T)}
    for i in range(1, len(strings), 2):
        if len(strings[i]) in (0, 1, 15, 16, 17, 33, 48):
            for opts in (0, T):
                one = lists_of("lexer3", [per[opts][i]], batch.offs[i:i + 2])
                bufs = lex_call(torch, "lexer3", batch, opts, one["count"] + 1, True, n=1, offs=batch.offs[i:i + 2].copy())
                check_lex(bufs, one, one["count"] + 1, ("alone", opts, i))


# ---- GPU: the CSR scan ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", (1023, 1024, 1025, 2049))
def test_tile_and_tile_sum_scan(torch_cuda, n):
    """short strings, every 7th empty, one pair of offsets that decreases (string 0: empty by the rule, nothing overlaps)"""
    torch = torch_cuda
    strings = H.random_strings(np.random.RandomState(n), n, 24, b"ab19 ?")
    for i in range(0, n, 7):
        strings[i] = b""
    batch = Batch(torch, strings)
    offs = batch.offs.copy()
    offs[0] = 37                                                # offsets[1] = 0 < offsets[0]: string 0 is empty
    for opts in (0, T):
        exp = lists_of("lexer3", model("lexer3", strings, opts), batch.offs)
        assert exp["count"] > 3 * n
        check_lex(lex_call(torch, "lexer3", batch, opts, exp["count"], True, offs=offs), exp, exp["count"], (n, opts, "decreasing"))
        check_lex(lex_call(torch, "lexer3", batch, opts, exp["count"], False), exp, exp["count"], (n, opts, "host"))


# ---- GPU: capacity -------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,opts", (("lexer3", T), ("kw", 0)))
def test_capacity_below_at_and_above_the_count(torch_cuda, name, opts):
    torch = torch_cuda
    strings = [b"if a1 ?? while9"] + H.random_strings(np.random.RandomState(13), 300, 40, b"ifelswh 19?") + [b"else if x 12 ??"]
    batch = Batch(torch, strings, lead=b"a" * 21, trail=b"1" * 40)
    entries = model(name, strings, opts)
    assert len(entries[0]) >= 2 and len(entries[-1]) >= 2       # the cuts at 1 and at count - 1 fall inside a string's row
    exp = lists_of(name, entries, batch.offs)
    count = exp["count"]
    assert count > 600
    for device in (True, False):
        for cap in (0, 1, count - 1, count, count + 1):
            for drop in (None, "owners", "spans", "masks"):
                want = tuple(k for k in LISTS if k != drop)
                check_lex(lex_call(torch, name, batch, opts, cap, device, want), exp, cap, (name, device, cap, drop))
        check_lex(lex_call(torch, name, batch, opts, 0, device, ("labels",)), exp, 0, (name, device, "count and label counts alone"))
        check_lex(lex_call(torch, name, batch, opts, 0, device, ()), exp, 0, (name, device, "the count alone"))
        check_lex(lex_call(torch, name, batch, opts, 5, device, ("masks",)), exp, 5, (name, device, "masks alone"))
    # n == 0 on the device: the counts (and rows[0]) zeroed on the stream
    bufs = lex_call(torch, name, batch, opts, 4, True, n=0)
    assert payload_of(bufs["count"], 8).view(np.uint64)[0] == 0 and payload_of(bufs["rows"], 8).view(np.uint64)[0] == 0
    assert (payload_of(bufs["labels"], 8 * len(exp["labels"])).view(np.uint64) == 0).all()
    payload_of(bufs["owners"], 0), payload_of(bufs["spans"], 0), payload_of(bufs["masks"], 0)


# ---- GPU: gaps ------------------------------------------------------------------------------------------------------------------------

@gpu
def test_gaps(torch_cuda):
    torch = torch_cuda
    strings = [b"????????????????????", b"?", b"??ab12??", b"?a", b"a?", b"a?" * 32, b"", b"7" * 4096, b"a1" * 2048, b"?" * 100 + b"x"]
    tokens = model("lexer3", strings, T)
    assert tokens[0] == [(0, 20, 0)] and tokens[2] == [(0, 2, 0), (2, 4, 1), (4, 6, 2), (6, 8, 0)]
    assert len(tokens[5]) == 64 and [k for _, _, k in tokens[5]] == [1, 0] * 32
    assert tokens[7] == [(0, 4096, 2)] and len(tokens[8]) == 4096 and [k for _, _, k in tokens[8][:4]] == [1, 2, 1, 2]
    for opts in (T, 0, T | S):
        exp = both(torch, "lexer3", strings, opts, "gaps")
    assert lists_of("lexer3", tokens, H.pack(strings)[1])["labels"].tolist()[3] == 1 + 1 + 2 + 1 + 1 + 32 + 1


# ---- GPU: labels outside the dense rows, bit 63, the EndMark, the label counts --------------------------------------------------------

@gpu
def test_labels_outside_the_dense_rows(torch_cuda):
    torch = torch_cuda
    rng = np.random.RandomState(23)
    strings = []
    for i in range(500):
        parts = []
        for _ in range(int(rng.randint(0, 5))):
            parts.append(bytes(rng.choice(u8(b"abcdefghijxyz "), size=int(rng.randint(0, 12)))))
            w = WORDS[int(rng.randint(len(WORDS)))]
            parts.append(w if rng.rand() < 0.7 else w[:-1])
        strings.append(b"".join(parts))
    for opts in (0, T):
        exp = both(torch, "words2", strings, opts, "words2")
        assert exp["labels"][0] > 100 and exp["labels"][1] > 100 and set(exp["masks"].tolist()) <= {0, 1, 2}


@gpu
def test_bit_63_the_end_mark_and_the_label_counts(torch_cuda):
    torch = torch_cuda
    rng = np.random.RandomState(3)
    keys = [b"k%02d" % i for i in range(64)]
    strings = [b" ".join(keys[int(j)] for j in rng.randint(0, 64, size=int(rng.randint(0, 9)))) for _ in range(300)] + [b"k63", b"k00k63", b"k6"]
    for opts in (0, T):
        exp = both(torch, "r64", strings, opts, "r64")
        assert exp["labels"][0] > 5 and exp["labels"][63] > 5 and int(exp["masks"].max()) == 1 << 63
    # the EndMark rule: only the entry that ends the string gets the `$` regexp's bit
    ends = [b"ab", b"ab cd", b"ab ", b"ab c", b"abc d", b"x", b"12 ab", b"ab 12"] + H.random_strings(rng, 300, 20, b"abc 12")
    tok = model("ends", ends, E | T)
    assert tok[0] == [(0, 2, 3)] and tok[1] == [(0, 2, 1), (2, 3, 0), (3, 5, 3)] and tok[3] == [(0, 2, 1), (2, 3, 0), (3, 4, 3)]
    assert tok[2] == [(0, 2, 1), (2, 3, 0)]                     # one byte before the end: no bit 1
    for name in ("ends", "eol"):
        for opts in (E, E | T, T, E | T | S):
            both(torch, name, ends, opts, name)
    # label counts: a Counter over the model's LOWEST bits, where lowest is not only
    pieces = (b"if", b"else", b"while", b"iffy", b"x9", b" ", b" ", b" ", b"?", b"10")
    kw = [b"if iffy 10 else x9", b"while(x) else9 elsewhere"] + [b"".join(pieces[int(j)] for j in rng.randint(0, 10, size=12)) for _ in range(300)]
    for opts in (0, T):
        exp = both(torch, "kw", kw, opts, "kw")
        assert (exp["masks"] == 3).sum() > 20 and exp["labels"][0] == (exp["masks"] == 3).sum() and exp["labels"][1] == (exp["masks"] == 2).sum()
    for opts in (B, B | T, T):
        both(torch, "bol", [b"#ab #c", b"x#", b"#", b"##"] + H.random_strings(rng, 200, 12, b"#ab "), opts, "bol")
    ips = [b"from 10.0.0.1:80 x 10.0.0", b"1.2.3.4", b"1234.5.6.7.8 9.9.9.9"] + H.random_strings(rng, 200, 60, b"0123456789. x")
    for opts in (0, T):                                         # (token mode: strings of at most 256 bytes for this set)
        both(torch, "ipnum", ips, opts, "ipnum")
    both(torch, "alt3", H.random_strings(rng, 300, 30, b"abc "), 0, "alt3")
    both(torch, "alt3", H.random_strings(rng, 300, 30, b"abc "), T, "alt3")


# ---- GPU: the lines form ---------------------------------------------------------------------------------------------------------------

def lines_call(torch, name, raw, delim, opts, cap, device, gather=None, lists=True, rev=True):
    """gather: None -- spans only --, or (tail_byte, text_cap)"""
    tr, tf = tables_of(name)
    R = SETS[name]["regexps"]
    keep = torch.as_tensor(raw, device="cuda") if device else raw
    tail_byte, text_cap = gather if gather else (0, 0)
    bufs = {"lines": guarded(torch, 8, device), "count": guarded(torch, 8, device), "labels": guarded(torch, 8 * (R + 1), device),
            "owners": guarded(torch, 8 * cap, device) if lists else None, "spans": guarded(torch, 16 * cap, device),
            "masks": guarded(torch, 8 * cap, device) if lists else None,
            "text": guarded(torch, text_cap, device) if gather else None, "offsets": guarded(torch, 8 * (cap + 1), device) if gather else None,
            "bytes": guarded(torch, 8, device) if gather else None}
    p = {k: (ptr_of(v) if v is not None else None) for k, v in bufs.items()}
    rc = pb.lib().pire_hip_lex_lines_gather(tr._h if rev else None, tf._h, opts, keep.data_ptr() if device else keep.ctypes.data, len(raw), delim,
                                            pb.FLAG_ON_DEVICE if device else 0, tail_byte, p["lines"], p["owners"], p["spans"], p["masks"], cap,
                                            p["count"], p["labels"], p["text"], text_cap, p["offsets"], p["bytes"],
                                            stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    if device:
        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
    return bufs


@gpu
@pytest.mark.parametrize("delim", (10, 0))
def test_lines_in_labelled_entries_out(torch_cuda, delim):
    torch = torch_cuda
    rng = np.random.RandomState(29)
    lines = H.random_strings(rng, 200, 40, b"ifelswh x19?")
    for i in range(0, 200, 9):
        lines[i] = b""
    lines[-1] = b"while x9"                                     # the last line has no delimiter behind it
    d = bytes([delim])
    raw = u8(d.join(lines)).copy()
    parts = TS.py_lines(raw, d)
    assert len(parts) == 200 and parts == lines
    for opts in (0, T):
        entries = model("kw", parts, opts)
        exp = lists_of("kw", entries, H.pack(parts)[1], shift=1)
        texts = [parts[i][b:e] for i, es in enumerate(entries) for b, e, _ in es]
        assert all(bytes(raw[b:e]) == t for (b, e), t in zip(exp["spans"].tolist(), texts)) and exp["count"] > 400
        for device in (True, False):
            for cap in (exp["count"] + 7, exp["count"] - 1):
                k = min(cap, exp["count"])
                what = (delim, opts, device, cap)
                for gather, listed in ((None, True), ((delim, len(raw) + cap), True), ((delim, len(raw) + cap), False), ((NO_TAIL, len(raw)), True)):
                    bufs = lines_call(torch, "kw", raw, delim, opts, cap, device, gather, listed, rev=not (opts & T and device))
                    assert payload_of(bufs["lines"], 8, what).view(np.uint64)[0] == 200
                    assert payload_of(bufs["count"], 8, what).view(np.uint64)[0] == exp["count"]
                    assert (payload_of(bufs["labels"], 24, what).view(np.uint64) == exp["labels"]).all(), what
                    assert (payload_of(bufs["spans"], 16 * k, what).view(np.uint64).reshape(-1, 2) == exp["spans"][:k]).all(), what
                    if listed:
                        assert (payload_of(bufs["owners"], 8 * k, what).view(np.uint64) == exp["owners"][:k]).all(), what
                        assert (payload_of(bufs["masks"], 8 * k, what).view(np.uint64) == exp["masks"][:k]).all(), what
                    if gather:
                        tail = b"" if gather[0] == NO_TAIL else d
                        want = b"".join(t + tail for t in texts[:k])
                        assert payload_of(bufs["bytes"], 8, what).view(np.uint64)[0] == len(want), what
                        assert payload_of(bufs["text"], len(want), what).tobytes() == want, what
                        ends = np.cumsum([0] + [len(t) + len(tail) for t in texts[:k]]).astype(np.uint64)
                        assert (payload_of(bufs["offsets"], 8 * (k + 1), what).view(np.uint64) == ends).all(), what
                        if opts & T and gather[0] == NO_TAIL and cap > exp["count"]:      # token mode: the line itself, cut
                            assert want == b"".join(parts)
    g = pb.lex_lines_gather_host(*tables_of("kw"), raw, opts=T, delim=delim, tail_byte=None)
    exp = lists_of("kw", model("kw", parts, T), H.pack(parts)[1], shift=1)
    assert g["lines"] == 200 and g["count"] == exp["count"] and (g["masks"] == exp["masks"]).all() and (g["spans"] == exp["spans"]).all()
    assert g["text"].tobytes() == b"".join(parts) and (g["label_counts"] == exp["labels"]).all()
    assert pb.lex_labels(g["masks"]).tolist() == [lowest(int(k)) if k else pb.LEX_GAP for k in exp["masks"].tolist()]


# ---- GPU: determinism -------------------------------------------------------------------------------------------------------------------

@gpu
def test_the_same_input_gives_the_same_bits(torch_cuda):
    torch = torch_cuda
    strings = TS.mixed_strings(9, 900) + [b"if a1 ?? while9"] * 40
    batch = Batch(torch, strings)
    text, offs = H.pack(strings)
    for name, opts in (("lexer3", 0), ("lexer3", T), ("kw", T | S)):
        exp = lists_of(name, model(name, strings, opts), batch.offs)
        cap = exp["count"] + 2
        runs = [lex_call(torch, name, batch, opts, cap), lex_call(torch, name, batch, opts, cap)]
        if opts & T:
            runs.append(lex_call(torch, name, batch, opts, cap, rev=False))             # token mode does not read rev
        sizes = (("rows", 8 * (batch.n + 1)), ("owners", 8 * exp["count"]), ("spans", 16 * exp["count"]), ("masks", 8 * exp["count"]),
                 ("labels", 8 * len(exp["labels"])), ("count", 8))
        for other in runs[1:]:
            for key, size in sizes:
                assert payload_of(runs[0][key], size).tobytes() == payload_of(other[key], size).tobytes(), (name, opts, key)
        check_lex(runs[0], exp, cap, (name, opts))
        tr, tf = tables_of(name)
        host = pb.lex(None if opts & T else tr, tf, text, offs, opts)
        assert host["count"] == exp["count"] and (host["rows"] == exp["rows"]).all() and (host["masks"] == exp["masks"]).all()
        assert (host["label_counts"] == exp["labels"]).all() and host["spans"].tobytes() == payload_of(runs[0]["spans"], 16 * exp["count"]).tobytes()
    assert pb.last_kernel() != "lex"
