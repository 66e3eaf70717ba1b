"""pire_hip_affix_select, pire_hip_affix_run_select and pire_hip_affix_lines_gather: from the lengths of pire_hip_prefix and
pire_hip_suffix to the strings (lines) that matched and the byte range of the matched head, the matched tail or what they
leave -- on the device (affix.hip).

Exact equality everywhere.  The expected values come from `model_affix_select` -- the formulas of include/pire_hip.h written
down with numpy, held against a hand-written truth table below --, applied, where a scan is involved, to what the C oracle's
LongestPrefix / ShortestPrefix / LongestSuffix / ShortestSuffix say (held against the unmodified reference where that is
built), and for lines to Python's own split and slices.  Nothing expected comes from the library.  Every output of a call sits
between poisoned guard bytes and is compared bytewise, what the call had no business writing included.

The scanners are tests/golden/affix/* (tests/golden/make_affix_inputs.py wrote them through the reference): small, not
Surround()ed, each in a forward form and a form compiled from Fsm::Reverse().  The batches are constructed, so that a known
share of the strings has a matching head, a matching tail, or is nothing but a head (where head and tail overlap)."""
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
AFFIX = os.path.join(H.GOLDEN, "affix")
POISON = 0xA5
GUARD = 64                     # poisoned bytes around every output
EINVAL = -1
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
HEAD, TAIL, REST = pb.AFFIX_HEAD, pb.AFFIX_TAIL, pb.AFFIX_REST
PARTS = (HEAD, TAIL, REST)
LONGEST, T_BEGIN, T_END = pb.AFFIX_LONGEST, pb.AFFIX_THROUGH_BEGIN, pb.AFFIX_THROUGH_END
gpu = pytest.mark.gpu
NAMES = ("pire_hip_affix_select", "pire_hip_affix_run_select", "pire_hip_affix_lines_gather")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_affix_select(offsets, head_len, tail_len, part, shift=0):
    """include/pire_hip.h, line by line; every hit, ascending, their spans and their number.  shift: string i lies shift * i
    bytes further into the buffer the spans are counted in (the lines form: 1)."""
    offs = np.asarray(offsets, dtype=np.uint64)
    n = len(offs) - 1
    o0, o1 = offs[:-1], offs[1:]
    ln = np.where(o1 >= o0, o1 - o0, np.uint64(0)).astype(np.uint64)
    sel = np.ones(n, dtype=bool)
    zero = np.zeros(n, dtype=np.uint64)

    def clamp(a, room):            # min(a, room) for the a that are >= 0 (the others are not selected: whatever)
        a = np.asarray(a, dtype=np.int64)
        return np.minimum(np.where(a >= 0, a, 0).astype(np.uint64), room)

    if head_len is not None:
        sel &= np.asarray(head_len, dtype=np.int64) >= 0
    if tail_len is not None:
        sel &= np.asarray(tail_len, dtype=np.int64) >= 0
    h = clamp(head_len, ln) if head_len is not None else zero
    t = clamp(tail_len, ln) if tail_len is not None else zero
    r = clamp(tail_len, ln - h) if tail_len is not None else zero
    base = o0 + np.uint64(shift) * np.arange(n, dtype=np.uint64)
    if part == HEAD:
        assert head_len is not None
        b, e = base, base + h
    elif part == TAIL:
        assert tail_len is not None
        b, e = base + ln - t, base + ln
    else:
        assert part == REST and (head_len is not None or tail_len is not None or n == 0)
        b, e = base + h, base + ln - r
    hits = np.flatnonzero(sel).astype(np.uint64)
    spans = np.stack([b[sel], e[sel]], axis=1).astype(np.uint64).reshape(-1, 2)
    return {"hits": hits, "spans": spans, "count": int(hits.size)}


def py_lines(raw, delim=b"\n"):
    """getline: the runs between delimiters; no extra empty line behind a trailing delimiter.  (lines, begin of every line in raw)"""
    parts = bytes(raw).split(delim)
    if parts and parts[-1] == b"":
        parts.pop()
    begins, pos = [], 0
    for s in parts:
        begins.append(pos)
        pos += len(s) + 1
    return parts, np.array(begins, dtype=np.uint64)


# rows of the truth table: string i is [OFFS[i], OFFS[i + 1]) -- the seventh has offsets that decrease (an empty string)
T_OFFS = [100, 110, 120, 128, 140, 150, 150, 145, 160, 170, 175]
T_HEAD = [3, 0, -1, 12, 7, I64_MAX, 2, I64_MIN, I64_MAX, 10]          # 12 = len, 10 = len + 5, 7 + 6 > 10
T_TAIL = [4, 0, 2, 17, 6, 0, 3, I64_MAX, I64_MAX, -1]                 # 17 = len + 5
TRUTH = {
    "both": ([0, 1, 3, 4, 5, 6, 8], {
        HEAD: [[100, 103], [110, 110], [128, 140], [140, 147], [150, 150], [150, 150], [160, 170]],
        TAIL: [[106, 110], [120, 120], [128, 140], [144, 150], [150, 150], [150, 150], [160, 170]],
        REST: [[103, 106], [110, 120], [140, 140], [147, 147], [150, 150], [150, 150], [170, 170]]}),
    "head": ([0, 1, 3, 4, 5, 6, 8, 9], {
        HEAD: [[100, 103], [110, 110], [128, 140], [140, 147], [150, 150], [150, 150], [160, 170], [170, 175]],
        REST: [[103, 110], [110, 120], [140, 140], [147, 150], [150, 150], [150, 150], [170, 170], [175, 175]]}),
    "tail": ([0, 1, 2, 3, 4, 5, 6, 7, 8], {
        TAIL: [[106, 110], [120, 120], [126, 128], [128, 140], [144, 150], [150, 150], [150, 150], [145, 160], [160, 170]],
        REST: [[100, 106], [110, 120], [120, 126], [128, 128], [140, 144], [150, 150], [150, 150], [145, 145], [160, 160]]}),
}


def given(which, head, tail):
    return (head if which in ("both", "head") else None, tail if which in ("both", "tail") else None)


def test_the_model_against_a_hand_written_truth_table():
    for which, (hits, spans) in TRUTH.items():
        h, t = given(which, T_HEAD, T_TAIL)
        for part, want in spans.items():
            got = model_affix_select(T_OFFS, h, t, part)
            assert got["hits"].tolist() == hits and got["count"] == len(hits), (which, part)
            assert got["spans"].tolist() == want, (which, part, got["spans"].tolist())
            lo, hi = np.array(T_OFFS)[hits], np.array(T_OFFS)[np.array(hits) + 1]
            s = got["spans"].astype(np.int64)
            assert ((s[:, 0] <= s[:, 1]) & (lo <= s[:, 0]) & (s[:, 1] <= np.maximum(lo, hi))).all()       # never outside the string
    assert model_affix_select([5], None, None, REST)["count"] == 0
    # shift: string i lies i bytes further on
    got = model_affix_select([0, 3, 5], [1, 1], None, REST, shift=1)
    assert got["spans"].tolist() == [[1, 3], [5, 6]]
    assert py_lines(b"a\n\nbc\n")[0] == [b"a", b"", b"bc"] and py_lines(b"a\n\nbc")[1].tolist() == [0, 2, 3]
    assert py_lines(b"")[0] == [] and py_lines(b"\n")[0] == [b""] and py_lines(b"x|y|", b"|")[0] == [b"x", b"y"]


# ---- the scanners, their batches and what the oracle says (shared; the oracle runs once per pair and option set) ---------------
with open(os.path.join(AFFIX, "cases.json")) as _f:
    CASES = json.load(_f)
BLANK = [b" ", b"\t\t", b"  \t "]
# name -> ((head scanner, form) or None, (tail scanner, form) or None, the alphabet of the bodies -- no byte of it starts or ends
# a match --, heads, tails, strings that are a head alone, options of the head scan, of the tail scan)
PAIRS = {
    "trim": (("blanks", "n"), ("blanks", "nr"), b"abcxyz", BLANK, BLANK, [b"   ", b"\t"], LONGEST, LONGEST),
    "star_trim": (("blanks_star", "n"), ("blanks", "nr"), b"abcxyz", BLANK, BLANK, [b"   ", b"\t"], LONGEST, LONGEST),
    "stamp_blank": (("stamp", "n"), ("blanks", "nr"), b"abcxyz:", [b"2024-01-02 ", b"1999-12-31 "], BLANK, [b"2024-01-02 "], LONGEST, LONGEST),
    "arrows": (("arrow", "n"), ("arrow", "nr"), b"abc ", [b"-->"], [b"-->"], [b"-->"], LONGEST, LONGEST),
    "exts": (("ext", "n"), ("ext", "nr"), b"abc/_ABC", [b".gz", b".log", b".txt"], [b".gz", b".log", b".txt"], [b".log", b".gz"], LONGEST, LONGEST),
    "alts": (("alt", "n"), ("alt", "nr"), b"xyz ", [b"abc", b"abcabc", b"bbbb", b"b"], [b"abc", b"abcabc", b"bbbb", b"b"], [b"abcabc", b"bbb"],
             LONGEST, LONGEST),
    "marked": (("marked_blanks", "n"), ("marked_blanks", "nr"), b"abcxyz", BLANK, BLANK, [b"   ", b"\t"], LONGEST | T_BEGIN, LONGEST | T_END),
    "same_table": (("blanks", "n"), ("blanks", "n"), b"abcxyz", BLANK, BLANK, [b"   ", b"\t"], LONGEST, LONGEST),
}
ref_built = ob.ref_available()
_blobs, _batches, _lengths = {}, {}, {}


def blob_of(scanner):
    if scanner not in _blobs:
        case = [c for c in CASES["scanners"] if (c["name"], c["form"]) == tuple(scanner)][0]
        _blobs[scanner] = H.load_blob(os.path.join("affix", case["blob"]))
    return _blobs[scanner]


def batch(pair):
    """3 000 strings: a random body; a matching head in front of every string with i % 3 == 0; a matching tail behind every string
    with i % 3 != 2; every fifteenth is a head alone; and b"" """
    if pair not in _batches:
        _, _, alphabet, heads, tails, alone, _, _ = PAIRS[pair]
        bodies = H.random_strings(np.random.RandomState(17), 3000, 120, alphabet)
        out = []
        for i, s in enumerate(bodies):
            if i % 15 == 0:
                out.append(alone[(i // 15) % len(alone)])
            else:
                out.append((heads[i % len(heads)] if i % 3 == 0 else b"") + s + (tails[i % len(tails)] if i % 3 != 2 else b""))
        _batches[pair] = out + [b""]
    return _batches[pair]


def opts_args(opts):
    """(longest, through_begin, through_end) of one scan's option bits"""
    return bool(opts & LONGEST), bool(opts & T_BEGIN), bool(opts & T_END)


def oracle_lengths(pair, head_opts=None, tail_opts=None, strings=None, only=None):
    """(head_len or None, tail_len or None) of the batch (or of `strings`) from the C oracle -- and from the reference where it is
    built: the same numbers.  only: "head" / "tail" -- the other table is not given."""
    hs, ts = PAIRS[pair][0], PAIRS[pair][1]
    head_opts = PAIRS[pair][6] if head_opts is None else head_opts
    tail_opts = PAIRS[pair][7] if tail_opts is None else tail_opts
    key = (pair, head_opts, tail_opts, only)
    if strings is None and key in _lengths:
        return _lengths[key]
    text, offs = H.pack(batch(pair) if strings is None else strings)
    hl = tl = None
    if only != "tail":
        lo, tb, te = opts_args(head_opts)
        hl = ob.OracleScanner(blob_of(hs)).prefix(text, offs, lo, tb, te)
        if ref_built and len(offs) > 1:
            assert (ob.RefScanner.load(blob_of(hs)).prefix(text, offs, lo, tb, te) == hl).all(), (pair, "prefix")
    if only != "head":
        lo, tb, te = opts_args(tail_opts)
        tl = ob.OracleScanner(blob_of(ts)).suffix(text, offs, lo, te, tb)
        if ref_built and len(offs) > 1:
            assert (ob.RefScanner.load(blob_of(ts)).suffix(text, offs, lo, te, tb) == tl).all(), (pair, "suffix")
    if strings is None:
        for a in (hl, tl):
            if a is not None:
                a.setflags(write=False)
        _lengths[key] = (hl, tl)
    return hl, tl


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
    for macro, value in (("HEAD", HEAD), ("TAIL", TAIL), ("REST", REST), ("LONGEST", LONGEST), ("THROUGH_BEGIN", T_BEGIN), ("THROUGH_END", T_END)):
        assert int(re.search(r"#define PIRE_HIP_AFFIX_%s (\d+)u" % macro, src).group(1)) == value, macro
    # the formulas the model is written from stand in the header
    for line in ("selected(i) = (head_len == NULL || head_len[i] >= 0) && (tail_len == NULL || tail_len[i] >= 0)",
                 "r_i         = tail_len ? min(tail_len[i], len_i - h_i) : 0"):
        assert line in src, line
    assert "affix" not in ",".join(pb.selftested_kernels())


def test_the_fixtures_are_what_their_generator_says():
    names = {c["name"] for c in CASES["scanners"]}
    assert {"blanks", "blanks_star", "stamp", "arrow", "ext", "alt"} <= names
    probes = [bytes.fromhex(h) for h in CASES["probes_hex"]]
    text, offs = H.pack(probes)
    for c in CASES["scanners"]:
        assert c["options"] == c["form"] and c["form"] in ("n", "nr")
        blob = blob_of((c["name"], c["form"]))
        assert len(blob) < 8192 and os.path.getsize(os.path.join(AFFIX, c["blob"])) == len(blob)
        o = ob.OracleScanner(blob)
        walk = o.prefix if c["form"] == "n" else o.suffix
        assert walk(text, offs, True, c["marks"], False).tolist() == c["longest"], c["name"]      # the oracle against the reference's record
        assert walk(text, offs, False, c["marks"], False).tolist() == c["shortest"], c["name"]
    star = [c for c in CASES["scanners"] if c["name"] == "blanks_star"]
    assert all(min(c["shortest"]) == 0 for c in star)                                           # accepts the empty string


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_every_batch_of_the_gpu_part_selects_a_known_share_and_overlaps(pair):
    """On the oracle's own numbers: between 1/4 and 3/4 of the strings are selected, and in at least 1/20 of the selected ones the
    head and the tail overlap (head_len + tail_len > len) -- no list of the GPU part can be right by being empty or full, and the
    tail-gives-way rule of REST is exercised.  Under the pair's own options; the other option sets of the GPU part are held against
    the oracle all the same."""
    strings = batch(pair)
    assert len(strings) == 3001 and strings[-1] == b"" and not any(b"\n" in s or b"|" in s for s in strings)
    hl, tl = oracle_lengths(pair)
    lens = np.array([len(s) for s in strings])
    sel = (hl >= 0) & (tl >= 0)
    share = sel.mean()
    assert 0.25 <= share <= 0.75, (pair, share)
    over = (hl[sel] + tl[sel] > lens[sel]).mean()
    assert over >= 0.05, (pair, over)
    assert (hl == 0).any() or (tl == 0).any() or pair != "star_trim"                            # a length of 0 that is a match
    exp = model_affix_select(H.pack(strings)[1], hl, tl, REST)
    assert exp["count"] == int(sel.sum())
    # the lines forms' buffers are cut from the same strings
    lines = lines_of(pair)
    lh, lt = oracle_lengths(pair, strings=lines)
    lsel = (lh >= 0) & (lt >= 0)
    assert 0.25 <= lsel.mean() <= 0.75 and lines.count(b"") >= 3 and lsel[-1] and lh[-1] == len(lines[-1])


def lines_of(pair):
    """~2 000 lines of the batch: three empty lines in a row, and a last line that is only a head"""
    strings = batch(pair)
    return strings[:100] + [b""] * 3 + strings[100:2000] + [PAIRS[pair][5][0]]


def _guarded(cap=4):
    return {"hits": np.full(8 * (cap + 2), POISON, dtype=np.uint8), "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8),
            "lens": np.full(64, POISON, dtype=np.uint8), "text": np.full(64, POISON, dtype=np.uint8),
            "offsets": np.full(8 * (cap + 3), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


# what pire_hip_affix_select refuses of (offsets, n, part, head_len, tail_len, out_hits, out_spans, hit_cap, out_hit_count): the
# message, and the arguments as a function of the valid ones
PASS_REFUSALS = {
    "unknown part": lambda o, a, b, h, s, c: (o, 3, 3, a, b, h, s, 4, c),
    "unknown part ": lambda o, a, b, h, s, c: (o, 3, 0x80000000, a, b, h, s, 4, c),
    "n > 0 with null head_len and null tail_len": lambda o, a, b, h, s, c: (o, 3, REST, None, None, h, s, 4, c),
    "PIRE_HIP_AFFIX_HEAD without head_len": lambda o, a, b, h, s, c: (o, 3, HEAD, None, b, h, s, 4, c),
    "PIRE_HIP_AFFIX_TAIL without tail_len": lambda o, a, b, h, s, c: (o, 3, TAIL, a, None, h, s, 4, c),
    "n > 0 with null offsets": lambda o, a, b, h, s, c: (None, 3, REST, a, b, h, s, 4, c),
    "null out_hit_count": lambda o, a, b, h, s, c: (o, 3, HEAD, a, b, h, s, 4, None),
    "hit_cap > 0 with null out_hits and null out_spans": lambda o, a, b, h, s, c: (o, 3, TAIL, a, b, None, None, 4, c),
    "2^32 strings or more": lambda o, a, b, h, s, c: (o, 1 << 32, REST, a, b, h, s, 4, c),
}


def test_affix_select_refuses_before_any_device_is_touched():
    L = pb.lib()
    offs = np.array([0, 4, 4, 9], dtype=np.uint64)
    head, tail = np.array([1, 0, -1], dtype=np.int64), np.array([2, -1, 0], dtype=np.int64)
    bufs, cnt = _guarded(), C.c_uint64(77)
    for what, args in PASS_REFUSALS.items():
        a = args(offs.ctypes.data, head.ctypes.data, tail.ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt))
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_affix_select(a[0], a[1], a[2], flags, *a[3:], None) == EINVAL, what
            msg = L.pire_hip_last_error().decode()
            assert what.strip() in msg and msg.startswith("pire_hip_affix_select: "), (what, msg)
    assert cnt.value == 77 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="PIRE_HIP_AFFIX_TAIL without tail_len"):   # (the wrappers raise what the library refuses)
        pb.affix_select_host(offs, head_len=head, part=TAIL)
    with pytest.raises(pb.PireHipError, match="null out_hits and null out_spans"):
        pb.affix_select_device(offs.ctypes.data, 3, C.addressof(cnt), head_len_ptr=head.ctypes.data, hit_cap=3)


def test_affix_run_select_refuses_before_any_device_is_touched():
    """what the pass refuses -- a table standing for its length array --, what the scans refuse, and the options"""
    L = pb.lib()
    text, offs = H.pack([b"  ab ", b"", b"b  "])
    text, offs = text.copy(), offs.copy()
    th, tt = pb.Table(blob_of(("blanks", "n"))), pb.Table(blob_of(("blanks", "nr")))
    bufs, cnt = _guarded(), C.c_uint64(77)
    x, o, h, s, c = text.ctypes.data, offs.ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    # (head, head_opts, tail, tail_opts, offsets, n, part, out_hits, out_spans, hit_cap, out_hit_count)
    cases = {
        "null head and null tail": (None, 1, None, 1, o, 3, REST, h, s, 4, c),
        "unknown bits in head_opts": (th._h, 8, tt._h, 1, o, 3, REST, h, s, 4, c),
        "unknown bits in tail_opts": (th._h, 1, tt._h, 0x10, o, 3, REST, h, s, 4, c),
        "unknown part": (th._h, 1, tt._h, 1, o, 3, 3, h, s, 4, c),
        "PIRE_HIP_AFFIX_HEAD without head_len": (None, 1, tt._h, 1, o, 3, HEAD, h, s, 4, c),
        "PIRE_HIP_AFFIX_TAIL without tail_len": (th._h, 1, None, 1, o, 3, TAIL, h, s, 4, c),
        "n > 0 with null offsets": (th._h, 1, tt._h, 1, None, 3, REST, h, s, 4, c),
        "null out_hit_count": (th._h, 1, tt._h, 1, o, 3, REST, h, s, 4, None),
        "hit_cap > 0 with null out_hits and null out_spans": (th._h, 1, th._h, 1, o, 3, REST, None, None, 4, c),
        "2^32 strings or more": (th._h, 1, tt._h, 1, o, 1 << 32, REST, h, s, 4, c),
    }
    lens = bufs["lens"].ctypes.data
    for what, a in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            rc = L.pire_hip_affix_run_select(a[0], a[1], a[2], a[3], x, a[4], a[5], a[6], flags, lens, lens + 32, *a[7:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_affix_run_select: "), (what, rc, msg)
    # host pointers: offsets that decrease (the scans' refusal, before any device)
    bad = np.array([0, 5, 3, 8], dtype=np.uint64)
    assert L.pire_hip_affix_run_select(th._h, 1, tt._h, 1, x, bad.ctypes.data, 3, REST, 0, None, None, h, s, 4, c, None) == EINVAL
    assert "non-decreasing" in L.pire_hip_last_error().decode()
    assert cnt.value == 77 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="null head and null tail"):
        pb.affix_run_select(None, None, text, offs)


def test_affix_lines_gather_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"  ab \n\nb  \n").copy()
    th, tt = pb.Table(blob_of(("blanks", "n"))), pb.Table(blob_of(("blanks", "nr")))
    bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    r, lp, h, s, c = raw.ctypes.data, C.addressof(lines), bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt)
    x, xo, bp = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data, C.addressof(total)
    # (head, head_opts, tail, tail_opts, raw, size, delim, part, tail_byte, out_line_count, out_hits, out_spans, hit_cap, out_hit_count,
    #  out_text, text_cap, out_offsets, out_bytes)
    ok = [th._h, 1, tt._h, 1, r, raw.size, 10, REST, 10, lp, h, s, 4, c, x, 32, xo, bp]

    def but(**kw):
        names = ("head", "head_opts", "tail", "tail_opts", "raw", "size", "delim", "part", "tail_byte", "lines", "hits", "spans", "cap", "count",
                 "text", "text_cap", "offsets", "bytes")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a

    cases = {
        "null head and null tail": but(head=None, tail=None),
        "unknown bits in head_opts": but(head_opts=9),
        "unknown bits in tail_opts": but(tail_opts=0x100),
        "unknown part": but(part=7),
        "PIRE_HIP_AFFIX_HEAD without head_len": but(head=None, part=HEAD),
        "PIRE_HIP_AFFIX_TAIL without tail_len": but(tail=None, part=TAIL),
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
            rc = L.pire_hip_affix_lines_gather(*a[:8], flags, *a[8:], None)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and what in msg and msg.startswith("pire_hip_affix_lines_gather: "), (what, rc, msg)
    assert (cnt.value, lines.value, total.value) == (77, 78, 79) and _untouched(bufs)
    assert (raw == u8(b"  ab \n\nb  \n")).all()


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    th, tt = pb.Table(blob_of(("blanks", "n"))), pb.Table(blob_of(("blanks", "nr")))
    offs0 = np.zeros(1, dtype=np.uint64)
    dummy = np.zeros(2, dtype=np.int64)
    for part in PARTS:
        bufs, cnt, lines, total = _guarded(), C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
        h, s, c, lp = bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, C.addressof(cnt), C.addressof(lines)
        for o in (None, offs0.ctypes.data):
            cnt.value = 77
            assert L.pire_hip_affix_select(o, 0, part, 0, dummy.ctypes.data, dummy.ctypes.data, h, s, 4, c, None) == 0, L.pire_hip_last_error()
            assert cnt.value == 0
        cnt.value = 77
        assert L.pire_hip_affix_select(None, 0, REST, 0, None, None, h, s, 4, c, None) == 0 and cnt.value == 0   # (both null: n > 0 only)
        cnt.value = 77
        assert L.pire_hip_affix_run_select(th._h, 1, tt._h, 1, None, offs0.ctypes.data, 0, part, 0, None, None, h, s, 4, c, None) == 0
        assert cnt.value == 0 and lines.value == 78
        cnt.value = 77
        assert L.pire_hip_affix_lines_gather(th._h, 1, tt._h, 1, None, 0, 10, part, 0, 10, lp, h, s, 4, c, None, 0, None, None, None) == 0   # spans only
        assert (cnt.value, lines.value) == (0, 0)
        assert _untouched(bufs)
        cnt.value, lines.value = 77, 78
        assert L.pire_hip_affix_lines_gather(th._h, 1, tt._h, 1, None, 0, 10, part, 0, 10, lp, h, s, 4, c, bufs["text"].ctypes.data, 32,
                                             bufs["offsets"].ctypes.data, C.addressof(total), None) == 0
        assert (cnt.value, lines.value, total.value) == (0, 0, 0)
        assert bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
        bufs["offsets"][:8] = POISON
        assert _untouched(bufs)
    # the wrappers on nothing
    got = pb.affix_select_host(offs0, head_len=np.zeros(0, np.int64), part=HEAD)
    assert got["count"] == 0 and got["hits"].size == 0 and got["spans"].shape == (0, 2)
    got = pb.affix_run_select(th, tt, np.zeros(0, np.uint8), offs0, part=REST)
    assert got["count"] == 0 and got["hits"].size == 0 and got["head_len"].size == 0 and got["tail_len"].size == 0
    gg = pb.affix_lines_gather_host(th, None, b"", part=HEAD)
    assert gg["lines"] == 0 and gg["count"] == 0 and gg["bytes"] == 0 and gg["text"].size == 0 and gg["offsets"].tolist() == [0]


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """affix.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "affix.hip" in ba.NO_SCRATCH and "affix.hip" in ba.UNITS and "affix" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\baffix\.hip\b", mk)) == 2                              # NAMES and AUDIT_UNITS
    names = re.search(r"^NAMES\s*:=(.*)$", mk, re.M).group(1).split()
    units = re.search(r"^AUDIT_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "affix.hip" in names and "affix.hip" in units
    fails, seen = ba.audit("affix.hip")
    assert not fails, fails
    assert len(seen) == 2 and all("Affix" in k for k in seen), seen                 # classify, scatter


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "affix.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
    for shared in ('#include "tile_pass.h"', "TilePass t(", "t.Front(", "t.Classify(", "t.Tail(", "list.Count(", "list.List("):
        assert shared in src, shared
    assert "__shfl" not in src and "__ballot" not in src and "BlockExclusive" not in src   # (the scan is select.hip's, not a copy)
    # both kernels, the launcher and the copies back are the shared ones: the unit has a predicate and a Write, nothing else of a pass
    for copy in ("__global__", "hipLaunchKernelGGL", "TileBallot(", "TileRank(", "LaunchTileScan(", "TileCompaction(", "hipGetLastError", "hipMemcpy"):
        assert copy not in src, copy


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class Outs:
    """The outputs of one call, host or device, each `bytes` long between GUARD poisoned bytes; check() compares every one of
    them bytewise with what the model says the call writes -- and leaves alone."""

    def __init__(self, torch, device, cap, hits=True, spans=True, lines=False, head_len=0, tail_len=0, text=None):
        self.torch, self.device, self.cap = torch, device, cap
        sizes = {"count": 8, "hits": 8 * cap if hits else None, "spans": 16 * cap if spans else None, "lines": 8 if lines else None,
                 "head_len": 8 * head_len or None, "tail_len": 8 * tail_len or None, "text": text,
                 "offsets": None if text is None else 8 * (cap + 1), "bytes": None if text is None else 8}
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
        """exp: the model's answer with every hit; the first min(count, cap) entries of the lists, and nothing else, were written.
        more: the payload of every other output the call has"""
        now = self.read()
        k = min(exp["count"], self.cap)
        want = {"count": np.array([exp["count"]], dtype=np.uint64), "hits": exp["hits"][:k].astype(np.uint64),
                "spans": exp["spans"][:k].astype(np.uint64)}
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

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3001)
BASE = (1 << 32) - 100                                     # the offsets cross 2^32 (the pass takes no text: nothing is allocated there)


def drawn(rng, n, pattern):
    """offsets from BASE on (a few of them decreasing), and lengths through every row of the truth table"""
    lens = rng.randint(0, 24, size=n).astype(np.int64)
    lens[rng.rand(n) < 0.1] = 0
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    offs += np.uint64(BASE)
    if n > 4:
        down = rng.choice(np.arange(1, n), size=max(n // 50, 1), replace=False)
        offs[down] += np.uint64(30)                        # string down - 1 grows, string `down` has offsets that decrease (or shrinks)
    arrays = []
    for _ in range(2):
        kind = rng.randint(0, 8, size=n)
        inside = (rng.rand(n) * (lens + 1)).astype(np.int64)
        a = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0, lens, lens + 5, I64_MAX, -1], default=inside)
        a = np.where(rng.rand(n) < 0.03, I64_MIN, a)
        if pattern == "all":
            a = np.where(a < 0, inside, a)
        elif pattern == "none":
            a = np.where(rng.rand(n) < 0.5, -1, I64_MIN)
        arrays.append(a.astype(np.int64))
    return offs, arrays[0], arrays[1]


def call_pass(torch, device, host, dev, n, part, which, cap, hits, spans):
    out = Outs(torch, device, cap, hits, spans)
    ptrs = [t.data_ptr() for t in dev] if device else [a.ctypes.data for a in host]
    hp, tp = given(which, ptrs[1], ptrs[2])
    rc = pb.lib().pire_hip_affix_select(ptrs[0], n, part, pb.FLAG_ON_DEVICE if device else 0, hp, tp, out.ptr("hits") if cap else None,
                                        out.ptr("spans") if cap else None, cap, out.ptr("count"), stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out


@gpu
def test_no_strings_from_host_pointers_and_on_the_device(torch_cuda):
    """n == 0: a count of 0, whatever the capacity; no list is touched, on either side"""
    torch = torch_cuda
    host = (np.array([BASE], dtype=np.uint64), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))   # (somewhere to point)
    dev = [torch.as_tensor(i64(a), device="cuda") for a in host]
    calls = 0
    for which in ("both", "head", "tail"):
        hl, tl = given(which, host[1][:0], host[2][:0])
        for part in TRUTH[which][1]:
            exp = model_affix_select(host[0], hl, tl, part)
            assert exp["count"] == 0 and exp["spans"].shape == (0, 2)
            for cap in (0, 7):
                for hits, spans in ((True, False), (False, True), (True, True)) if cap else ((False, False),):
                    for device in (True, False):
                        what = (which, part, cap, hits, spans, "device" if device else "host")
                        call_pass(torch, device, host, dev, 0, part, which, cap, hits, spans).check(exp, what)
                        calls += 1
    assert calls == 7 * 4 * 2


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_on_arrays_drawn_by_the_test(torch_cuda, n):
    torch = torch_cuda
    rng = np.random.RandomState(2000 + n)
    calls = 0
    for pattern in ("mixed", "all", "none"):
        host = drawn(rng, n, pattern)
        before = [a.copy() for a in host]
        dev = [torch.as_tensor(i64(a), device="cuda") for a in host]
        assert int(host[0][0]) < (1 << 32) and (n < 63 or int(host[0][-1]) > (1 << 32))
        for which in ("both", "head", "tail"):
            hl, tl = given(which, host[1], host[2])
            for part in TRUTH[which][1]:
                exp = model_affix_select(host[0], hl, tl, part)
                count = exp["count"]
                if pattern != "mixed":
                    assert count == (n if pattern == "all" else 0)
                lo = host[0][exp["hits"].astype(np.int64)]
                hi = np.maximum(lo, host[0][exp["hits"].astype(np.int64) + 1])
                s = exp["spans"]
                assert ((lo <= s[:, 0]) & (s[:, 0] <= s[:, 1]) & (s[:, 1] <= hi)).all()
                for cap in sorted({c for c in (0, 1, count - 1, count, count + 7) if c >= 0}):
                    for hits, spans in ((True, False), (False, True), (True, True)) if cap else ((False, False),):
                        for device in (True, False):
                            what = (n, pattern, which, part, cap, hits, spans, "device" if device else "host")
                            call_pass(torch, device, host, dev, n, part, which, cap, hits, spans).check(exp, what)
                            calls += 1
        for a, b, d in zip(host, before, dev):
            assert (a == b).all() and (d.cpu().numpy().view(a.dtype) == b).all(), "an input was written to"
    assert calls >= 3 * 7 * 2 * 2
    # the wrappers, and the same input twice: the same bits
    offs, hl, tl = host = drawn(rng, n, "mixed")
    exp = model_affix_select(offs, hl, tl, REST)
    w = pb.affix_select_host(offs, hl, tl, part=REST, hit_cap=5)
    assert w["count"] == exp["count"] and (w["hits"] == exp["hits"][:5]).all() and (w["spans"] == exp["spans"][:5]).all()
    dev = [torch.as_tensor(i64(a), device="cuda") for a in host]
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    lists = torch.zeros((2, 2 * n), dtype=torch.int64, device="cuda")
    for k in range(2):
        pb.affix_select_device(dev[0].data_ptr(), n, cnt[k:].data_ptr(), head_len_ptr=dev[1].data_ptr(), tail_len_ptr=dev[2].data_ptr(), part=REST,
                               out_spans_ptr=lists[k].data_ptr(), hit_cap=n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = lists.cpu().numpy().view(np.uint64)
    assert cnt.cpu().tolist() == [exp["count"]] * 2 and (got[:, :2 * exp["count"]] == exp["spans"].reshape(-1)).all()


@gpu
def test_the_tile_loop_behind_the_largest_grid(torch_cuda):
    """8 194 tiles on a grid of 8 192 blocks: two blocks take a second tile.  The arrays are made on the device from formulas the
    host repeats; the count and the last 2 000 hits and spans against the model."""
    torch = torch_cuda
    n = 8194 * 1024
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    lens = i % 11
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    head = torch.where(i % 3 == 0, (i * 7) % 13, torch.full_like(i, -1))
    tail = torch.where(i % 5 != 2, (i * 5) % 7, torch.full_like(i, -1))
    hi = np.arange(n, dtype=np.int64)
    h_lens = hi % 11
    h_offs = np.zeros(n + 1, dtype=np.uint64)
    h_offs[1:] = np.cumsum(h_lens, dtype=np.uint64)
    h_head = np.where(hi % 3 == 0, (hi * 7) % 13, -1)
    h_tail = np.where(hi % 5 != 2, (hi * 5) % 7, -1)
    exp = model_affix_select(h_offs, h_head, h_tail, REST)
    count = exp["count"]
    assert exp["hits"][-1] >= 8193 * 1024 and exp["hits"][-2000] < 8192 * 1024 + 1024 and count > n // 4   # hits in the tiles of the second turn
    hits = torch.full((count + 8,), -1, dtype=torch.int64, device="cuda")
    spans = torch.full((2 * count + 8,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    pb.affix_select_device(offs.data_ptr(), n, cnt[1:].data_ptr(), head_len_ptr=head.data_ptr(), tail_len_ptr=tail.data_ptr(), part=REST,
                           out_hits_ptr=hits.data_ptr(), out_spans_ptr=spans.data_ptr(), hit_cap=count + 8,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [-1, count, -1]
    assert (hits[count - 2000:].cpu().numpy() == np.concatenate([exp["hits"][-2000:].astype(np.int64), np.full(8, -1)])).all()
    assert (spans[2 * count - 4000:].cpu().numpy() == np.concatenate([exp["spans"][-2000:].reshape(-1).astype(np.int64), np.full(8, -1)])).all()
    assert (hits[:1000].cpu().numpy() == exp["hits"][:1000].astype(np.int64)).all()


# ---- GPU: behind the two scans ------------------------------------------------------------------------------------------------------

def tables_of(pair):
    hs, ts = PAIRS[pair][0], PAIRS[pair][1]
    th = pb.Table(blob_of(hs))
    return th, th if hs == ts else pb.Table(blob_of(ts))


def run_form(torch, tabs, device, ptrs, n, part, head_opts, tail_opts, cap, keep, flags=0, hits=True, spans=True):
    """pire_hip_affix_run_select; keep: the caller has out_head_len / out_tail_len (poisoned first)"""
    th, tt = tabs
    out = Outs(torch, device, cap, hits, spans, head_len=n if keep and th else 0, tail_len=n if keep and tt else 0)
    rc = pb.lib().pire_hip_affix_run_select(th._h if th else None, head_opts, tt._h if tt else None, tail_opts, ptrs[0], ptrs[1], n, part,
                                            flags | (pb.FLAG_ON_DEVICE if device else 0), out.ptr("head_len"), out.ptr("tail_len"),
                                            out.ptr("hits") if cap else None, out.ptr("spans") if cap else None, cap, out.ptr("count"),
                                            stream_of(torch) if device else None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out


def lens_payload(hl, tl, keep):
    more = {}
    if keep and hl is not None:
        more["head_len"] = hl
    if keep and tl is not None:
        more["tail_len"] = tl
    return more


@gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_behind_the_prefix_and_suffix_scans(torch_cuda, pair):
    torch = torch_cuda
    tabs = tables_of(pair)
    assert (tabs[0] is tabs[1]) == (pair == "same_table")
    text, offs = H.pack(batch(pair))
    text, offs = text.copy(), offs.copy()
    n = len(offs) - 1
    dev_batch = (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))   # the text ends with the last string
    assert dev_batch[0].numel() == int(offs[-1])
    ptrs = {True: (dev_batch[0].data_ptr(), dev_batch[1].data_ptr()), False: (text.ctypes.data, offs.ctypes.data)}
    own_h, own_t = PAIRS[pair][6], PAIRS[pair][7]
    option_sets = [(own_h, own_t), (own_h & ~LONGEST, own_t & ~LONGEST)]
    if pair == "marked":                                                             # the four through-mark combinations
        option_sets += [(LONGEST | b | e, LONGEST | b | e) for b in (0, T_BEGIN) for e in (0, T_END)]
    kernels = set()
    for head_opts, tail_opts in option_sets:
        hl, tl = oracle_lengths(pair, head_opts, tail_opts)
        lo, tb, te = opts_args(head_opts)
        assert (tabs[0].prefix(text, offs, lo, tb, te) == hl).all()                    # the scans alone, and what they name
        head_kernel = pb.last_kernel()
        lo, tb, te = opts_args(tail_opts)
        assert (tabs[1].suffix(text, offs, lo, te, tb) == tl).all()
        tail_kernel = pb.last_kernel()
        kernels.add(head_kernel)
        for part in PARTS:
            exp = model_affix_select(offs, hl, tl, part)
            for device in (True, False):
                for keep in (True, False):
                    cap = n if keep else max(exp["count"] - 1, 0)
                    what = (pair, head_opts, tail_opts, part, "device" if device else "host", keep, cap)
                    out = run_form(torch, tabs, device, ptrs[device], n, part, head_opts, tail_opts, cap, keep)
                    assert pb.last_kernel() == tail_kernel, (what, pb.last_kernel())     # the scan that ran last
                    out.check(exp, what, **lens_payload(hl, tl, keep))
    # head only, tail only: the pass gets one array
    for only, one in (("head", (tabs[0], None)), ("tail", (None, tabs[1]))):
        hl, tl = oracle_lengths(pair, only=only)
        for part in TRUTH[only][1]:
            exp = model_affix_select(offs, hl, tl, part)
            assert exp["count"] > 0
            for device in (True, False):
                out = run_form(torch, one, device, ptrs[device], n, part, own_h, own_t, n, True, hits=device, spans=True)
                out.check(exp, (pair, only, part, device), **lens_payload(hl, tl, True))
    # once with PIRE_HIP_RUN_GENERIC (handed to the prefix scan), once after adapt() on both tables: the same answers
    hl, tl = oracle_lengths(pair)
    exp = model_affix_select(offs, hl, tl, REST)
    run_form(torch, tabs, True, ptrs[True], n, REST, own_h, own_t, n, True, flags=pb.FLAG_GENERIC).check(exp, (pair, "generic"), head_len=hl, tail_len=tl)
    for t in set(tabs):
        t.adapt()
    for device in (True, False):
        run_form(torch, tabs, device, ptrs[device], n, REST, own_h, own_t, n, True).check(exp, (pair, "adapted", device), head_len=hl, tail_len=tl)
    assert (dev_batch[0].cpu().numpy() == text).all() and (dev_batch[1].cpu().numpy().view(np.uint64) == offs).all()
    # the wrappers
    w = pb.affix_run_select(tabs[0], tabs[1], text, offs, part=REST, head_opts=own_h, tail_opts=own_t)
    assert w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all() and (w["spans"] == exp["spans"]).all()
    assert (w["head_len"] == hl).all() and (w["tail_len"] == tl).all()
    w = pb.affix_run_select(tabs[0], tabs[1], text, offs, part=REST, head_opts=own_h, tail_opts=own_t, hit_cap=3, lengths=False)
    assert w["count"] == exp["count"] and (w["spans"] == exp["spans"][:3]).all() and "head_len" not in w
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    spans = torch.full((n, 2), -1, dtype=torch.int64, device="cuda")
    pb.affix_run_select_device(tabs[0], tabs[1], ptrs[True][0], ptrs[True][1], n, cnt.data_ptr(), part=REST, head_opts=own_h, tail_opts=own_t,
                               out_spans_ptr=spans.data_ptr(), hit_cap=n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == exp["count"] and (spans.cpu().numpy()[:exp["count"]] == exp["spans"].astype(np.int64)).all()
    assert (spans.cpu().numpy()[exp["count"]:] == -1).all()
    print("%s: prefix kernels %s" % (pair, sorted(kernels)))


# ---- GPU: lines ---------------------------------------------------------------------------------------------------------------

LINES_CASES = (("trim", REST), ("stamp_blank", HEAD), ("exts", TAIL), ("alts", REST))


def expected_lines(pair, raw, delim, part, only=None):
    """Python's split, the oracle on the lines, the model with shift = 1 (spans are ranges of raw) -- and Python's slices"""
    parts, begins = py_lines(raw, bytes([delim]))
    if parts:
        hl, tl = oracle_lengths(pair, strings=parts, only=only)
    else:
        hl, tl = given("both" if only is None else only, np.zeros(0, np.int64), np.zeros(0, np.int64))
    exp = model_affix_select(H.pack(parts)[1], hl, tl, part, shift=1)
    texts = []
    for i, (b, e) in zip(exp["hits"].tolist(), exp["spans"].tolist()):
        s = parts[i]
        h = 0 if hl is None else min(int(hl[i]), len(s))
        t = 0 if tl is None else min(int(tl[i]), len(s))
        r = 0 if tl is None else min(int(tl[i]), len(s) - h)
        want = s[:h] if part == HEAD else s[len(s) - t:] if part == TAIL else s[h:len(s) - r]
        assert bytes(raw[b:e]) == want and int(begins[i]) <= b <= e <= int(begins[i]) + len(s), (pair, i)
        texts.append(want)
    return len(parts), exp, texts


def lines_call(torch, tabs, device, raw, delim, part, opts, cap, gather=None, hits=True, spans=True):
    """gather: None -- spans only --, or (tail_byte, text_cap)"""
    keep = torch.as_tensor(raw, device="cuda") if device and len(raw) else raw
    rp = (keep.data_ptr() if device else keep.ctypes.data) if len(raw) else None
    th, tt = tabs
    tail_byte, text_cap = gather if gather else (0, None)
    out = Outs(torch, device, cap, hits, spans, lines=True, text=text_cap)
    rc = pb.lib().pire_hip_affix_lines_gather(th._h if th else None, opts[0], tt._h if tt else None, opts[1], rp, len(raw), delim, part,
                                              pb.FLAG_ON_DEVICE if device else 0, tail_byte, out.ptr("lines"), out.ptr("hits") if cap else None,
                                              out.ptr("spans") if cap else None, cap, out.ptr("count"), out.ptr("text") if text_cap else None,
                                              text_cap or 0, out.ptr("offsets"), out.ptr("bytes"), stream_of(torch))
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out, keep


@gpu
@pytest.mark.parametrize("pair,part", LINES_CASES)
def test_lines_in_matched_text_out(torch_cuda, pair, part):
    torch = torch_cuda
    tabs = tables_of(pair)
    opts = (PAIRS[pair][6], PAIRS[pair][7])
    lines = lines_of(pair)
    joined = b"\n".join(lines)
    buffers = [(u8(joined).copy(), 10), (u8(joined + b"\n").copy(), 10), (u8(b"\n" * 70).copy(), 10), (u8(b"").copy(), 10),
               (u8(b"|".join(lines) + b"|").copy(), ord("|"))]
    for raw, delim in buffers:
        nlines, exp, texts = expected_lines(pair, raw, delim, part)
        assert nlines == (0 if not len(raw) else 70 if raw[0] == 10 else len(lines))
        count = exp["count"]
        lines_word = np.array([nlines], dtype=np.uint64)
        for device in (True, False):
            for cap in sorted({nlines, max(count - 1, 0)}):
                what = (pair, part, len(raw), delim, "device" if device else "host", cap)
                k = min(count, cap)
                # all gather outputs null: spans only
                out, keep = lines_call(torch, tabs, device, raw, delim, part, opts, cap)
                out.check(exp, what, lines=lines_word)
                for tail_byte in (0, 1 + delim):
                    want = b"".join(t + bytes([tail_byte]) for t in texts[:k])
                    ends = np.cumsum([0] + [len(t) + 1 for t in texts[:k]]).astype(np.uint64)
                    for with_lists in (True, False):
                        out, keep = lines_call(torch, tabs, device, raw, delim, part, opts, cap, gather=(tail_byte, len(raw) + cap),
                                               hits=with_lists, spans=with_lists)
                        out.check(exp, what + (tail_byte, with_lists), text=want, offsets=ends, bytes=np.array([len(want)], dtype=np.uint64),
                                  lines=lines_word)
                if device and len(raw):
                    assert (keep.cpu().numpy() == raw).all(), "the input was written to"
    # one table alone: grep -o '^re' (the head) and sed 's/^re//' on the lines that match (the rest)
    raw = u8(joined + b"\n").copy()
    for only, one, one_part in (("head", (tabs[0], None), HEAD), ("head", (tabs[0], None), REST), ("tail", (None, tabs[1]), REST)):
        nlines, exp, texts = expected_lines(pair, raw, 10, one_part, only=only)
        want = b"".join(t + b"\n" for t in texts)
        ends = np.cumsum([0] + [len(t) + 1 for t in texts]).astype(np.uint64)
        out, _ = lines_call(torch, one, True, raw, 10, one_part, opts, nlines, gather=(10, len(raw) + nlines))
        out.check(exp, (pair, only, one_part), text=want, offsets=ends, bytes=np.array([len(want)], dtype=np.uint64),
                  lines=np.array([nlines], dtype=np.uint64))
    # the wrappers
    nlines, exp, texts = expected_lines(pair, raw, 10, part)
    g = pb.affix_lines_gather_host(tabs[0], tabs[1], raw, part=part, head_opts=opts[0], tail_opts=opts[1])
    want = b"".join(t + b"\n" for t in texts)
    assert g["lines"] == nlines and g["count"] == exp["count"] and (g["hits"] == exp["hits"]).all() and (g["spans"] == exp["spans"]).all()
    assert g["text"].tobytes() == want and g["bytes"] == len(want)
    g = pb.affix_lines_gather_host(tabs[0], tabs[1], raw, part=part, head_opts=opts[0], tail_opts=opts[1], gather=False, hit_cap=7)
    assert g["count"] == exp["count"] and (g["spans"] == exp["spans"][:7]).all() and "text" not in g


@gpu
def test_the_chain_by_hand_on_device_pointers(torch_cuda):
    """pire_hip_split -> pire_hip_prefix -> pire_hip_suffix -> pire_hip_affix_select -> pire_hip_gather_spans, every pointer the
    device's and nothing read back in between: the bytes of the fused call (a trim of both ends)"""
    torch = torch_cuda
    pair = "trim"
    th, tt = tables_of(pair)
    lines = lines_of(pair)
    raw = u8(b"\n".join(lines) + b"\n").copy()
    nlines, exp, texts = expected_lines(pair, raw, 10, REST)
    want = b"".join(t + b"\n" for t in texts)
    n = nlines                                                   # (the host knows how many lines it joined: room for the offsets)
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(raw, device="cuda")
    d_text = torch.zeros(len(raw), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int64, device="cuda")   # n, the hit count, the bytes
    d_head = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    d_tail = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    d_spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    d_out = torch.full((len(raw) + n,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    pb.split_device(d_raw.data_ptr(), len(raw), words.data_ptr(), out_text_ptr=d_text.data_ptr(), out_offsets_ptr=d_offs.data_ptr(),
                    offsets_cap=n, stream=stream)
    th.prefix_device(d_text.data_ptr(), d_offs.data_ptr(), n, True, d_head.data_ptr(), stream=stream)
    tt.suffix_device(d_text.data_ptr(), d_offs.data_ptr(), n, True, d_tail.data_ptr(), stream=stream)
    pb.affix_select_device(d_offs.data_ptr(), n, words[1:].data_ptr(), head_len_ptr=d_head.data_ptr(), tail_len_ptr=d_tail.data_ptr(), part=REST,
                           out_spans_ptr=d_spans.data_ptr(), hit_cap=n, stream=stream)
    rc = pb.lib().pire_hip_gather_spans(d_text.data_ptr(), len(raw), d_spans.data_ptr(), words[1:].data_ptr(), n, 10, pb.FLAG_ON_DEVICE,
                                        d_out.data_ptr(), len(raw) + n, d_ends.data_ptr(), words[2:].data_ptr(), stream)
    assert rc == 0, pb.lib().pire_hip_last_error()
    torch.cuda.synchronize()
    assert words.cpu().tolist() == [n, exp["count"], len(want)]
    got = d_out.cpu().numpy()
    assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all()
    # ... which is what the fused call wrote
    out, _ = lines_call(torch, (th, tt), True, raw, 10, REST, (LONGEST, LONGEST), n, gather=(10, len(raw) + n))
    ends = np.cumsum([0] + [len(t) + 1 for t in texts]).astype(np.uint64)
    out.check(exp, "fused", text=want, offsets=ends, bytes=np.array([len(want)], dtype=np.uint64), lines=np.array([n], dtype=np.uint64))
    assert (d_ends.cpu().numpy()[:exp["count"] + 1].view(np.uint64) == ends).all()
