"""Every text path at byte offsets past 4 GiB.

The C ABI takes 64-bit byte offsets and sizes; inside the kernels positions are 32 bits wide wherever a task is small enough
(the stream kernel's positions from its sub-task's first line, the per-lane offsets of the tiled, wide and pair kernels, the
tile-relative positions of split, gather and fields, the lengths of the counting and capture kernels).  Each narrowing is
right only while the base it is relative to, and every running byte total, stays 64 bits wide.  Nothing else in the suite
hands an entry point a byte that lies 2^32 or more behind the text pointer.

Part A lays the small batches the suite already uses across byte 2^32 of one buffer of 2^32 + 2^26 bytes -- 2^32 between two
strings, inside one in the middle of a 16-byte chunk, inside one on a 128-byte line, on an empty string; the batch starting
0, 1, 77 and 112 bytes into a line -- and addresses each placement twice: pointer = the buffer, offsets[0] = lead (every
offset near or past 2^32 is used), and pointer = buffer + lead, offsets from 0 (only the address is large: the control that
tells a truncated offset from a truncated address).  Part B fills the buffer with one period of 2^24 bytes of corpus lines,
257 times, and runs the entry points that divide their work by running byte totals over all of it; what is expected is the
oracle's answer on ONE period, repeated on the device.

Every expected value is the oracle's (or getline / awk semantics written down with numpy) on a zero-based host copy, every
comparison is exact, outputs are poisoned before the call, and every case asserts the kernel it meant to reach.

Not covered: the stream kernel's walk for positions that do not fit 32 bits (a string of 4 GiB among short ones:
one lane walks it byte by byte), host-pointer calls above 4 GiB, multi-device shards."""
import functools
import zlib

import numpy as np
import pytest

from oracle import binding as ob
from pire_amd import workloads as W
from tests import helpers as H
from tests.test_poisoned_surroundings import EmbeddedAt, long_mix, poisoned, short_mix
from tests.test_slow_forms import FORMS as SLOW_FORMS, ORDER_FROM, Out as SlowOut, blob_of as slow_blob, case_strings as slow_strings

G4 = H.FOUR_GIB
BIG_BYTES = G4 + (1 << 26)
P, K = 1 << 24, 257                      # Part B: the period and how often it is repeated, K * P = 2^32 + 2^24
BE = ob.FLAG_BEGIN | ob.FLAG_END
gpu = pytest.mark.gpu
POISON64 = int(np.uint64(0xA5A5A5A5A5A5A5A5).astype(np.int64))      # what `poisoned` leaves in an int64

BATCHES = ("short508", "long900", "short100")
PLACEMENTS = [(b, w, H.ACROSS_LEAD_MODS[(i + j) % 4]) for i, b in enumerate(BATCHES) for j, w in enumerate(H.ACROSS_WHERE)]

# family of strings -> the alphabet its mixes draw from
ALPHABETS = {
    "set_a": b"ABCDEFGHIJKLMNOPQRSTUVWXYZ hello wd0123456789-() @net",   # tests/test_poisoned_surroundings.py, with set_a
    "abc": b"abcde w",                                                    # ... with the half-final and counting tables
    "count": b"abcdef ,w",                                                # the counting tables (count_ut.cpp's texts)
    "tsv": b"abc\tde w",                                                  # columns
    "digits": b"=12 ab;",                                                 # capture_digits: =(\d+)[^\d]
}


def big_set(name):
    return [b for b in H.big_sets() if b["name"] == name][0]


def golden_case(group, name):
    return [c for c in H.golden()[group] if c["name"] == name][0]


def mix(batch, rng, alphabet):
    if batch == "short508":
        return short_mix(rng, 508, alphabet)
    if batch == "long900":
        return long_mix(rng, 900, alphabet)
    return short_mix(rng, 100, alphabet)


@functools.lru_cache(maxsize=None)
def batch_of(family, batch):
    """The strings of a family's batch, before they are placed: (strings, pad)."""
    rng = np.random.RandomState(zlib.crc32(("%s/%s" % (family, batch)).encode()) & 0x7FFFFFFF)
    if family == "dict_1k":
        # the dictionary scanner's own corpus cut to the mix's lengths; every third string holds a whole word of the
        # dictionary (the Surround()ed scanner is Final for good behind it)
        entry = W.wide_set("dict_1k")
        lens = [len(s) for s in mix(batch, rng, b"a")]
        flat = W.wide_records(entry, "k512", 23, (sum(lens) + 127) // 1024 + 2, 1024).reshape(-1)
        ends = np.cumsum(lens)
        strings = [flat[int(e) - k:int(e)].tobytes() for e, k in zip(ends, lens)]
        words = W.dictionary_words(entry)
        for i in range(0, len(strings), 3):
            w = words[(11 + i) % len(words)]
            if len(strings[i]) >= len(w) + 2:
                at = (len(strings[i]) - len(w)) // 2
                strings[i] = strings[i][:at] + w + strings[i][at + len(w):]
        return tuple(strings), flat[int(ends[-1]):int(ends[-1]) + 127].tobytes()
    if family == "google":
        # as tests/test_capture.py: the capture case's own strings among random bytes of its alphabet
        case = golden_case("capturing", "capture_google")
        pool = [bytes.fromhex(h) for h in case["strings_hex"][:5]]
        a = b"google_id ='\";x1/"
        strings = []
        for s in mix(batch, rng, a):
            strings.append(s[:len(s) // 2] + pool[rng.randint(0, len(pool))] + s[len(s) // 2:] if rng.randint(0, 3) == 0 else s)
        return tuple(strings), bytes(rng.choice(np.frombuffer(a, dtype=np.uint8), size=127))
    a = ALPHABETS[family]
    strings = mix(batch, rng, a)
    if family == "count":           # count2's regexp is http://[a-z]+: one in every fourth string
        strings = [s[:len(s) // 2] + b"http://abc, " + s[len(s) // 2:] if i % 4 == 0 else s for i, s in enumerate(strings)]
    return tuple(strings), bytes(rng.choice(np.frombuffer(a, dtype=np.uint8), size=127))


@functools.lru_cache(maxsize=None)
def placed(family, batch, where, mod):
    """(strings, lead, k, d) of a Part A placement: helpers.across_4gib on the family's batch."""
    strings, pad = batch_of(family, batch)
    s, lead, k, d = H.across_4gib(strings, where, mod, pad)
    return tuple(s), lead, k, d


LARGE_REPEATS = 26        # (900 + 508) * 26 = 36 608 strings: more than order.hip's 32 768, from which the strings are ordered


@functools.lru_cache(maxsize=None)
def large_placed(family, where):
    """(strings, lead, k, d): the family's long900 and short508 batches LARGE_REPEATS times over, laid across 2^32 -- a batch
    that the kernels with one string per lane take in the order of its length classes (order.hip OrdersByLength)."""
    strings = (batch_of(family, "long900")[0] + batch_of(family, "short508")[0]) * LARGE_REPEATS
    s, lead, k, d = H.across_4gib(strings, where, H.ACROSS_LEAD_MODS[H.ACROSS_WHERE.index(where)], batch_of(family, "long900")[1])
    return tuple(s), lead, k, d


SEGMENT_CUTS = (0, 200 * 1024, 400 * 1024 + 5, 600 * 1024)
SEGMENT_PLACES = ((0, 100 * 1024 + 8), (77, 3 * 4096), (1, 4096 * 7 - 1), (112, 1))     # lead % 128, bytes of string 1 below 2^32


@functools.lru_cache(maxsize=None)
def segment_strings():
    """Three strings of about 200 KiB of set_a's corpus: the first and the last end with a record (most records end with a
    planted match), the second five bytes into one."""
    entry = big_set("set_a")
    rec = ob.corpus_fill(31, 0, 150, 4096, H.plants_for(entry), threads=4).reshape(-1)
    return tuple(rec[a:b].tobytes() for a, b in zip(SEGMENT_CUTS, SEGMENT_CUTS[1:]))


def segment_lead(mod, d):
    lead = G4 - SEGMENT_CUTS[1] - d
    return lead - (lead - mod) % 128


def slow_placed(case, where):
    """(strings, lead, k, d): a SlowScanner fixture's own strings (tests/test_slow_forms.py) laid across 2^32."""
    return want(("slow placed", case["name"], where),
                lambda: H.across_4gib(slow_strings(case), where, H.ACROSS_LEAD_MODS[H.ACROSS_WHERE.index(where)],
                                      ((case["head"].encode() or b"x") * 127)[:127]))


_want = {}


def want(key, compute):
    """An expected value, computed once and shared by the cases that need it; never changed."""
    if key not in _want:
        _want[key] = compute()
    return _want[key]


def fields_of(strings, field, sep=9, rest=False):
    """pire_hip_fields as include/pire_hip.h states it, on strings packed from 0: int64[n, 2]."""
    out, at = np.zeros((len(strings), 2), dtype=np.int64), 0
    for i, s in enumerate(strings):
        q = [at - 1] + [at + j for j, c in enumerate(s) if c == sep] + [at + len(s)]
        m = len(q) - 2
        out[i] = (q[field] + 1, at + len(s) if rest else q[field + 1]) if field <= m else (at + len(s), at + len(s))
        at += len(s)
    return out


def masks_of(o, idx):
    """(mask u64[n], final bool[n]) of the end states `idx`, from the oracle's accessors (tables of up to 64 regexps)."""
    rec = {s: (sum(1 << r for r in o.accepted(s) if r < o.regexps), o.final(s) and o.regexps > 0) for s in np.unique(idx).tolist()}
    return (np.array([rec[s][0] for s in idx.tolist()], dtype=np.uint64), np.array([rec[s][1] for s in idx.tolist()], dtype=bool))


# ---- CPU: the expectations are not trivial -------------------------------------------------------------------------------

def both(mask, side):
    return bool(mask[side].any()) and bool((~mask[side]).any())


def test_the_placements_and_the_period_put_something_on_both_sides_of_4gib():
    """The inputs of the GPU tests below, from the same builders, with the oracle alone.  Every Part A placement: a string
    that starts below 2^32 and one that starts at or above it; 2^32 where the placement says (between two strings that are
    not empty, behind byte d of string k with d % 16 == 8 or d a whole number of lines, on an empty string); lead % 128 as
    asked; with `chunk` and `line` a string that has byte 2^32 in its interior; on both sides a Final and a non-Final end
    state (BEGIN | END) -- a count and none, a prefix and none for the half-final tables; counts, and more than one row of
    them, for the counting tables --, a capture and none, a second column and none; the SlowScanner fixtures' strings end in
    more than one set of states on either side.  Part B: the period has hits and misses, by whole lines and by their second
    column; the state map of a period is not constant."""
    scanners = {
        "set_a": [ob.OracleScanner(H.load_blob(big_set("set_a")["blob"]))],
        "dict_1k": [ob.OracleScanner(W.load_blob(W.wide_set("dict_1k")["blob"]))],
    }
    mods = set()
    for family in ("set_a", "abc", "count", "dict_1k", "tsv", "digits", "google"):
        for batch, where, mod in PLACEMENTS:
            strings, lead, k, d = placed(family, batch, where, mod)
            what = (family, batch, where, mod)
            below, above, inside = H.sides_of_4gib(strings, lead)
            _, offs = H.pack(strings)
            assert below.any() and above.any() and lead % 128 == mod and int(offs[k]) + d + lead == G4, what
            mods.add((where, mod))
            if where == "between":
                assert len(strings[k - 1]) and len(strings[k]) and d == 0 and not inside.any(), what
            elif where == "empty":
                assert strings[k] == b"" and d == 0, what
            else:
                assert inside[k] and inside.sum() == 1 and 0 < d < len(strings[k]), what
                assert d % 16 == 8 if where == "chunk" else d % (128 if batch == "long900" else 16) == 0, what
            for o in scanners.get(family, []):
                fin = o.run_strings(list(strings))[1].astype(bool)
                assert both(fin, below) and both(fin, above), what
            if family == "abc":
                # (the half-final tables end none of these strings in a Final state: what they count, and the prefixes and
                # suffixes they find, are their results)
                for _, blob in half_tables():
                    o = ob.OracleScanner(blob)
                    text, offs = ob.pack_strings(list(strings))
                    for hit in ((o.run_half_final(text, offs)[2] > 0).any(axis=1), o.prefix(text, offs, True, True, True) >= 0,
                                o.suffix(text, offs, True, True, True) >= 0):
                        assert both(hit, below) and both(hit, above), what
            if family == "count":
                for c in H.golden()["counting"]:
                    res = ob.OracleCountingScanner(H.load_blob(c["blob"]), c["kind"]).run_strings(list(strings))[1]
                    assert res[below].any() and res[above].any(), what + (c["name"],)
                    assert len(np.unique(res[below], axis=0)) > 1 and len(np.unique(res[above], axis=0)) > 1, what + (c["name"],)
            if family in ("digits", "google"):
                blob = H.load_blob(golden_case("capturing", "capture_" + family)["blob"])
                cap = ob.OracleCountingScanner(blob, 0).capture(*ob.pack_strings(list(strings)))[2].astype(bool)
                assert both(cap, below) and both(cap, above), what
            if family == "tsv":
                f = fields_of(strings, 1)
                some = f[:, 1] > f[:, 0]
                assert both(some, below) and both(some, above), what
    assert {m for _, m in mods} == set(H.ACROSS_LEAD_MODS) and len(mods) == 12
    for case in SLOW_FORMS:           # the SlowScanner fixtures' own strings
        o = ob.OracleSlowScanner(slow_blob(case))      # (few of them match; without the End step the state sets tell them apart)
        for where in H.ACROSS_WHERE:
            strings, lead = slow_placed(case, where)[:2]
            below, above, _ = H.sides_of_4gib(strings, lead)
            bits = o.run_strings(strings, flags=ob.FLAG_BEGIN)[1]
            assert below.any() and above.any(), (case["name"], where)
            assert len(np.unique(bits[below], axis=0)) > 1 and len(np.unique(bits[above], axis=0)) > 1, (case["name"], where)
    # the three long strings of the segmented case: one that starts below 2^32 and ends Final, the one that holds 2^32 and
    # does not, one that starts above (three strings cannot put both kinds on both sides)
    seg = list(segment_strings())
    fin = ob.OracleScanner(H.load_blob(big_set("set_a")["blob"])).run_strings(seg)[1].tolist()
    assert fin == [1, 0, 1] and all(190 * 1024 < len(x) < 210 * 1024 for x in seg)
    for mod, d in SEGMENT_PLACES:
        lead = segment_lead(mod, d)
        below, above, inside = H.sides_of_4gib(seg, lead)
        assert lead % 128 == mod and below.tolist() == [True, True, False] and inside.tolist() == [False, True, False], (mod, d)
    # Part B
    for shares in strided_expectations()["shares"].values():      # the fixed-length records: hits and misses in every period
        assert 0.05 < shares < 0.95, strided_expectations()["shares"]
    assert RECORDS * STRIDE > G4 and (RECORDS + 37) * STRIDE + (1 << 20) <= BIG_BYTES
    per = period()
    assert per.raw.size == P and per.raw[-1] == 10 and K * P == G4 + (1 << 24) and per.lines * K >= 1 << 20
    assert 1024 <= per.lens.min() and per.lens.max() <= 4096
    for fin in (per.final, per.field_final):
        assert 0.05 < fin.mean() < 0.95
    assert len({per.state_map(s) for s in (per.o.initial, 0, 1, per.o.size // 2, per.o.size - 1)}) > 1


# ---- Part B's period (host side) -----------------------------------------------------------------------------------------

class Period:
    """One period of Part B: `raw` (P bytes of lines, each ended by a newline), what getline makes of it (text, offs), and the
    oracle's answers on it for set_a."""

    def __init__(self):
        entry = big_set("set_a")
        self.raw, self.lens = H.period_of_lines(H.plants_for(entry), P, 5)
        self.lines = len(self.lens)
        self.text = self.raw[self.raw != 10]
        self.offs = np.zeros(self.lines + 1, dtype=np.uint64)
        self.offs[1:] = np.cumsum(self.lens)
        self.keep = self.offs + np.arange(self.lines + 1, dtype=np.uint64)     # line i is raw[keep[i], keep[i + 1] - 1)
        self.o = ob.OracleScanner(H.load_blob(entry["blob"]))
        self.idx, fin = self.o.run(self.text, self.offs, threads=4)
        self.final = fin.astype(bool)
        # the second column of every line (one separator a third of the way in), scanned alone
        self.fields = np.stack([self.offs[:-1].astype(np.int64) + self.lens // 3 + 1, self.offs[1:].astype(np.int64)], axis=1)
        cols = [self.text[b:e].tobytes() for b, e in self.fields.tolist()]
        self.field_idx, ffin = self.o.run_strings(cols, threads=4)
        self.field_final = ffin.astype(bool)
        self._map = {}

    def state_map(self, s):
        """The state the scanner is in behind one period that it entered in state s (no Begin, no End)."""
        if s not in self._map:
            self._map[s] = int(self.o.run(self.raw, np.array([0, P], dtype=np.uint64), flags=0, init_idx=[s])[0][0])
        return self._map[s]


@functools.lru_cache(maxsize=None)
def period():
    return Period()


# ---- the buffer ------------------------------------------------------------------------------------------------------------

def device_bytes(torch, nbytes, more=0):
    """A device buffer of nbytes; the test skips where the device has not that much free memory (and `more` for what the
    test allocates besides)."""
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + more + (1 << 28):
        pytest.skip("%.1f GiB of device memory free, the test needs %.1f" % (free / 2 ** 30, (nbytes + more) / 2 ** 30 + 0.25))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def big():
    """The one buffer of 2^32 + 2^26 bytes, filled with 0xA5 once."""
    import torch

    assert torch.cuda.is_available()
    buf = device_bytes(torch, BIG_BYTES)
    buf.fill_(0xA5)
    try:
        yield buf
    finally:
        del buf
        torch.cuda.empty_cache()


@pytest.fixture
def periodic(big):
    """`big` holding the period K times (Part B), laid anew for every test: the other tests write into the buffer."""
    import torch

    block = torch.as_tensor(period().raw, device="cuda")
    big[:K * P].view(K, P).copy_(block.expand(K, P))
    big[K * P:].fill_(0xA5)
    torch.cuda.synchronize()
    return big


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def placements(big, family, skews=(0,), batches=BATCHES):
    """Every placement of the family, each in both addressings: (what, strings, EmbeddedAt)."""
    for batch, where, mod in PLACEMENTS:
        if batch not in batches:
            continue
        strings, lead, _, _ = placed(family, batch, where, mod)
        for skew in skews:
            for shifted in (True, False):
                yield (family, batch, where, mod, skew, "offsets" if shifted else "pointer"), list(strings), \
                    EmbeddedAt(big, strings, lead, shifted, skew)


def large_placements(big, family):
    """The family's batch of LARGE_REPEATS mixes in every placement and both addressings: (what, strings, EmbeddedAt)."""
    for where in H.ACROSS_WHERE:
        strings, lead, _, _ = large_placed(family, where)
        for shifted in (True, False):
            yield (family, "large", where, lead % 128, 0, "offsets" if shifted else "pointer"), list(strings), \
                EmbeddedAt(big, strings, lead, shifted)


def host(t):
    return t.cpu().numpy()


def same_states(idx, fin, oi, of, what):
    gi, gf = host(idx).astype(np.uint32), host(fin)
    bad = np.nonzero((gi != oi) | (gf != of))[0]
    assert bad.size == 0, (what, bad[:8], gi[bad[:8]], oi[bad[:8]])


# ---- Part A: pire_hip_run ------------------------------------------------------------------------------------------------

def run_cases(torch, pb, big, t, o, family, kernel_of, symbol_ok=None, generic=False):
    from tests.test_gpu_parity import expected_counts

    s = stream_of(torch)
    gen = pb.FLAG_GENERIC if generic else 0
    for what, strings, e in placements(big, family):
        n = e.n
        idx, fin = poisoned(n, torch.int32), poisoned(n, torch.uint8)
        for flags in (BE, 0):
            oi, of = want(("run", o.tag) + what[:4] + (flags,), lambda: o.run(e.text, e.offs, flags=flags))
            cnt = torch.zeros(o.regexps + 2, dtype=torch.int64, device="cuda")
            t.run_device(e.ptr, e.dev_offs.data_ptr(), n, flags | gen, idx.data_ptr(), fin.data_ptr(), cnt.data_ptr(), 0, s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == kernel_of(n, False), (what, flags, pb.last_kernel())
            assert symbol_ok is None or symbol_ok(n, pb.last_kernel_symbol()), (what, pb.last_kernel_symbol())
            same_states(idx, fin, oi, of, what + (flags,))
            assert (host(cnt).astype(np.uint64) == want(("counts", o.tag) + what[:4] + (flags,), lambda: expected_counts(o, oi, of))).all(), what
            idx.view(torch.uint8).fill_(0xA5), fin.fill_(0xA5)
        # every string resumed in a state of its own (init_state_idx); counters again
        init = np.random.RandomState(n).randint(0, o.size, size=n).astype(np.uint32)
        oi, of = want(("resume", o.tag) + what[:4], lambda: o.run(e.text, e.offs, flags=ob.FLAG_END, init_idx=init))
        dinit = torch.as_tensor(init.astype(np.int32), device="cuda")
        cnt = torch.zeros(o.regexps + 2, dtype=torch.int64, device="cuda")
        t.run_device(e.ptr, e.dev_offs.data_ptr(), n, ob.FLAG_END | gen, idx.data_ptr(), fin.data_ptr(), cnt.data_ptr(), dinit.data_ptr(), s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == kernel_of(n, True), (what, "resume", pb.last_kernel())
        same_states(idx, fin, oi, of, what + ("resume",))
        assert int(cnt[1]) == n and int(cnt[0]) == int(of.sum()), what


@gpu
@pytest.mark.parametrize("kernel", ["ragged", "stream", "generic"])
def test_run_across_4gib(big, cfg, kernel):
    """pire_hip_run on set_a through the ragged kernel, the stream kernel (>= 256 strings) and the generic one: flags 3 and 0,
    out_counts, init_state_idx (the stream kernel starts every string in the same state: resumed batches keep `ragged`)."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_offsets_peek=1, ragged_variant=2 if kernel == "stream" else 1)
    blob = H.load_blob(big_set("set_a")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    o.tag = "set_a"

    def kernel_of(n, resumed):
        if kernel == "generic" or n < 256:
            return "generic"
        return "ragged" if resumed else kernel

    run_cases(torch, pb, big, t, o, "set_a", kernel_of, generic=kernel == "generic")


@gpu
@pytest.mark.parametrize("zipv", [1, 2], ids=["plain rows", "zipped"])
@pytest.mark.parametrize("kernel", ["ragged_wide", "stream_wide"])
def test_run_across_4gib_on_the_wide_walk(big, cfg, kernel, zipv):
    """The same through the class-indexed walk of a dictionary scanner (dict_1k), plain rows and zipped."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_offsets_peek=1, ragged_variant=2 if kernel == "stream_wide" else 1, walk_variant=2, zip_variant=zipv, auto_adapt=1)
    blob = W.load_blob(W.wide_set("dict_1k")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    o.tag = "dict_1k"

    def kernel_of(n, resumed):
        return "generic" if n < 256 else "ragged_wide" if resumed else kernel

    run_cases(torch, pb, big, t, o, "dict_1k", kernel_of, symbol_ok=lambda n, sym: ("zipped" in sym) == (zipv == 2 and n >= 256))


@gpu
def test_segmented_run_across_4gib(big, cfg):
    """Three strings of about 200 KiB, 2^32 inside the second one, cut into segments (segment_bytes set): offsets on the host
    (the segmented scan needs the lengths there), both addressings."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(segment_bytes=4096, segment_warmup=256)
    blob = H.load_blob(big_set("set_a")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    strings = list(segment_strings())
    s = stream_of(torch)
    for mod, d in SEGMENT_PLACES:
        lead = segment_lead(mod, d)
        for shifted in (True, False):
            e = EmbeddedAt(big, strings, lead, shifted)
            idx, fin = poisoned(3, torch.int32), poisoned(3, torch.uint8)
            for flags in (BE, 0):
                oi, of = want(("seg", flags), lambda: o.run(e.text, e.offs, flags=flags))
                t.run_device_host_offsets(e.ptr, e.host_offs, flags, idx.data_ptr(), fin.data_ptr(), 0, 0, s)
                torch.cuda.synchronize()
                assert pb.last_kernel().startswith("segmented"), pb.last_kernel()
                same_states(idx, fin, oi, of, (mod, d, shifted, flags))
                idx.view(torch.uint8).fill_(0xA5), fin.fill_(0xA5)


# ---- Part A: the walks with actions --------------------------------------------------------------------------------------

def half_tables():
    return [(c["name"], H.load_blob(c["blob"])) for c in H.golden()["half_final"] if c["name"] in ("half_0", "half_1", "half_3")]


def prefix_suffix_half_final(torch, pb, big, t, o, family, n_kernel, skews=(0,), suffix=True, batches=BATCHES, symbol_ok=None):
    """pire_hip_prefix, pire_hip_suffix and pire_hip_run_half_final on every placement; n_kernel(n) -> the names of the prefix
    and the half-final kernel for a batch of n strings.  (Prefix and half-final kernels read 16-byte chunks from the string's
    first byte; only the suffix kernel's blocks depend on where the text pointer lies in a block: `skews` is for it.)"""
    s = stream_of(torch)
    for what, strings, e in placements(big, family, skews, batches):
        n = e.n
        key = (o.tag,) + what[:4]
        idx, fin, ln = poisoned(n, torch.int32), poisoned(n, torch.uint8), poisoned(n, torch.int64)
        res = poisoned((n, o.regexps), torch.int32)
        names = n_kernel(n)
        if what[4] == 0:
            for flags in (BE, 0):
                oi, of, orr = want(("half", flags) + key, lambda: o.run_half_final(e.text, e.offs, flags=flags))
                t.run_half_final_device(e.ptr, e.dev_offs.data_ptr(), n, flags, idx.data_ptr(), fin.data_ptr(), res.data_ptr(), s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == names["half_final"], (what, flags, pb.last_kernel())
                assert symbol_ok is None or symbol_ok(pb.last_kernel_symbol()), (what, pb.last_kernel_symbol())
                same_states(idx, fin, oi, of, what + (flags,))
                got = host(res).astype(np.uint32)
                assert (got == orr).all(), (what, flags, np.nonzero((got != orr).any(axis=1))[0][:8])
                idx.view(torch.uint8).fill_(0xA5), fin.fill_(0xA5), res.view(torch.uint8).fill_(0xA5)
            for longest in (True, False):
                w = want(("prefix", longest) + key, lambda: o.prefix(e.text, e.offs, longest, True, True))
                t.prefix_device(e.ptr, e.dev_offs.data_ptr(), n, longest, ln.data_ptr(), through_begin=True, through_end=True, stream=s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == names["prefix"], (what, longest, pb.last_kernel())
                assert symbol_ok is None or symbol_ok(pb.last_kernel_symbol()), (what, pb.last_kernel_symbol())
                assert (host(ln) == w).all(), (what, longest, "prefix")
                ln.view(torch.uint8).fill_(0xA5)
        if suffix:
            for longest in (True, False):
                w = want(("suffix", longest) + key, lambda: o.suffix(e.text, e.offs, longest, True, True))
                t.suffix_device(e.ptr, e.dev_offs.data_ptr(), n, longest, ln.data_ptr(), through_end=True, through_begin=True, stream=s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == "suffix", (what, longest, pb.last_kernel())
                assert (host(ln) == w).all(), (what, longest, "suffix")
                ln.view(torch.uint8).fill_(0xA5)


@gpu
@pytest.mark.parametrize("form", ["lane", "rows", "ragged"])
@pytest.mark.parametrize("name,blob", half_tables(), ids=[b[0] for b in half_tables()])
def test_prefix_suffix_and_half_final_across_4gib(big, cfg, name, blob, form):
    """pire_hip_prefix (prefix, ragged_prefix), pire_hip_suffix and pire_hip_run_half_final (half_final, half_final_rows,
    ragged_half_final).  The suffix kernel reads 16-byte blocks by absolute address, downwards from the string's end: with the
    text pointer 0, 1 and 15 bytes into a block, byte 2^32 of the text lies on a block's base, one byte above it and one
    byte below the next."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    if form == "ragged":
        cfg.set(ragged_act_always=1, counting_variant=1)
    else:
        cfg.set(no_ragged_act=1, counting_variant=2 if form == "rows" else 1)
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    o.tag = name
    t.upload()

    def names(n):
        if form == "ragged" and n >= 256:
            return {"prefix": "ragged_prefix", "half_final": "ragged_half_final"}
        return {"prefix": "prefix", "half_final": "half_final_rows" if form == "rows" else "half_final"}

    prefix_suffix_half_final(torch, pb, big, t, o, "abc", names, skews=(0, 1, 15) if form == "lane" else (0,), suffix=form == "lane")


@gpu
@pytest.mark.parametrize("zipv", [1, 2], ids=["plain rows", "zipped"])
def test_prefix_and_half_final_across_4gib_on_the_wide_walk(big, cfg, zipv):
    """ragged_prefix_wide and ragged_half_final_wide (dict_1k on the class-indexed walk)."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(walk_variant=2, zip_variant=zipv, ragged_act_always=1, auto_adapt=1, counting_variant=1)
    blob = W.load_blob(W.wide_set("dict_1k")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    o.tag = "dict_1k"
    prefix_suffix_half_final(torch, pb, big, t, o, "dict_1k", lambda n: {"prefix": "ragged_prefix_wide", "half_final": "ragged_half_final_wide"},
                             suffix=False, batches=("short508", "long900"), symbol_ok=lambda sym: ("zipped" in sym) == (zipv == 2))


@gpu
@pytest.mark.parametrize("kernel", ["ragged", "stream"])
def test_run_pair_across_4gib(big, cfg, kernel):
    """pire_hip_run_pair (two passes behind one call for offset batches): set_a and set_d on the same text, the passes on the
    ragged and on the stream kernel (batches of fewer than 256 strings: generic)."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_offsets_peek=1, ragged_variant=2 if kernel == "stream" else 1)
    b1, b2 = H.load_blob(big_set("set_a")["blob"]), H.load_blob(big_set("set_d")["blob"])
    t1, t2, o1, o2 = pire_amd.Table(b1), pire_amd.Table(b2), ob.OracleScanner(b1), ob.OracleScanner(b2)
    s = stream_of(torch)
    for what, strings, e in placements(big, "set_a"):
        n = e.n
        i1, i2, fin = poisoned(n, torch.int32), poisoned(n, torch.int32), poisoned(n, torch.uint8)
        for flags in (BE, 0):
            w1 = want(("pair1", flags) + what[:4], lambda: o1.run(e.text, e.offs, flags=flags))
            w2 = want(("pair2", flags) + what[:4], lambda: o2.run(e.text, e.offs, flags=flags))
            pb.run_pair_device(t1, t2, e.ptr, e.dev_offs.data_ptr(), n, flags, i1.data_ptr(), i2.data_ptr(), fin.data_ptr(), s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == (kernel if n >= 256 else "generic"), (what, pb.last_kernel())
            assert (host(i1).astype(np.uint32) == w1[0]).all() and (host(i2).astype(np.uint32) == w2[0]).all(), (what, flags)
            assert (host(fin) == (w1[1] | w2[1])).all(), (what, flags)
            i1.view(torch.uint8).fill_(0xA5), i2.view(torch.uint8).fill_(0xA5), fin.fill_(0xA5)


# ---- Part A: counting, capture, SlowScanner ------------------------------------------------------------------------------

def counting_kernel(t, kind, variant, generic):
    """counting.hip LaunchCounting's choice, from pire_hip_counting_table_forms."""
    f = t.forms()
    if generic or kind == 2 or not (f["packed_nreg"] or f["letter_rows_nreg"]):
        return "counting"
    if variant == 2 and f["byte_rows"]:
        return "counting_rows"
    if variant == 2 and f["letter_rows_nreg"]:
        return "counting_letter_rows"
    return "counting_packed" if f["packed_nreg"] else "counting"


def counting_tables():
    """The golden counting cases -- every one of them has at most 64 states, so the rows indexed by the byte are theirs and
    `counting_letter_rows` is out of their reach -- and, where the reference library is there to compile them, the 7-regexp
    scanners of tests/test_counting.py (143 and 573 states: rows indexed by the table's letters)."""
    out = [(c["name"], c["kind"], H.load_blob(c["blob"])) for c in H.golden()["counting"]]
    if ob.ref_available():
        res_ = ["[a-z]+", "http", "abc", "[0-9]+", "e", "th", "ing"]
        seps = ["\\s", ".*", ".*", "\\s", ".*", ".*", ".*"]
        out += [("seven_%d" % kind, kind, ob.RefCountingScanner.compile(kind, res_, seps).save()) for kind in (0, 1)]
    return out


@gpu
@pytest.mark.parametrize("order", [1, 0], ids=["by length", "caller's order"])
def test_counting_across_4gib(big, cfg, order):
    """pire_hip_counting_run: counting, counting_packed, counting_rows (and counting_letter_rows).  `by length`: batches of
    36 608 strings, which every one of these kernels takes in the order of their length classes (order.hip: from 32 768
    strings on; its histogram, scan and scatter read the offsets past 2^32, the kernels take string order[k] in a
    serpentine).  `caller's order`: the small batches, which are too few to be ordered, and the order switched off."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    s = stream_of(torch)
    reached = set()
    for name, kind, blob in counting_tables():
        t, o = pire_amd.CountingTable(blob, kind), ob.OracleCountingScanner(blob, kind)
        for variant, generic in ((1, False), (2, False), (1, True)):
            cfg.set(counting_variant=variant, no_length_order=0 if order else 1)
            kernel = counting_kernel(t, kind, variant, generic)
            if (variant, generic) != (1, False) and kernel == counting_kernel(t, kind, 1, False):
                continue
            reached.add(kernel)
            for what, strings, e in (large_placements if order else placements)(big, "count"):
                n = e.n
                assert (n >= ORDER_FROM) == bool(order)        # order.hip OrdersByLength, with no_length_order above
                idx, res = poisoned(n, torch.int32), poisoned((n, t.RegexpsCount), torch.int32)
                oi, orr = want(("count", name) + what[:4], lambda: o.run(e.text, e.offs, flags=BE))
                t.run_device(e.ptr, e.dev_offs.data_ptr(), n, BE | (pb.FLAG_GENERIC if generic else 0), idx.data_ptr(), res.data_ptr(), s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == kernel, (name, what, pb.last_kernel(), kernel)
                assert (host(idx).astype(np.uint32) == oi).all(), (name, kernel, what)
                assert (host(res).astype(np.uint32).astype(np.uint64) == orr).all(), (name, kernel, what)
    assert {"counting", "counting_packed", "counting_rows"} <= reached and ("counting_letter_rows" in reached) == ob.ref_available()


CAPTURE_FORMS = {      # form -> (configuration, PIRE_HIP_RUN_GENERIC)
    "capture": ({}, True),
    "capture_dense": ({"no_ragged_act": 1, "counting_variant": 1}, False),
    "capture_rows": ({"no_ragged_act": 1, "counting_variant": 2}, False),
    "ragged_capture": ({"ragged_act_always": 1}, False),
}


@gpu
@pytest.mark.parametrize("form", list(CAPTURE_FORMS))
@pytest.mark.parametrize("family", ["digits", "google"])
def test_capture_across_4gib(big, cfg, family, form):
    """pire_hip_capture_run through capture, capture_dense, capture_rows and ragged_capture (>= 256 strings; smaller batches
    keep the dense rows), and pire_hip_capture_select / pire_hip_capture_run_select behind it: the byte ranges are the
    oracle's plus what the offsets are ahead of the batch, so with offsets[0] = lead most of them exceed 2^32."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    knobs, generic = CAPTURE_FORMS[form]
    cfg.set(**knobs)
    blob = H.load_blob(golden_case("capturing", "capture_" + family)["blob"])
    t, o = pire_amd.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    assert t.Size <= 34 and t.LettersCount <= 127
    s = stream_of(torch)
    gen = pb.FLAG_GENERIC if generic else 0
    high = 0
    for what, strings, e in placements(big, family):
        n = e.n
        kernel = "capture_dense" if form == "ragged_capture" and n < 256 else form
        idx, fin, bg, en = poisoned(n, torch.int32), poisoned(n, torch.uint8), poisoned(n, torch.int64), poisoned(n, torch.int64)
        for flags in (BE, 0):
            wi, wf, wc, wb, we = want(("capture", family, flags) + what[:4], lambda: o.capture(e.text, e.offs, flags=flags))
            t.capture_device(e.ptr, e.dev_offs.data_ptr(), n, flags | gen, idx.data_ptr(), fin.data_ptr(), bg.data_ptr(), en.data_ptr(), s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == kernel, (what, flags, pb.last_kernel())
            assert (host(idx).astype(np.uint32) == wi).all() and (host(fin) == wf).all(), (what, flags)
            assert (host(bg) == wb).all() and (host(en) == we).all(), (what, flags)
            # the ranges, as include/pire_hip.h states them, from the oracle's positions
            b1 = flags & 1
            lens = np.diff(e.offs.astype(np.int64))
            sel = (wb >= 0) & (we >= 0)
            b = np.clip(wb - b1, 0, lens)
            en_ = np.minimum(np.maximum(we - b1, b), lens)
            at = e.host_offs[:-1].astype(np.int64)
            spans = np.stack([at + b, at + en_], axis=1)[sel]
            hits = np.nonzero(sel)[0]
            high += int((spans >= G4).sum())
            for fused in (False, True):
                oh, osp, cnt = poisoned(n, torch.int64), poisoned((n, 2), torch.int64), poisoned(1, torch.int64)
                if fused:
                    t.capture_select_device(e.ptr, e.dev_offs.data_ptr(), n, flags | gen, cnt.data_ptr(), out_hits_ptr=oh.data_ptr(),
                                            out_spans_ptr=osp.data_ptr(), hit_cap=n, stream=s)
                else:
                    pb.capture_select_device(e.dev_offs.data_ptr(), n, flags, bg.data_ptr(), en.data_ptr(), cnt.data_ptr(),
                                             out_hits_ptr=oh.data_ptr(), out_spans_ptr=osp.data_ptr(), hit_cap=n, stream=s)
                torch.cuda.synchronize()
                k = int(cnt[0])
                assert k == len(hits) and (host(oh)[:k] == hits).all() and (host(osp)[:k] == spans).all(), (what, flags, fused)
                assert (host(oh)[k:] == POISON64).all(), (what, flags, fused)
            idx.view(torch.uint8).fill_(0xA5), fin.fill_(0xA5), bg.view(torch.uint8).fill_(0xA5), en.view(torch.uint8).fill_(0xA5)
    assert high > 0


@gpu
@pytest.mark.parametrize("no_list", [0, 1], ids=["default", "no_list"])
@pytest.mark.parametrize("case", SLOW_FORMS, ids=lambda c: c["name"])
def test_slow_forms_across_4gib(big, cfg, case, no_list):
    """pire_hip_slow_run: every launch form of tests/test_slow_forms.py, its own strings laid across 2^32."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    blob = slow_blob(case)
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    cfg.set(slow_no_list=no_list)
    plan = t.plan(len(slow_strings(case)), True, 0)
    s = stream_of(torch)
    for where in H.ACROSS_WHERE:
        strings, lead = slow_placed(case, where)[:2]
        for shifted in (True, False):
            e = EmbeddedAt(big, strings, lead, shifted)
            for flags in (BE, ob.FLAG_BEGIN):
                of, obits = want(("slow", case["name"], where, flags), lambda: o.run(e.text, e.offs, flags=flags))
                out = SlowOut(e.n, t.words)
                t.run_device(e.ptr, e.dev_offs.data_ptr(), e.n, flags, *out.ptrs(), s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == plan["kernel"], (pb.last_kernel(), plan["kernel"])
                out.check(of, obits, (case["name"], where, shifted, flags))


# ---- Part A: batches large enough to be taken by length (order.hip) -----------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,blob", half_tables(), ids=[b[0] for b in half_tables()])
def test_half_final_rows_by_length_across_4gib(big, cfg, name, blob):
    """half_final_rows on 36 608 strings: LaunchHalfFinalRows orders them by length class first."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_ragged_act=1, counting_variant=2, no_length_order=0)
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    s = stream_of(torch)
    for what, strings, e in large_placements(big, "abc"):
        n = e.n
        assert n >= ORDER_FROM
        idx, fin, res = poisoned(n, torch.int32), poisoned(n, torch.uint8), poisoned((n, o.regexps), torch.int32)
        oi, of, orr = want(("half large", name) + what[:4], lambda: o.run_half_final(e.text, e.offs, flags=BE))
        t.run_half_final_device(e.ptr, e.dev_offs.data_ptr(), n, BE, idx.data_ptr(), fin.data_ptr(), res.data_ptr(), s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == "half_final_rows", (what, pb.last_kernel())
        same_states(idx, fin, oi, of, what)
        got = host(res).astype(np.uint32)
        assert (got == orr).all(), (what, np.nonzero((got != orr).any(axis=1))[0][:8])


@gpu
@pytest.mark.parametrize("form", ["capture_rows", "capture_dense"])
def test_capture_by_length_across_4gib(big, cfg, form):
    """capture_rows (which takes its strings by length) and capture_dense with capture_by_length, on 36 608 strings."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_ragged_act=1, no_length_order=0, counting_variant=2 if form == "capture_rows" else 1, capture_by_length=form == "capture_dense")
    blob = H.load_blob(golden_case("capturing", "capture_digits")["blob"])
    t, o = pire_amd.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s = stream_of(torch)
    for what, strings, e in large_placements(big, "digits"):
        n = e.n
        assert n >= ORDER_FROM
        idx, fin, bg, en = poisoned(n, torch.int32), poisoned(n, torch.uint8), poisoned(n, torch.int64), poisoned(n, torch.int64)
        wi, wf, wc, wb, we = want(("capture large",) + what[:4], lambda: o.capture(e.text, e.offs, flags=BE))
        t.capture_device(e.ptr, e.dev_offs.data_ptr(), n, BE, idx.data_ptr(), fin.data_ptr(), bg.data_ptr(), en.data_ptr(), s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == form, (what, pb.last_kernel())
        assert (host(idx).astype(np.uint32) == wi).all() and (host(fin) == wf).all(), what
        assert (host(bg) == wb).all() and (host(en) == we).all() and wc.sum() > 0, what


@gpu
def test_slow_list_by_length_across_4gib(big, cfg):
    """The SlowScanner list kernel on 36 608 strings: its plan says by_length, and does not with no_length_order."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    blob = H.load_blob(W.slow_case("slow_alt")["blob"])
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    s = stream_of(torch)
    for no_order in (0, 1):
        cfg.set(no_length_order=no_order, slow_no_list=0)
        for what, strings, e in large_placements(big, "abc"):
            plan = t.plan(e.n, True, 0)
            assert plan["kernel"] == "slow_list" and plan["by_length"] == (not no_order), plan
            for flags in (BE, ob.FLAG_BEGIN):
                of, obits = want(("slow large", flags) + what[:4], lambda: o.run(e.text, e.offs, flags=flags))
                out = SlowOut(e.n, t.words)
                t.run_device(e.ptr, e.dev_offs.data_ptr(), e.n, flags, *out.ptrs(), s)
                torch.cuda.synchronize()
                assert pb.last_kernel() == "slow_list", pb.last_kernel()
                out.check(of, obits, what + (flags, no_order))


# ---- Part A: the passes whose outputs are byte positions ------------------------------------------------------------------

@gpu
def test_fields_gather_and_gather_spans_across_4gib(big):
    """pire_hip_fields (spans = awk's, plus what the offsets are ahead of the batch), pire_hip_gather (sources above 2^32,
    any order, a tail byte) and pire_hip_gather_spans (the fields' spans into the raw buffer, size above 2^32)."""
    import torch
    from pire_amd import binding as pb

    s = stream_of(torch)
    high = 0
    for what, strings, e in placements(big, "tsv"):
        n = e.n
        total = int(e.offs[-1])
        for field, rest in ((0, False), (1, False), (1, True), (3, False)):
            w = want(("fields", field, rest) + what[:4], lambda: fields_of(strings, field, 9, rest)) + e.shift
            high += int((w >= G4).sum())
            spans = poisoned((n + 4, 2), torch.int64)
            pb.fields_device(e.ptr, e.dev_offs.data_ptr(), n, field, spans.data_ptr(), sep=9, rest=rest, stream=s)
            torch.cuda.synchronize()
            got = host(spans)
            assert (got[:n] == w).all(), (what, field, rest, np.nonzero((got[:n] != w).any(axis=1))[0][:8])
            assert (got[n:] == POISON64).all()
            # ... and the bytes of those columns, through their spans into the buffer the offsets index
            cols = [strings[i][int(b - e.shift - int(e.offs[i])):int(en - e.shift - int(e.offs[i]))] for i, (b, en) in enumerate(w.tolist())]
            for tail in (None, 10):
                a = 0 if tail is None else 1
                wt = b"".join(c + (b"" if tail is None else bytes([tail])) for c in cols)
                wo = np.concatenate([[0], np.cumsum([len(c) + a for c in cols])])
                out, oo, ob_ = poisoned(len(wt) + 64, torch.uint8), poisoned(n + 5, torch.int64), poisoned(1, torch.int64)
                pb.gather_spans_device(e.ptr, e.shift + total, spans.data_ptr(), ob_.data_ptr(), span_cap=n, tail=tail,
                                       out_text_ptr=out.data_ptr(), text_cap=len(wt), out_offsets_ptr=oo.data_ptr(), stream=s)
                torch.cuda.synchronize()
                assert int(ob_[0]) == len(wt) and host(out)[:len(wt)].tobytes() == wt, (what, field, rest, tail)
                assert (host(out)[len(wt):] == 0xA5).all() and (host(oo)[:n + 1] == wo).all(), (what, field, rest, tail)
        # the strings themselves: all of them in order, and every third one from the back, with and without a tail
        for pick in (None, np.arange(n - 1, -1, -3, dtype=np.int64)):
            src = list(range(n)) if pick is None else pick.tolist()
            didx = None if pick is None else torch.as_tensor(pick, device="cuda")
            for tail in (None, 10):
                a = 0 if tail is None else 1
                wt = b"".join(strings[i] + (b"" if tail is None else bytes([tail])) for i in src)
                wo = np.concatenate([[0], np.cumsum([len(strings[i]) + a for i in src])])
                out, oo, ob_ = poisoned(len(wt) + 64, torch.uint8), poisoned(len(src) + 5, torch.int64), poisoned(1, torch.int64)
                pb.gather_device(e.ptr, e.dev_offs.data_ptr(), n, ob_.data_ptr(), idx_ptr=0 if didx is None else didx.data_ptr(),
                                 idx_cap=len(src), tail=tail, out_text_ptr=out.data_ptr(), text_cap=len(wt), out_offsets_ptr=oo.data_ptr(), stream=s)
                torch.cuda.synchronize()
                assert int(ob_[0]) == len(wt) and host(out)[:len(wt)].tobytes() == wt, (what, pick is None, tail)
                assert (host(out)[len(wt):] == 0xA5).all() and (host(oo)[:len(src) + 1] == wo).all(), (what, pick is None, tail)
    assert high > 0


@gpu
@pytest.mark.parametrize("kernel", ["ragged", "stream"])
def test_run_select_and_run_route_across_4gib(big, cfg, kernel):
    """pire_hip_run_select and pire_hip_run_route: the scan and the pass behind it on the high batch (set_a)."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    cfg.set(no_offsets_peek=1, ragged_variant=2 if kernel == "stream" else 1)
    blob = H.load_blob(big_set("set_a")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    o.tag = "set_a"
    assert t.mask_words == 1
    R = o.regexps
    s = stream_of(torch)
    for what, strings, e in placements(big, "set_a"):
        n = e.n
        oi, of = want(("run", o.tag) + what[:4] + (BE,), lambda: o.run(e.text, e.offs, flags=BE))
        masks, fin = want(("masks",) + what[:4], lambda: masks_of(o, oi))
        for wanted in (None, [0, 5]):
            sel = fin if wanted is None else (masks & np.uint64(sum(1 << r for r in wanted))) != 0
            hits = np.nonzero(sel)[0]
            om, oh, ohm, cnt = (poisoned(n + 3, torch.int64) for _ in range(4))
            wm = t.want_mask(wanted)
            dw = None if wm is None else torch.as_tensor(wm.view(np.int64), device="cuda")
            t.run_select_device(e.ptr, e.dev_offs.data_ptr(), n, BE, cnt.data_ptr(), want_ptr=0 if dw is None else dw.data_ptr(),
                                out_masks_ptr=om.data_ptr(), out_hits_ptr=oh.data_ptr(), out_hit_masks_ptr=ohm.data_ptr(), hit_cap=n, stream=s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == (kernel if n >= 256 else "generic"), (what, pb.last_kernel())
            k = int(cnt[0])
            assert k == len(hits) and (host(oh)[:k] == hits).all() and (host(oh)[k:] == POISON64).all(), (what, wanted)
            assert (host(om)[:n].view(np.uint64) == masks).all() and (host(ohm)[:k].view(np.uint64) == masks[sel]).all(), (what, wanted)
        rows = [np.nonzero((masks >> np.uint64(r)) & np.uint64(1))[0] for r in range(R)]
        oh, cnts = poisoned((R, n), torch.int64), poisoned(R, torch.int64)
        t.run_route_device(e.ptr, e.dev_offs.data_ptr(), n, BE, cnts.data_ptr(), out_hits_ptr=oh.data_ptr(), hit_cap=n, stream=s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == (kernel if n >= 256 else "generic"), (what, pb.last_kernel())
        assert host(cnts).tolist() == [len(r) for r in rows], what
        for r in range(R):
            assert (host(oh)[r, :len(rows[r])] == rows[r]).all() and (host(oh)[r, len(rows[r]):] == POISON64).all(), (what, r)


# ---- Part B: the whole span ----------------------------------------------------------------------------------------------

def repeated(torch, block, step, count=K, last=None):
    """int64[count * len(block) (+ 1)] on the device: block + k * step for k < count, then `last`."""
    b = torch.as_tensor(np.asarray(block).astype(np.int64), device="cuda")
    out = (b[None, :] + torch.arange(count, device="cuda", dtype=torch.int64)[:, None] * step).reshape(-1)
    return out if last is None else torch.cat([out, torch.tensor([last], device="cuda", dtype=torch.int64)])


def rows_equal(torch, buf, block, count=K):
    """buf[:count * len(block)] is `block` count times (row by row: nothing of 4 GiB is made for the comparison)."""
    rows = buf[:count * block.numel()].view(count, block.numel())
    return all(torch.equal(rows[k], block) for k in range(count))


@gpu
@pytest.mark.parametrize("variant", [0, 1], ids=["default", "ragged_variant=1"])
def test_run_over_more_than_4gib_of_short_strings(big, cfg, variant):
    """pire_hip_run, offsets on the device, 1.7 million lines of 1 .. 4 KiB in 2^32 + 2^24 bytes less their newlines: the
    router itself takes the stream kernel (n >= 2^20), whose cost key and last tasks lie past 2^32; ragged_variant = 1 the
    ragged kernel.  The text is the period's lines without their newlines (what getline makes of it), laid 257 times into
    the module's buffer."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    per = period()
    cfg.set(ragged_variant=variant)
    blob = H.load_blob(big_set("set_a")["blob"])
    t = pire_amd.Table(blob)
    n, pt = per.lines * K, per.text.size
    try:
        block = torch.as_tensor(per.text, device="cuda")
        big[:K * pt].view(K, pt).copy_(block.expand(K, pt))
        big[K * pt:].fill_(0xA5)
        offs = repeated(torch, per.offs[:-1], pt, last=K * pt)
        assert offs.numel() == n + 1 and n >= 1 << 20 and K * pt > G4
        idx, fin = poisoned(n, torch.int32), poisoned(n, torch.uint8)
        cnt = torch.zeros(per.o.regexps + 2, dtype=torch.int64, device="cuda")
        t.run_device(big.data_ptr(), offs.data_ptr(), n, BE, idx.data_ptr(), fin.data_ptr(), cnt.data_ptr(), 0, stream_of(torch))
        torch.cuda.synchronize()
        assert pb.last_kernel() == ("ragged" if variant else "stream"), pb.last_kernel()
        wi = torch.as_tensor(per.idx.astype(np.int32), device="cuda")
        wf = torch.as_tensor(per.final.astype(np.uint8), device="cuda")
        bad = torch.nonzero((idx.view(K, -1) != wi[None, :]) | (fin.view(K, -1) != wf[None, :]))
        assert bad.numel() == 0, (bad.shape[0], bad[:8].tolist())
        assert int(cnt[1]) == n and int(cnt[0]) == K * int(per.final.sum())
    finally:
        big.fill_(0xA5)           # as the other tests of the module found it
        torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("with_text", [True, False], ids=["out_text", "offsets into raw"])
def test_split_over_more_than_4gib(periodic, with_text):
    """pire_hip_split on size = 2^32 + 2^24: the line count, every offset (those of the last period exceed 2^32 in both forms)
    and, with out_text, the copied bytes."""
    import torch
    from pire_amd import binding as pb

    per = period()
    n, pt = per.lines * K, per.text.size
    out = device_bytes(torch, BIG_BYTES) if with_text else None
    try:
        if out is not None:
            out.fill_(0xA5)
        offs, cnt = poisoned(n + 1 + 8, torch.int64), poisoned(1, torch.int64)
        pb.split_device(periodic.data_ptr(), K * P, cnt.data_ptr(), out_text_ptr=0 if out is None else out.data_ptr(),
                        out_offsets_ptr=offs.data_ptr(), offsets_cap=n + 4, stream=stream_of(torch))
        torch.cuda.synchronize()
        assert int(cnt[0]) == n
        w = repeated(torch, per.offs[:-1], pt, last=K * pt) if with_text else repeated(torch, per.keep[:-1], P, last=K * P)
        assert int(w[-1]) > G4 and torch.equal(offs[:n + 1], w)
        assert bool((offs[n + 1:] == POISON64).all())
        if out is not None:
            assert rows_equal(torch, out, torch.as_tensor(per.text, device="cuda"))
            assert bool((out[K * pt:] == 0xA5).all())
    finally:
        del out
        torch.cuda.empty_cache()


@gpu
def test_run_lines_select_gather_and_field_select_over_more_than_4gib(periodic):
    """pire_hip_run_lines_select, pire_hip_run_lines_gather and pire_hip_run_lines_field_select on size = 2^32 + 2^24: the line
    count, the hit indices, the byte ranges (offsets[i] + i, the last period's above 2^32) and the gathered bytes."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    per = period()
    t = pire_amd.Table(H.load_blob(big_set("set_a")["blob"]))
    n = per.lines * K
    s = stream_of(torch)
    for column in (False, True):
        fin = per.field_final if column else per.final
        hits = np.nonzero(fin)[0]
        cap = len(hits) * K + 5
        spans = np.stack([per.keep[:-1][fin], per.keep[1:][fin] - np.uint64(1)], axis=1).astype(np.int64)
        oh, osp, cnt = poisoned(cap, torch.int64), poisoned((cap, 2), torch.int64), poisoned(2, torch.int64)
        if column:
            t.run_lines_field_select_device(periodic.data_ptr(), K * P, 1, BE, cnt.data_ptr(), cnt.data_ptr() + 8, sep=9,
                                            out_hits_ptr=oh.data_ptr(), out_hit_spans_ptr=osp.data_ptr(), hit_cap=cap, stream=s)
        else:
            t.run_lines_select_device(periodic.data_ptr(), K * P, BE, cnt.data_ptr(), cnt.data_ptr() + 8, out_hits_ptr=oh.data_ptr(),
                                      out_hit_spans_ptr=osp.data_ptr(), hit_cap=cap, stream=s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == "stream", pb.last_kernel()
        assert host(cnt).tolist() == [n, len(hits) * K], (column, host(cnt).tolist())
        k = len(hits) * K
        assert torch.equal(oh[:k], repeated(torch, hits, per.lines)) and bool((oh[k:] == POISON64).all()), column
        assert torch.equal(osp[:k].reshape(-1), repeated(torch, spans.reshape(-1), P)) and bool((osp[k:] == POISON64).all()), column
        assert int(osp[k - 1, 1]) > G4
    # grep's output: the matching lines and their newlines, back to back
    fin = per.final
    hits = np.nonzero(fin)[0]
    k = len(hits) * K
    lines = [per.raw[int(per.keep[i]):int(per.keep[i + 1])] for i in hits.tolist()]
    block = np.concatenate(lines)
    wo = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
    room = block.size * K
    out = device_bytes(torch, room + 64)
    try:
        out.fill_(0xA5)
        oo, cnt = poisoned(k + 1 + 4, torch.int64), poisoned(3, torch.int64)
        t.run_lines_gather_device(periodic.data_ptr(), K * P, BE, cnt.data_ptr(), cnt.data_ptr() + 8, cnt.data_ptr() + 16,
                                  hit_cap=k, out_text_ptr=out.data_ptr(), text_cap=room, out_offsets_ptr=oo.data_ptr(), stream=s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == "stream", pb.last_kernel()
        assert host(cnt).tolist() == [n, k, room]
        assert torch.equal(oo[:k + 1], repeated(torch, wo[:-1], block.size, last=room)) and bool((oo[k + 1:] == POISON64).all())
        assert rows_equal(torch, out, torch.as_tensor(block, device="cuda")) and bool((out[room:] == 0xA5).all())
    finally:
        del out
        torch.cuda.empty_cache()


@gpu
def test_gather_and_fields_over_more_than_4gib(periodic):
    """pire_hip_fields over the whole batch (the lines with their newlines, as pire_hip_split's out_text == NULL form hands
    them over) and pire_hip_gather of every string with a tail byte: out_text and out_offsets pass 2^32, and with the
    newline removed by the offsets and put back as the tail the output must be the raw buffer again."""
    import torch
    from pire_amd import binding as pb

    per = period()
    n = per.lines * K
    s = stream_of(torch)
    keep = repeated(torch, per.keep[:-1], P, last=K * P)
    spans = poisoned((n + 2, 2), torch.int64)
    pb.fields_device(periodic.data_ptr(), keep.data_ptr(), n, 1, spans.data_ptr(), sep=9, stream=s)
    torch.cuda.synchronize()
    # second column of line i: behind its separator (a third of the way in), up to the end of the string -- the newline is
    # the string's last byte in this form
    w = np.stack([per.keep[:-1].astype(np.int64) + per.lens // 3 + 1, per.keep[1:].astype(np.int64)], axis=1)
    assert torch.equal(spans[:n].reshape(-1), repeated(torch, w.reshape(-1), P)) and int(spans[n - 1, 1]) == K * P
    assert bool((spans[n:] == POISON64).all())
    # the lines without their newlines (offsets of the split's out_text form into a buffer that holds them back to back)
    pt = per.text.size
    text = device_bytes(torch, BIG_BYTES, more=BIG_BYTES)
    out = device_bytes(torch, BIG_BYTES)
    try:
        block = torch.as_tensor(per.text, device="cuda")
        text[:K * pt].view(K, pt).copy_(block.expand(K, pt))
        out.fill_(0xA5)
        offs = repeated(torch, per.offs[:-1], pt, last=K * pt)
        oo, total = poisoned(n + 1 + 4, torch.int64), poisoned(1, torch.int64)
        pb.gather_device(text.data_ptr(), offs.data_ptr(), n, total.data_ptr(), idx_cap=n, tail=10, out_text_ptr=out.data_ptr(),
                         text_cap=K * P, out_offsets_ptr=oo.data_ptr(), stream=s)
        torch.cuda.synchronize()
        assert int(total[0]) == K * P
        assert torch.equal(oo[:n + 1], keep) and bool((oo[n + 1:] == POISON64).all())
        assert all(torch.equal(out[k * P:(k + 1) * P], periodic[k * P:(k + 1) * P]) for k in range(K))
        assert bool((out[K * P:] == 0xA5).all())
    finally:
        del text, out
        torch.cuda.empty_cache()


STRIDE, LENGTH = 4096 + 16, 4096
RECORDS = 64 * 16330          # 1 045 120 records of 4 112 bytes: n * stride = 2^32 + 2 566 144


def strided_period(entry_name, dictionary):
    """Part B's fixed-length records: one period of 1024 records of LENGTH bytes in STRIDE (padding 0xFF), repeated."""
    def make():
        rec = np.full((1024, STRIDE), 0xFF, dtype=np.uint8)
        if dictionary:
            rec[:, :LENGTH] = W.wide_records(W.wide_set(entry_name), "k512", 9, 1024, LENGTH)
            words = W.dictionary_words(W.wide_set(entry_name))       # a whole word in every third record: Final for good behind it
            for i in range(0, 1024, 3):
                w = np.frombuffer(words[(11 + i) % len(words)], dtype=np.uint8)
                rec[i, 2000 + i:2000 + i + len(w)] = w
        else:
            entry = big_set(entry_name)
            rec[:, :LENGTH] = ob.corpus_fill(17, 0, 1024, LENGTH, H.plants_for(entry), threads=4)
        return rec
    return want(("strided period", entry_name), make)


@functools.lru_cache(maxsize=None)
def strided_expectations():
    """The oracle's answers on one period of the fixed-length records: set_a and set_d (the pair), the SlowScanner slow_alt, and
    dict_1k on its own corpus; "shares": the share of Final records of each."""
    offs = np.arange(1025, dtype=np.uint64) * LENGTH
    text = np.ascontiguousarray(strided_period("set_a", False)[:, :LENGTH]).reshape(-1)
    out = {}
    for name in ("set_a", "set_d"):
        out[name] = ob.OracleScanner(H.load_blob(big_set(name)["blob"])).run(text, offs, threads=4)
    out["slow_alt"] = ob.OracleSlowScanner(H.load_blob(W.slow_case("slow_alt")["blob"])).run(text, offs)
    wide = np.ascontiguousarray(strided_period("dict_1k", True)[:, :LENGTH]).reshape(-1)
    out["dict_1k"] = ob.OracleScanner(W.load_blob(W.wide_set("dict_1k")["blob"])).run(wide, offs, threads=4)
    out["shares"] = {"set_a": float(out["set_a"][1].mean()), "set_d": float(out["set_d"][1].mean()),
                     "slow_alt": float(out["slow_alt"][0].mean()), "dict_1k": float(out["dict_1k"][1].mean())}
    return out


def lay_records(torch, big, rec, n):
    per = rec.shape[0]
    block = torch.as_tensor(rec.reshape(-1), device="cuda")
    full = n // per
    big[:full * block.numel()].view(full, block.numel()).copy_(block.expand(full, block.numel()))
    rest = (n - full * per) * STRIDE
    big[full * block.numel():full * block.numel() + rest].copy_(block[:rest])
    big[n * STRIDE:n * STRIDE + (1 << 20)].fill_(0xA5)


def check_periodic(torch, got, block, n, what):
    """got[i] == block[i % len(block)] for i < n, on the device."""
    w = torch.as_tensor(block, device="cuda")
    per = w.numel()
    full = n // per
    bad = torch.nonzero(got[:full * per].view(full, per) != w[None, :])
    assert bad.numel() == 0, (what, bad.shape[0], bad[:8].tolist())
    assert torch.equal(got[full * per:n], w[:n - full * per]), (what, "the last period")


@gpu
def test_strided_records_over_more_than_4gib(big, cfg):
    """pire_hip_run_strided with n * stride > 2^32 (stride 4096 + 16, len 4096) through tiled, wide (walk_variant 2 and 3), a
    record count that leaves a remainder for the generic kernel (its text pointer lies past 2^32), pire_hip_run_pair_strided
    and pire_hip_slow_run_strided."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    s = stream_of(torch)
    assert RECORDS * STRIDE > G4 and (RECORDS + 37) * STRIDE + (1 << 20) <= BIG_BYTES
    try:
        # set_a: tiled, and tiled + the generic kernel on the remainder; the pair kernel with set_d
        rec = strided_period("set_a", False)
        lay_records(torch, big, rec, RECORDS + 37)
        exp = strided_expectations()
        b1, b2 = H.load_blob(big_set("set_a")["blob"]), H.load_blob(big_set("set_d")["blob"])
        t1, t2, o1 = pire_amd.Table(b1), pire_amd.Table(b2), ob.OracleScanner(b1)
        w1, w2 = exp["set_a"], exp["set_d"]
        # (RECORDS + 37: the 37 records behind the last task of 64 go through the generic kernel, LaunchRemainder, whose text
        # pointer then lies past 2^32; pire_hip_last_kernel() keeps naming the kernel that took the tasks)
        for n in (RECORDS, RECORDS + 37):
            idx, fin = poisoned(n + 8, torch.int32), poisoned(n + 8, torch.uint8)
            cnt = torch.zeros(o1.regexps + 2, dtype=torch.int64, device="cuda")
            t1.run_strided_device(big.data_ptr(), n, LENGTH, STRIDE, BE, idx.data_ptr(), fin.data_ptr(), cnt.data_ptr(), 0, s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == "tiled", pb.last_kernel()
            check_periodic(torch, idx, w1[0].astype(np.int32), n, ("idx", n))
            check_periodic(torch, fin, w1[1], n, ("final", n))
            assert bool((fin[n:] == 0xA5).all()) and int(cnt[1]) == n
        n = RECORDS
        i1, i2, fin = poisoned(n, torch.int32), poisoned(n, torch.int32), poisoned(n, torch.uint8)
        pb.run_pair_strided_device(t1, t2, big.data_ptr(), n, LENGTH, STRIDE, BE, i1.data_ptr(), i2.data_ptr(), fin.data_ptr(), s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == "pair_tiled", pb.last_kernel()
        check_periodic(torch, i1, w1[0].astype(np.int32), n, "pair 1")
        check_periodic(torch, i2, w2[0].astype(np.int32), n, "pair 2")
        check_periodic(torch, fin, w1[1] | w2[1], n, "pair final")
        # a SlowScanner on the same records
        case = W.slow_case("slow_alt")
        sblob = H.load_blob(case["blob"])
        st = pire_amd.SlowTable(sblob)
        sf, sbits = exp["slow_alt"]
        out_f, out_b = poisoned(n, torch.uint8), poisoned((n, st.words), torch.int32)
        st.run_strided_device(big.data_ptr(), n, LENGTH, STRIDE, BE, out_f.data_ptr(), out_b.data_ptr(), 0, s)
        torch.cuda.synchronize()
        assert pb.last_kernel() == st.plan(n, False, 0)["kernel"], pb.last_kernel()
        check_periodic(torch, out_f, sf, n, "slow final")
        check_periodic(torch, out_b.reshape(-1), sbits.view(np.int32).reshape(-1), n * st.words, "slow bits")
        # the dictionary scanner: the class-indexed walk, one and two strings per lane
        rec = strided_period("dict_1k", True)
        lay_records(torch, big, rec, RECORDS)
        blob = W.load_blob(W.wide_set("dict_1k")["blob"])
        wi, wf = exp["dict_1k"]
        for walk in (2, 3):
            cfg.set(walk_variant=walk)
            t = pire_amd.Table(blob)
            idx, fin = poisoned(n, torch.int32), poisoned(n, torch.uint8)
            t.run_strided_device(big.data_ptr(), n, LENGTH, STRIDE, BE, idx.data_ptr(), fin.data_ptr(), 0, 0, s)
            torch.cuda.synchronize()
            assert pb.last_kernel() == "wide" and ("ScanWide2Kernel" if walk == 3 else "ScanWideKernel<") in pb.last_kernel_symbol(), \
                (pb.last_kernel(), pb.last_kernel_symbol())
            check_periodic(torch, idx, wi.astype(np.int32), n, ("wide idx", walk))
            check_periodic(torch, fin, wf, n, ("wide final", walk))
    finally:
        big.fill_(0xA5)           # as the other tests of the module found it
        torch.cuda.synchronize()


@gpu
def test_one_string_of_more_than_4gib_through_the_segmented_scan(periodic, cfg):
    """One string of 2^32 + 2^24 + 5 bytes, offsets on the host, segment_bytes set.  Expected: the oracle's state map of one
    period, composed 257 times from the state behind Begin and memoised per start state, then the five bytes of the tail and
    End.  The identical call on the string's first 64 MiB comes first and must take the segmented scan."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    per = period()
    o = per.o
    blob = H.load_blob(big_set("set_a")["blob"])
    t = pire_amd.Table(blob)
    cfg.set(segment_bytes=1 << 20)
    tail = np.frombuffer(b"hello", dtype=np.uint8)
    s = stream_of(torch)

    def expected(periods):
        st = int(o.run(per.raw, np.array([0, P], dtype=np.uint64), flags=ob.FLAG_BEGIN)[0][0])
        for _ in range(periods - 1):
            st = per.state_map(st)
        i, f = o.run(tail, np.array([0, 5], dtype=np.uint64), flags=ob.FLAG_END, init_idx=[st])
        return int(i[0]), int(f[0])

    assert expected(1) == tuple(int(x[0]) for x in o.run(np.concatenate([per.raw, tail]), np.array([0, P + 5], dtype=np.uint64)))
    try:
        for periods in (4, K):
            size = periods * P
            saved = periodic[size:size + 5].clone()
            periodic[size:size + 5].copy_(torch.as_tensor(tail))
            idx, fin = poisoned(1, torch.int32), poisoned(1, torch.uint8)
            t.run_device_host_offsets(periodic.data_ptr(), np.array([0, size + 5], dtype=np.uint64), BE, idx.data_ptr(), fin.data_ptr(), 0, 0, s)
            torch.cuda.synchronize()
            periodic[size:size + 5].copy_(saved)
            assert pb.last_kernel().startswith("segmented"), (periods, pb.last_kernel())
            assert (int(idx[0]), int(fin[0])) == expected(periods), (periods, int(idx[0]), int(fin[0]), expected(periods))
    finally:
        torch.cuda.synchronize()
