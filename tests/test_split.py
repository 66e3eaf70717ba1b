"""pire_hip_split / pire_hip_run_lines_select: raw bytes cut into lines on the device (split.hip), and the matching lines
of a raw buffer in one call.

Exact equality everywhere.  The expected values come from `restate` -- getline's semantics written down with
np.flatnonzero -- and, for the scan, from the C oracle on the lines `restate` produces; masks and Final from the host
accessors Table.AcceptedRegexps / Table.Final.  Nothing expected comes from the library."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = pb.SPLIT_TILE
BE = pb.FLAG_BEGIN | pb.FLAG_END
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8
gpu = pytest.mark.gpu


# ---- the restatement ---------------------------------------------------------------------------------------------------

def restate(raw, delim=10, keep=False):
    """(text, offsets, n) as include/pire_hip.h states them; keep: the out_text == NULL form (offsets into raw itself)."""
    raw = np.asarray(raw, dtype=np.uint8)
    p = np.flatnonzero(raw == delim).astype(np.uint64)
    d, size = len(p), len(raw)
    n = d + (1 if size and raw[-1] != delim else 0)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:d + 1] = p + np.uint64(1) if keep else p - np.arange(d, dtype=np.uint64)
    offs[n] = size if keep else size - d
    return raw[raw != delim], offs, n


def lines_of(raw, delim=10):
    text, offs, n = restate(raw, delim)
    return [text[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


# ---- CPU -----------------------------------------------------------------------------------------------------------------

HAND_WRITTEN = [b"", b"\n", b"a", b"a\n", b"a\nb", b"a\nb\n", b"\n\n", b"\na", b"a\n\n\nb", b"\n\n\n", b"ab\r\ncd\r\n", b"abc\n\nde\nf",
                b"no newline at all", b"\nx\n\ny\n\n"]


def test_restatement_agrees_with_bytes_split_on_hand_written_cases():
    for raw in HAND_WRITTEN:
        want = raw.split(b"\n")
        if want[-1] == b"":          # a buffer that ends in a delimiter (or is empty) has no extra empty string behind it
            want.pop()
        assert lines_of(u8(raw)) == want, raw
        text, offs, n = restate(u8(raw))
        assert n == len(want) and text.tobytes() == raw.replace(b"\n", b"") and int(offs[0]) == 0 and int(offs[-1]) == len(text)
        # the consequence the header documents: line i is raw[offsets[i] + i, offsets[i + 1] + i)
        assert [raw[int(offs[i]) + i:int(offs[i + 1]) + i] for i in range(n)] == want
        _, keep, kn = restate(u8(raw), keep=True)
        assert kn == n and [raw[int(keep[i]):int(keep[i + 1])].rstrip(b"\n") for i in range(n)] == want
        assert all(raw[int(keep[i]):int(keep[i + 1])].endswith(b"\n") for i in range(n - 1))
    assert lines_of(u8(b"a\x00b\x00"), 0) == [b"a", b"b"] and lines_of(u8(b"\xffa\xff\xffb"), 255) == [b"", b"a", b"", b"b"]


def test_the_library_exports_the_split_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    for name in ("pire_hip_split", "pire_hip_run_lines_select"):
        assert hasattr(L, name), name
        assert name in {n for n, _, _ in pb.ABI}
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        assert int(re.search(r"#define PIRE_HIP_SPLIT_TILE_BYTES (\d+)u", f.read()).group(1)) == T == 16384


def test_split_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    raw = np.frombuffer(b"ab\ncd\nef" * 4, dtype=np.uint8).copy()
    text = np.zeros(64, dtype=np.uint8)
    offs = np.zeros(16, dtype=np.uint64)
    n = C.c_uint64(77)
    r, nn = raw.ctypes.data, C.addressof(n)
    cases = {
        "delim > 255": (r, raw.size, 256, text.ctypes.data, offs.ctypes.data, 8, nn),
        "null out_n": (r, raw.size, 10, text.ctypes.data, offs.ctypes.data, 8, None),
        "size > 0 with null raw": (None, raw.size, 10, text.ctypes.data, offs.ctypes.data, 8, nn),
        "offsets_cap > 0 with null out_offsets": (r, raw.size, 10, text.ctypes.data, None, 8, nn),
        "overlaps raw": (r, raw.size, 10, r + raw.size - 1, offs.ctypes.data, 8, nn),
    }
    for what, (a_raw, size, delim, a_text, a_offs, cap, a_n) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_split(a_raw, size, delim, flags, a_text, a_offs, cap, a_n, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    # the overlap is a matter of the two pointers and the size alone (addresses nobody owns: the call must not touch them) ...
    for a_raw, a_text in ((0x7000000000, 0x7000000000), (0x7000000000, 0x7000000000 + 4095), (0x7000000000 + 4095, 0x7000000000)):
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_split(a_raw, 4096, 10, flags, a_text, None, 0, nn, None) == -1
            assert "overlaps raw" in L.pire_hip_last_error().decode()
    assert n.value == 77 and not text.any() and not offs.any()
    # ... and an empty buffer is answered without a device: no strings, offsets[0] = 0
    offs[:] = 5
    assert L.pire_hip_split(None, 0, 10, 0, text.ctypes.data, offs.ctypes.data, 8, nn, None) == 0
    assert n.value == 0 and offs.tolist() == [0] + [5] * 15
    t, o, k = pb.split_host(b"")
    assert (t.size, o.tolist(), k) == (0, [0], 0)


def test_run_lines_select_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    t = pb.Table(H.load_blob("c2_single.blob"))
    raw = np.frombuffer(b"hello  world\nabc\n", dtype=np.uint8).copy()
    hits, spans, masks = np.zeros(4, np.uint64), np.zeros(8, np.uint64), np.zeros(4, np.uint64)
    lines, cnt = C.c_uint64(77), C.c_uint64(78)
    r, lp, cp = raw.ctypes.data, C.addressof(lines), C.addressof(cnt)
    h, s, m = hits.ctypes.data, spans.ctypes.data, masks.ctypes.data
    cases = {
        "null table": (None, r, raw.size, 10, None, lp, h, s, m, 4, cp),
        "delim > 255": (t._h, r, raw.size, 300, None, lp, h, s, m, 4, cp),
        "null out_line_count": (t._h, r, raw.size, 10, None, None, h, s, m, 4, cp),
        "size > 0 with null raw": (t._h, None, raw.size, 10, None, lp, h, s, m, 4, cp),
        "null out_hit_count": (t._h, r, raw.size, 10, None, lp, h, s, m, 4, None),
        "hit_cap > 0 with null out_hits": (t._h, r, raw.size, 10, None, lp, None, None, None, 4, cp),
        "out_hit_masks without out_hits": (t._h, r, raw.size, 10, None, lp, None, None, m, 0, cp),
        "out_hit_spans without out_hits": (t._h, r, raw.size, 10, None, lp, None, s, None, 0, cp),
    }
    for what, (th, a_raw, size, delim, want, a_lines, a_h, a_s, a_m, cap, a_c) in cases.items():
        for flags in (BE, BE | pb.FLAG_ON_DEVICE):
            assert L.pire_hip_run_lines_select(th, a_raw, size, delim, flags, want, a_lines, a_h, a_s, a_m, cap, a_c, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    assert (lines.value, cnt.value) == (77, 78) and not hits.any() and not spans.any()
    assert L.pire_hip_run_lines_select(t._h, None, 0, 10, BE, None, lp, h, s, m, 4, cp, None) == 0
    assert (lines.value, cnt.value) == (0, 0)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_split_unit_passes_the_build_audit():
    """split.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "split.hip" in ba.NO_SCRATCH and "split.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        assert f.read().count("split.hip") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("split.hip")
    assert not fails, fails
    assert len(seen) == 5 and all("Split" in k for k in seen), seen


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class DevSplit:
    """One pire_hip_split call on device pointers.  raw sits `raw_off` bytes into an aligned allocation whose other bytes
    ARE the delimiter (a lane that reads past either end of the buffer counts them); out_text `text_off` bytes into a
    poisoned one; out_offsets has GUARD poisoned words behind entry `cap`.  After fetch(): text, offs, n -- and every byte
    the call had no business writing has been looked at."""

    def __init__(self, torch, raw, delim=10, raw_off=0, text_off=0, cap=None, keep=False, exp_n=None):
        self.torch = torch
        raw = np.asarray(raw, dtype=np.uint8)
        self.raw, self.size, self.delim, self.keep, self.text_off = raw, len(raw), delim, keep, text_off
        self.cap = (restate(raw, delim)[2] if exp_n is None else exp_n) if cap is None else cap
        host = np.full(raw_off + self.size + 256, delim, dtype=np.uint8)
        host[raw_off:raw_off + self.size] = raw
        self.host_in = host
        self.dev_in = torch.as_tensor(host, device="cuda")
        self.raw_ptr = self.dev_in.data_ptr() + raw_off
        assert self.dev_in.data_ptr() % 256 == 0
        self.text = None if keep else torch.full((text_off + self.size + 256,), POISON, dtype=torch.uint8, device="cuda")
        self.offs = torch.full((self.cap + 1 + GUARD,), int(np.uint64(POISON64).astype(np.int64)), dtype=torch.int64, device="cuda")
        self.n = torch.full((1,), int(np.uint64(POISON64).astype(np.int64)), dtype=torch.int64, device="cuda")
        assert self.text is None or self.text.data_ptr() % 256 == 0

    def run(self):
        pb.split_device(self.raw_ptr if self.size else 0, self.size, self.n.data_ptr(), self.delim,
                        0 if self.text is None else self.text.data_ptr() + self.text_off, self.offs.data_ptr(), self.cap,
                        self.torch.cuda.current_stream().cuda_stream)
        return self

    def fetch(self):
        self.torch.cuda.synchronize()
        assert (self.dev_in.cpu().numpy() == self.host_in).all(), "the input was written to"
        n = int(self.n.cpu().numpy().view(np.uint64)[0])
        offs = self.offs.cpu().numpy().view(np.uint64)
        k = min(n, self.cap)
        assert (offs[k + 1:] == np.uint64(POISON64)).all(), "out_offsets written behind entry min(n, offsets_cap)"
        text = None
        if self.text is not None:
            buf = self.text.cpu().numpy()
            length = self.size - int((self.raw == self.delim).sum())
            assert (buf[:self.text_off] == POISON).all() and (buf[self.text_off + length:] == POISON).all(), "bytes around out_text written"
            text = buf[self.text_off:self.text_off + length]
        return text, offs[:k + 1], n

    def everything(self):
        """Every output buffer, whole (for bit-identity of two calls)."""
        self.torch.cuda.synchronize()
        return [b.cpu().numpy().tobytes() for b in (self.text, self.offs, self.n) if b is not None]


def check_split(torch, raw, delim=10, **kw):
    raw = np.asarray(raw, dtype=np.uint8)
    et, eo, en = restate(raw, delim, keep=kw.get("keep", False))
    text, offs, n = DevSplit(torch, raw, delim, exp_n=en, **kw).run().fetch()
    assert n == en
    k = min(en, kw["cap"]) if kw.get("cap") is not None else en
    assert len(offs) == k + 1 and (offs == eo[:k + 1]).all(), np.flatnonzero(offs != eo[:k + 1])[:5]
    if text is not None:
        assert len(text) == len(et) and (text == et).all(), np.flatnonzero(text != et)[:5]
    return n


def plain(rng, size):
    """Bytes that are no delimiter of these tests (printable ASCII)."""
    return rng.randint(32, 127, size=size).astype(np.uint8)


def edge_cases(size, rng):
    """(name, raw) for one size: delimiter placements and patterns around byte 0, the last byte, the tile edge at T and the
    16-byte groups."""
    out = [("none", plain(rng, size)), ("all", np.full(size, 10, dtype=np.uint8))]
    if size:
        r = plain(rng, size)
        r[rng.rand(size) < 1 / 40] = 10
        out.append(("random", r))
    places = {"first": [0], "last": [size - 1], "first_and_last": [0, size - 1], "tile_last": [T - 1], "tile_first": [T],
              "tile_both": [T - 1, T], "group_last": [15], "group_first": [16], "group_both": [15, 16]}
    for name, at in places.items():
        if all(0 <= a < size for a in at):
            r = plain(rng, size)
            r[at] = 10
            out.append((name, r))
    for run in (2, 3, 16, 17, 33, 40):
        for name, start in (("tile", T - run // 2), ("tile_end", T - run + 1), ("group", 16 * 5 - run // 2), ("head", 0), ("tail", size - run)):
            if 0 <= start and start + run <= size:
                r = plain(rng, size)
                r[start:start + run] = 10
                out.append(("run%d_%s" % (run, name), r))
    return out


# ---- GPU: pire_hip_split ---------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("size", [0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5])
def test_tile_edges(torch_cuda, size):
    rng = np.random.RandomState(size + 1)
    for name, raw in edge_cases(size, rng):
        try:
            check_split(torch_cuda, raw)
            check_split(torch_cuda, raw, keep=True)
        except AssertionError as e:
            raise AssertionError("size %d, case %s: %s" % (size, name, e))


@gpu
@pytest.mark.parametrize("raw_off", [1, 17, 127])
def test_misaligned_raw_and_out_text_in_poisoned_surroundings(torch_cuda, raw_off):
    """raw at any distance from a 16-byte boundary (its tiles are cut on the boundaries), out_text at another; the bytes in
    front of and behind both outputs stay as they were (DevSplit.fetch looks)."""
    rng = np.random.RandomState(raw_off)
    for size in (3 * T + 5, T - raw_off, T - raw_off + 1, 40, 5):
        raw = plain(rng, size)
        raw[rng.rand(size) < 1 / 30] = 10
        for at in (0, 15 - raw_off % 16, 16 - raw_off % 16, T - raw_off - 1, T - raw_off, size - 1):   # the edges of the grid the kernel cuts on
            if 0 <= at < size:
                raw[at] = 10
        for text_off in (0, 3, 15):
            check_split(torch_cuda, raw, raw_off=raw_off, text_off=text_off)
        check_split(torch_cuda, raw, raw_off=raw_off, keep=True)
    check_split(torch_cuda, plain(rng, 2 * T + 100), raw_off=raw_off, text_off=15)   # one line over three tiles, shifted


def random_lines_raw(rng, lines, top=300, delim=10, last_terminated=True):
    lens = rng.randint(0, top + 1, size=lines)
    raw = plain(rng, int(lens.sum()) + lines)
    raw[np.cumsum(lens + 1) - 1] = delim
    return raw if last_terminated else raw[:-1]


@gpu
def test_scan_carry_over_more_than_1024_tiles(torch_cuda):
    """The one-block scan takes 1 024 tiles a step: a buffer of more tiles than that carries a total from step to step."""
    rng = np.random.RandomState(1024)
    raw = random_lines_raw(rng, 116000)
    assert len(raw) > 1030 * T
    n = check_split(torch_cuda, raw, raw_off=17, text_off=3)
    assert n == 116000
    check_split(torch_cuda, raw[:-1], keep=True)


@gpu
@pytest.mark.parametrize("delim", [0x00, 0x0A, 0xFF])
def test_delimiter_values_on_random_bytes(torch_cuda, delim):
    rng = np.random.RandomState(delim)
    raw = rng.randint(0, 256, size=3 * T + 5).astype(np.uint8)
    raw[rng.rand(len(raw)) < 1 / 50] = delim
    assert 100 < (raw == delim).sum() < len(raw) // 10
    check_split(torch_cuda, raw, delim)
    check_split(torch_cuda, raw, delim, keep=True)
    # bytes that differ from the delimiter in one bit only are none
    near = np.array([delim ^ (1 << b) for b in range(8)], dtype=np.uint8)
    check_split(torch_cuda, np.tile(near, 500), delim)


@gpu
@pytest.mark.parametrize("terminated", [True, False])
def test_offsets_cap(torch_cuda, terminated):
    rng = np.random.RandomState(5)
    raw = random_lines_raw(rng, 700, top=60, last_terminated=terminated)
    n = restate(raw)[2]
    assert n == 700
    for cap in (0, n - 1, n, n + 7):
        for keep in (False, True):
            assert check_split(torch_cuda, raw, cap=cap, keep=keep) == n      # *out_n == n whatever the room
    # no room and no array at all: the count alone
    cnt = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    d = torch_cuda.as_tensor(raw, device="cuda")
    pb.split_device(d.data_ptr(), len(raw), cnt.data_ptr(), stream=torch_cuda.cuda.current_stream().cuda_stream)
    torch_cuda.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n


@gpu
def test_keep_delimiter_form_writes_no_text(torch_cuda):
    rng = np.random.RandomState(9)
    raw = random_lines_raw(rng, 900, top=100, last_terminated=False)
    p = np.flatnonzero(raw == 10)
    call = DevSplit(torch_cuda, raw, keep=True).run()
    text, offs, n = call.fetch()
    assert text is None and n == len(p) + 1
    assert (offs[1:len(p) + 1] == (p + 1).astype(np.uint64)).all() and int(offs[0]) == 0 and int(offs[n]) == len(raw)


@gpu
def test_host_pointers_against_device_pointers(torch_cuda):
    rng = np.random.RandomState(11)
    for raw in (random_lines_raw(rng, 2000), random_lines_raw(rng, 50, last_terminated=False), plain(rng, T + 7),
                np.full(300, 10, dtype=np.uint8)):
        for keep in (False, True):
            et, eo, en = restate(raw, keep=keep)
            dt, do, dn = DevSplit(torch_cuda, raw, keep=keep).run().fetch()
            ht, ho, hn = pb.split_host(raw, keep_delim=keep)
            assert hn == dn == en and (ho == do).all() and (ho == eo).all()
            if not keep:
                assert (ht == dt).all() and (ht == et).all()
            else:
                assert ht is None
            for cap in (0, en - 1, en + 7):
                ht, ho, hn = pb.split_host(raw, keep_delim=keep, offsets_cap=cap)
                assert hn == en and (ho == eo[:min(en, cap) + 1]).all()
    # the host form in its caller's poisoned arrays: nothing behind what it owes
    raw = random_lines_raw(rng, 300, top=40)
    et, eo, en = restate(raw)
    text = np.full(len(raw) + 64, POISON, dtype=np.uint8)
    offs = np.full(en - 5 + 1 + GUARD, POISON64, dtype=np.uint64)
    n = C.c_uint64(0)
    assert pb.lib().pire_hip_split(raw.ctypes.data, len(raw), 10, 0, text.ctypes.data, offs.ctypes.data, en - 5, C.byref(n), None) == 0
    assert n.value == en and (offs[:en - 4] == eo[:en - 4]).all() and (offs[en - 4:] == np.uint64(POISON64)).all()
    assert (text[:len(et)] == et).all() and (text[len(et):] == POISON).all()


@gpu
def test_two_device_calls_are_bit_identical(torch_cuda):
    rng = np.random.RandomState(13)
    raw = random_lines_raw(rng, 30000, last_terminated=False)
    a = DevSplit(torch_cuda, raw, raw_off=1, text_off=3).run().everything()
    b = DevSplit(torch_cuda, raw, raw_off=1, text_off=3).run().everything()
    assert a == b
    et, eo, en = restate(raw)
    assert a[0][3:3 + len(et)] == et.tobytes()


# ---- GPU: pire_hip_run_lines_select --------------------------------------------------------------------------------------

LINES = 4000


def planted_raw(big, seed, lines=LINES, top=300, last_terminated=True):
    """About `lines` lines of 0..top bytes cut from the tails of the synthetic corpus' records (where helpers.plants_for puts
    most witnesses), newline between them; a newline inside a record becomes a blank."""
    rec = ob.corpus_fill(seed, 0, lines, top, H.plants_for(big), threads=4)
    rec[rec == 10] = 32
    lens = np.random.RandomState(seed).randint(0, top + 1, size=lines)
    parts = []
    for i in range(lines):
        parts.append(rec[i, top - lens[i]:])
        parts.append(np.array([10], dtype=np.uint8))
    raw = np.concatenate(parts)
    return raw if last_terminated else raw[:-1]


_expect_cache = {}


def expected_lines_select(name, t, o, raw, flags, want):
    """From the restatement and the oracle: lines, hits, spans' bytes, masks, count."""
    key = (name, raw.tobytes(), flags)
    if key not in _expect_cache:
        text, offs, n = restate(raw)
        idx = o.run(text, offs, flags=flags, threads=4)[0] if n else np.zeros(0, dtype=np.uint32)
        rec = {}
        for s in np.unique(idx).tolist():
            m = 0
            for r in t.AcceptedRegexps(s):
                if r < t.RegexpsCount:
                    m |= 1 << r
            rec[s] = (m, bool(t.Final(s)) and t.RegexpsCount > 0)
        masks = np.array([rec[s][0] for s in idx.tolist()], dtype=np.uint64)
        fin = np.array([rec[s][1] for s in idx.tolist()], dtype=bool)
        _expect_cache[key] = (text, offs, n, masks, fin)
    text, offs, n, masks, fin = _expect_cache[key]
    sel = fin if want is None else (masks & np.uint64(sum(1 << r for r in want))) != 0
    hits = np.flatnonzero(sel).astype(np.uint64)
    return {"lines": n, "hits": hits, "count": len(hits), "hit_masks": masks[sel],
            "bytes": [text[int(offs[i]):int(offs[i + 1])].tobytes() for i in hits.tolist()]}


def dev_run_lines_select(torch, t, raw, flags, want=None, cap=None, raw_off=0):
    size = len(raw)
    cap = size if cap is None else cap
    host = np.full(raw_off + size + 256, 10, dtype=np.uint8)
    host[raw_off:raw_off + size] = raw
    d = torch.as_tensor(host, device="cuda")
    poison = int(np.uint64(POISON64).astype(np.int64))
    hits = torch.full((cap + GUARD,), poison, dtype=torch.int64, device="cuda")
    spans = torch.full(((cap + GUARD) * 2,), poison, dtype=torch.int64, device="cuda")
    masks = torch.full((cap + GUARD,), poison, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), poison, dtype=torch.int64, device="cuda")
    wm = t.want_mask(want)
    dw = None if wm is None else torch.as_tensor(wm.view(np.int64), device="cuda")
    assert t.mask_words == 1
    t.run_lines_select_device(d.data_ptr() + raw_off if size else 0, size, flags, counts.data_ptr(), counts.data_ptr() + 8,
                              want_ptr=0 if dw is None else dw.data_ptr(), out_hits_ptr=hits.data_ptr() if cap else 0,
                              out_hit_spans_ptr=spans.data_ptr() if cap else 0, out_hit_masks_ptr=masks.data_ptr() if cap else 0,
                              hit_cap=cap, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64)
    k = min(int(c[1]), cap)
    h, s, m = (b.cpu().numpy().view(np.uint64) for b in (hits, spans, masks))
    assert (h[k:] == np.uint64(POISON64)).all() and (s[2 * k:] == np.uint64(POISON64)).all() and (m[k:] == np.uint64(POISON64)).all()
    return {"lines": int(c[0]), "count": int(c[1]), "hits": h[:k], "spans": s[:2 * k].reshape(k, 2), "hit_masks": m[:k]}


def check_lines_select(got, exp, raw, cap=None):
    assert got["lines"] == exp["lines"] and got["count"] == exp["count"]
    k = exp["count"] if cap is None else min(cap, exp["count"])
    assert len(got["hits"]) == k and (got["hits"] == exp["hits"][:k]).all()
    assert (got["hit_masks"].reshape(-1) == exp["hit_masks"][:k]).all()
    assert got["spans"].shape == (k, 2)
    assert [raw[int(b):int(e)].tobytes() for b, e in got["spans"]] == exp["bytes"][:k]


@gpu
@pytest.mark.parametrize("name", ["set_a", "c2_single"])     # set_a: eight regexps glued into one scanner
def test_run_lines_select_against_oracle_and_restatement(torch_cuda, name):
    big = [b for b in H.big_sets() if b["name"] == name][0]
    blob = H.load_blob(big["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    raw = planted_raw(big, seed=77, last_terminated=(name == "set_a"))
    full = expected_lines_select(name, t, o, raw, BE, None)
    assert full["lines"] == LINES and 100 < full["count"] < LINES - 100, full["count"]   # (hits and misses both plentiful)
    for flags in (0, pb.FLAG_BEGIN, pb.FLAG_END, BE):
        for want in (None, [0]):
            exp = expected_lines_select(name, t, o, raw, flags, want)
            check_lines_select(dev_run_lines_select(torch_cuda, t, raw, flags, want, raw_off=flags), exp, raw)
    # room for fewer hits than there are; no room at all
    for cap in (full["count"] - 3, 1, 0):
        check_lines_select(dev_run_lines_select(torch_cuda, t, raw, BE, None, cap=cap), full, raw, cap=cap)
    # the scan kernel is the one the call names
    assert pb.last_kernel() not in ("", None)
    # host pointers: the same answer
    got = t.run_lines_select_host(raw)
    check_lines_select(got, full, raw)
    got = t.run_lines_select_host(raw, want=[0], hit_cap=5)
    check_lines_select(got, expected_lines_select(name, t, o, raw, BE, [0]), raw, cap=5)


@gpu
def test_run_lines_select_on_empty_and_delimiter_only_buffers(torch_cuda):
    big = [b for b in H.big_sets() if b["name"] == "c2_single"][0]
    blob = H.load_blob(big["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    for raw in (np.zeros(0, dtype=np.uint8), np.full(1, 10, dtype=np.uint8), np.full(T + 3, 10, dtype=np.uint8)):
        exp = expected_lines_select("c2_single", t, o, raw, BE, None)
        assert exp["lines"] == len(raw) and exp["count"] == 0
        check_lines_select(dev_run_lines_select(torch_cuda, t, raw, BE, cap=4), exp, raw, cap=4)
        check_lines_select(t.run_lines_select_host(raw, hit_cap=4), exp, raw, cap=4)
    # a scanner that accepts the empty line: every line of a buffer of delimiters is a hit
    case = [c for c in H.all_cases() if c["name"] == "rep_3_inf"][0]
    star = [c for c in H.all_cases() if c["name"] == "misc_1"][0]     # ^[^\s=/>]*$
    for c in (case, star):
        blob = H.load_blob(c["blob"])
        t, o = pb.Table(blob), ob.OracleScanner(blob)
        raw = np.concatenate([np.full(70, 10, dtype=np.uint8), u8(b"xxx\nxx\n\nxxxx")])
        exp = expected_lines_select(c["name"], t, o, raw, BE, None)
        check_lines_select(dev_run_lines_select(torch_cuda, t, raw, BE), exp, raw)
    assert exp["count"] >= 71
