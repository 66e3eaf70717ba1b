"""pire_hip_fields / pire_hip_run_lines_field_select / _gather: where one column of every string is, found on the device
(fields.hip), and the lines of a raw buffer whose column matches, in one call.

Exact equality everywhere.  The expected spans come from `restate` -- the header's formulas written down over bytes.split --,
the scan's from the C oracle on the fields `restate` cuts; masks and Final from the host accessors Table.AcceptedRegexps /
Table.Final.  Nothing expected comes from the library."""
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
T = pb.FIELDS_TILE
BE = pb.FLAG_BEGIN | pb.FLAG_END
POISON64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8
FIELDS = [0, 1, 2, 7, 2 ** 31]
gpu = pytest.mark.gpu


# ---- the restatement ---------------------------------------------------------------------------------------------------

def restate(text, offs, field, sep=9, rest=False):
    """spans uint64[n, 2] as include/pire_hip.h states them."""
    data, n = bytes(np.asarray(text, dtype=np.uint8)), len(offs) - 1
    spans = np.zeros((n, 2), dtype=np.uint64)
    for i in range(n):
        b, e = int(offs[i]), int(offs[i + 1])
        parts = data[b:e].split(bytes([sep]))          # m separators: m + 1 fields, empty ones included
        if field < len(parts):
            begin = b + sum(len(p) + 1 for p in parts[:field])
            spans[i] = (begin, e if rest else begin + len(parts[field]))
        else:
            spans[i] = (e, e)
    return spans


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def cut(text, lens):
    """offsets of strings of the given lengths over text (they add up to its size)."""
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    assert int(offs[-1]) == len(text)
    return offs


# ---- CPU -----------------------------------------------------------------------------------------------------------------

def test_restatement_on_hand_written_cases():
    strings = [b"a\tbb\tccc", b"", b"\t", b"x", b"\tx", b"x\t", b"a\t\tb", b"\t\t"]
    text, offs = H.pack(strings)
    o = [int(x) for x in offs]

    def cols(field, rest=False):
        return [bytes(text[int(b):int(e)]) for b, e in restate(text, offs, field, rest=rest)]

    assert cols(0) == [b"a", b"", b"", b"x", b"", b"x", b"a", b""]
    assert cols(1) == [b"bb", b"", b"", b"", b"x", b"", b"", b""]
    assert cols(2) == [b"ccc", b"", b"", b"", b"", b"", b"b", b""]
    assert cols(3) == [b""] * 8 and cols(2 ** 31) == [b""] * 8
    assert cols(0, rest=True) == strings
    assert cols(1, rest=True) == [b"bb\tccc", b"", b"", b"", b"x", b"", b"\tb", b"\t"]
    # where the empty spans lie: behind the separator that opens the field, or at the end of a string that has too few
    assert restate(text, offs, 1).tolist()[2] == [o[2] + 1, o[2] + 1] and restate(text, offs, 1).tolist()[3] == [o[4], o[4]]
    assert restate(text, offs, 1).tolist()[6] == [o[6] + 2, o[6] + 2] and restate(text, offs, 5).tolist()[1] == [o[1], o[1]]
    assert cols(0, rest=False) == [s.split(b"\t")[0] for s in strings]
    assert restate(u8(b"a\x00b\xffc"), [0, 5], 1, sep=0).tolist() == [[2, 5]] and restate(u8(b"a\x00b\xffc"), [0, 5], 1, sep=255).tolist() == [[4, 5]]


def test_the_library_exports_the_fields_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    for name in ("pire_hip_fields", "pire_hip_run_lines_field_select", "pire_hip_run_lines_field_gather"):
        assert hasattr(L, name), name
        assert name in {n for n, _, _ in pb.ABI}
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        h = f.read()
    assert int(re.search(r"#define PIRE_HIP_FIELDS_TILE_BYTES (\d+)u", h).group(1)) == T == 16384
    assert int(re.search(r"#define PIRE_HIP_FIELDS_REST (0x[0-9a-f]+)u", h).group(1), 16) == pb.FIELDS_REST == 1


def test_fields_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    text = u8(b"a\tb" * 4).copy()
    offs = np.array([0, 3, 6, 9, 12], dtype=np.uint64)
    spans = np.full(8, 77, dtype=np.uint64)
    t, o, s = text.ctypes.data, offs.ctypes.data, spans.ctypes.data
    cases = {
        "sep > 255": (t, o, 4, 256, 0, 0, s),
        "unknown bits in mode": (t, o, 4, 9, 0, 2, s),
        "n > 0 with null offsets": (t, None, 4, 9, 0, 0, s),
        "n > 0 with null out_spans": (t, o, 4, 9, 0, 0, None),
    }
    for what, (a_t, a_o, n, sep, field, mode, a_s) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_fields(a_t, a_o, n, sep, field, mode, flags, a_s, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    # host pointers: the text the offsets speak of has to be there, and they must not decrease
    assert L.pire_hip_fields(None, o, 4, 9, 0, 0, 0, s, None) == -1 and "null text" in L.pire_hip_last_error().decode()
    down = np.array([0, 3, 2, 9, 12], dtype=np.uint64)
    assert L.pire_hip_fields(t, down.ctypes.data, 4, 9, 0, 0, 0, s, None) == -1 and "non-decreasing" in L.pire_hip_last_error().decode()
    # 2^32 strings (addresses nobody owns: the call must not touch them)
    for flags in (0, pb.FLAG_ON_DEVICE):
        assert L.pire_hip_fields(0x7000000000, 0x7100000000, 1 << 32, 9, 0, 0, flags, 0x7200000000, None) == -5
        assert "2^32" in L.pire_hip_last_error().decode()
    # no strings: nothing to do, nothing written, no device
    for flags in (0, pb.FLAG_ON_DEVICE):
        assert L.pire_hip_fields(None, None, 0, 9, 3, 1, flags, None, None) == 0
    assert (spans == 77).all()


def test_run_lines_field_validation_refuses_before_any_device_is_touched():
    L = pb.lib()
    t = pb.Table(H.load_blob("c2_single.blob"))
    raw = u8(b"k\thello  world\nabc\n").copy()
    hits, spans, masks, offs = np.zeros(4, np.uint64), np.zeros(8, np.uint64), np.zeros(4, np.uint64), np.zeros(5, np.uint64)
    out = np.zeros(64, np.uint8)
    lines, cnt, total = C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    r, lp, cp, bp = raw.ctypes.data, C.addressof(lines), C.addressof(cnt), C.addressof(total)
    h, s, m = hits.ctypes.data, spans.ctypes.data, masks.ctypes.data
    cases = {
        "null table": (None, r, raw.size, 10, 9, 0, lp, h, 4, cp),
        "delim > 255": (t._h, r, raw.size, 300, 9, 0, lp, h, 4, cp),
        "sep > 255": (t._h, r, raw.size, 10, 256, 0, lp, h, 4, cp),
        "sep == delim": (t._h, r, raw.size, 10, 10, 0, lp, h, 4, cp),
        "unknown bits in mode": (t._h, r, raw.size, 10, 9, 4, lp, h, 4, cp),
        "null out_line_count": (t._h, r, raw.size, 10, 9, 0, None, h, 4, cp),
        "size > 0 with null raw": (t._h, None, raw.size, 10, 9, 0, lp, h, 4, cp),
        "null out_hit_count": (t._h, r, raw.size, 10, 9, 0, lp, h, 4, None),
    }
    for what, (th, a_raw, size, delim, sep, mode, a_lines, a_h, cap, a_c) in cases.items():
        for flags in (BE, BE | pb.FLAG_ON_DEVICE):
            assert L.pire_hip_run_lines_field_select(th, a_raw, size, delim, sep, 1, mode, flags, None, a_lines, a_h, s, m, cap, a_c,
                                                     None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
            assert L.pire_hip_run_lines_field_gather(th, a_raw, size, delim, sep, 1, mode, flags, None, 10, a_lines, a_h, cap, a_c,
                                                     out.ctypes.data, out.size, offs.ctypes.data, bp, None) == -1, what
            assert what in L.pire_hip_last_error().decode(), (what, L.pire_hip_last_error())
    for flags in (BE, BE | pb.FLAG_ON_DEVICE):
        assert L.pire_hip_run_lines_field_select(t._h, r, raw.size, 10, 9, 1, 0, flags, None, lp, None, None, None, 4, cp, None) == -1
        assert "hit_cap > 0 with null out_hits" in L.pire_hip_last_error().decode()
        assert L.pire_hip_run_lines_field_gather(t._h, r, raw.size, 10, 9, 1, 0, flags, None, 10, lp, h, 4, cp, out.ctypes.data, out.size,
                                                 offs.ctypes.data, None, None) == -1
        assert "null out_bytes" in L.pire_hip_last_error().decode()
    assert (lines.value, cnt.value, total.value) == (77, 78, 79) and not hits.any() and not spans.any() and not out.any()
    # an empty buffer with host pointers is answered without a device
    assert L.pire_hip_run_lines_field_select(t._h, None, 0, 10, 9, 1, 0, BE, None, lp, h, s, m, 4, cp, None) == 0
    assert (lines.value, cnt.value) == (0, 0)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_fields_unit_passes_the_build_audit():
    """fields.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "fields.hip" in ba.NO_SCRATCH and "fields.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        assert f.read().count("fields.hip") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("fields.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Fields" in k for k in seen), seen


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def dev_u64(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64), device="cuda")


class DevFields:
    """One pire_hip_fields call on device pointers.  text sits `text_off` bytes into an aligned allocation whose other bytes
    ARE the separator (a lane that reads past either end of the text counts them); out_spans has GUARD poisoned words behind
    entry 2n.  After fetch(): spans -- and the guard and the inputs have been looked at."""

    def __init__(self, torch, text, offs, field, sep=9, rest=False, text_off=0):
        self.torch = torch
        text = np.asarray(text, dtype=np.uint8)
        self.n, self.field, self.sep, self.rest = len(offs) - 1, field, sep, rest
        host = np.full(text_off + len(text) + 256, sep, dtype=np.uint8)
        host[text_off:text_off + len(text)] = text
        self.host_in = host
        self.dev_in = torch.as_tensor(host, device="cuda")
        assert self.dev_in.data_ptr() % 256 == 0
        self.text_ptr = self.dev_in.data_ptr() + text_off
        self.offs = dev_u64(torch, offs)
        self.spans = torch.full((2 * self.n + GUARD,), int(np.uint64(POISON64).astype(np.int64)), dtype=torch.int64, device="cuda")

    def run(self):
        pb.fields_device(self.text_ptr, self.offs.data_ptr(), self.n, self.field, self.spans.data_ptr(), self.sep, self.rest,
                         self.torch.cuda.current_stream().cuda_stream)
        return self

    def fetch(self):
        self.torch.cuda.synchronize()
        assert (self.dev_in.cpu().numpy() == self.host_in).all(), "the input was written to"
        s = self.spans.cpu().numpy().view(np.uint64)
        assert (s[2 * self.n:] == np.uint64(POISON64)).all(), "out_spans written behind entry 2n"
        return s[:2 * self.n].reshape(self.n, 2)


def check_fields(torch, text, offs, fields=FIELDS, seps=(9,), text_off=0):
    for sep in seps:
        for field in fields:
            for rest in (False, True):
                exp = restate(text, offs, field, sep, rest)
                got = DevFields(torch, text, offs, field, sep, rest, text_off).run().fetch()
                bad = np.flatnonzero((got != exp).any(axis=1))
                assert not len(bad), "field %d rest %d sep %d: strings %s: got %s, expected %s" % (
                    field, rest, sep, bad[:5].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())


def plain(rng, size):
    """Bytes that are no separator or delimiter of these tests (printable ASCII)."""
    return rng.randint(32, 127, size=size).astype(np.uint8)


def random_cut(rng, size, mean):
    """Random string lengths that add up to size: empty strings, short ones and a few long ones."""
    lens = []
    left = size
    while left:
        k = int(rng.choice([0, 0, rng.randint(0, 2 * mean + 1), rng.randint(0, 2 * mean + 1), rng.randint(0, 8 * mean + 1)]))
        k = min(k, left)
        lens.append(k)
        left -= k
    return lens + [0, 0]


def with_seps(rng, size, density, sep=9):
    text = plain(rng, size)
    if density >= 1:
        text[:] = sep
    elif density > 0:
        text[rng.rand(size) < density] = sep
    return text


# ---- GPU: pire_hip_fields --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("size", [0, 1, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5])
def test_text_sizes_and_separator_densities(torch_cuda, size):
    rng = np.random.RandomState(size + 1)
    for density in (0, 1 / 8, 1):
        text = with_seps(rng, size, density)
        check_fields(torch_cuda, text, cut(text, random_cut(rng, size, 40)))
    # one string that is the whole text; the whole text behind n empty strings, and in front of them
    text = with_seps(rng, size, 1 / 8)
    check_fields(torch_cuda, text, cut(text, [size]))
    check_fields(torch_cuda, text, cut(text, [0, 0, 0, size]), fields=[0, 2])
    check_fields(torch_cuda, text, cut(text, [size, 0, 0, 0]), fields=[0, 2])


@gpu
def test_separator_positions_inside_a_string(torch_cuda):
    """The separator as a string's first byte, its last one, doubled, tripled; strings without one; every field up to 4."""
    pieces = [b"\tab", b"ab\t", b"\t", b"\t\t", b"a\t\tb", b"ab", b"", b"\tab\t", b"a\tb\tc\td\te", b"\t\t\t", b"abc\t\t", b"x"]
    rng = np.random.RandomState(3)
    strings = [pieces[i] for i in rng.randint(0, len(pieces), size=3000)]   # (48 tiles of strings would be one per lane; these fill 1)
    text, offs = H.pack(strings)
    check_fields(torch_cuda, text, offs, fields=[0, 1, 2, 3, 4])
    text, offs = H.pack(pieces)
    check_fields(torch_cuda, text, offs, fields=[0, 1, 2, 3, 4, 5], text_off=5)


def across_tiles(rng, edge):
    """Strings laid around the tile edges at edge, edge + T, edge + 2T: a string over more than three tiles whose first three
    separators lie one in each of the tiles BEHIND the one it starts in; runs of equal offsets (empty strings) at edge - 1,
    edge and edge + 1 and at the next edge; a string that starts exactly on an edge."""
    lens = [edge - 41, 40, 0, 0, 1, 0, 0, 0, 1, 0, 7,           # boundaries at edge - 1 (x3), edge (x4), edge + 1 (x2)
            T - 8 - 200, 3 * T + 300,                           # the long one: starts at edge + T - 200
            0, 0, T - 100, 0, 50]                               # ends on edge + 5T exactly: the next string starts on an edge
    text = plain(rng, sum(lens))
    offs = cut(text, lens)
    long_at = int(offs[12])
    assert long_at == edge + T - 200 and int(offs[13]) == edge + 4 * T + 100 and int(offs[16]) == edge + 5 * T
    for tile in (2, 3, 4):
        text[edge + (tile - 1) * T + 77 * tile] = 9             # the long string's separators: in tiles 2, 3 and 4
    text[long_at - 3] = 9                                       # one in the string in front of it, in the long one's first tile
    text[[edge - 1, edge, edge + 1]] = 9                        # the one-byte strings around the first edge ARE separators
    text[int(offs[16])] = 9                                     # ... and the first byte of the string that starts on an edge
    text[int(offs[16]) + 30] = 9
    text[5], text[20] = 9, 9
    return text, offs


@gpu
@pytest.mark.parametrize("text_off", [0, 1, 15])
def test_strings_across_tiles_and_empty_strings_on_tile_edges(torch_cuda, text_off):
    rng = np.random.RandomState(text_off + 40)
    text, offs = across_tiles(rng, T - text_off)                # (tiles are cut on the 16-byte grid of text's ADDRESS)
    exp = restate(text, offs, 2)
    assert exp[12].tolist() == [T - text_off + 2 * T + 77 * 3 + 1, T - text_off + 3 * T + 77 * 4]   # begin and end in different tiles
    check_fields(torch_cuda, text, offs, fields=[0, 1, 2, 3, 4], text_off=text_off)
    # the same text as ONE string, and as one string between two empty ones
    check_fields(torch_cuda, text, cut(text, [len(text)]), fields=[0, 3, 7, 9, 10], text_off=text_off)
    check_fields(torch_cuda, text, cut(text, [0, len(text), 0]), fields=[1, 8], text_off=text_off)


@gpu
def test_carry_over_more_than_1024_tiles(torch_cuda):
    """16 MiB + 5 bytes are 1 025 tiles, one per block: the one-block carry pass takes 1 024 records a step, and the string
    that is open across tile 1 024 has its separators on both sides of that step."""
    rng = np.random.RandomState(1024)
    size = 1024 * T + 5
    text = plain(rng, size)
    lens = [int(x) for x in rng.randint(0, 6000, size=5400)]
    while sum(lens) > 1000 * T:
        lens.pop()
    lens += [1000 * T - sum(lens) + 123]
    long_at = sum(lens)
    lens += [size - long_at]                                    # open from tile 1 000 to the last byte
    assert 1000 * T < long_at < 1001 * T
    text[rng.rand(size) < 1 / 700] = 9
    text[long_at:] = 65
    marks = [long_at + 5, 1010 * T + 3, 1023 * T + 16383, 1024 * T, 1024 * T + 3, size - 1]
    text[marks] = 9
    offs = cut(text, lens)
    n = len(lens)
    for field, rest in ((0, False), (3, False), (4, False), (5, True), (6, False), (7, False)):
        exp = restate(text, offs, field, rest=rest)
        got = DevFields(torch_cuda, text, offs, field, rest=rest).run().fetch()
        assert (got == exp).all(), (field, np.flatnonzero((got != exp).any(axis=1))[:5])
        if field in (3, 4, 5):
            assert int(exp[n - 1][0]) == marks[field - 1] + 1       # the span begins in or behind tile 1 023
    host = pb.fields_host(text, offs, 4)
    assert (host == restate(text, offs, 4)).all()


@gpu
def test_blocks_that_walk_more_than_one_tile(torch_cuda):
    """A device-pointer call has 2 048 blocks: 48 MiB + 5 bytes are 3 073 tiles, so block b walks tiles 2b and 2b + 1 and
    carries the open string's separators from the one into the other itself (the inner edges are the odd multiples of T, the
    edges between two runs the even ones).  One string open from tile 99 to tile 105 with its separators on both sides of an
    inner edge (ranks 2 and 3) and of an edge between runs (ranks 0 and 1), tiles without any string start in the middle and
    at the head of a run; strings that start exactly on an inner edge and on a run edge, empty strings on both."""
    rng = np.random.RandomState(2048)
    size = 3072 * T + 5
    text = plain(rng, size)
    text[rng.randint(0, size, size=25000)] = 9
    lens = []
    while sum(lens) < 100 * T - 50 - 6000:
        lens.append(int(rng.choice([0, rng.randint(0, 6000)])))
    lens.append(100 * T - 50 - sum(lens))
    long_at = sum(lens)
    lens += [5 * T + 60,                                         # the long one: [100T - 50, 105T + 10)
             2 * T - 11, 1, 0, 0, 0, 1, 0, 0, T - 1, 0, 0]       # ..., [107T - 1], 3 empty, [107T], 2 empty, [107T + 1, 108T), 2 empty
    assert long_at == 100 * T - 50 and sum(lens) == 108 * T
    inner_start, run_start = len(lens) - 6, len(lens)            # the strings that begin at 107T and at 108T
    while size - sum(lens) > 40000:
        lens.append(int(rng.choice([0, rng.randint(0, 40000)])))
    lens.append(size - sum(lens))
    text[long_at:105 * T + 10] = 65
    marks = [100 * T - 10, 100 * T + 5, 101 * T - 1, 101 * T, 102 * T + 7, 103 * T + 100, 105 * T + 3]
    text[marks] = 9
    text[[107 * T - 1, 107 * T, 107 * T + 1, 107 * T + 9, 108 * T - 1, 108 * T, 108 * T + 1]] = 9
    offs = cut(text, lens)
    long_i = int(np.flatnonzero(offs[:-1] == np.uint64(long_at))[-1])
    assert int(offs[inner_start]) == 107 * T and int(offs[inner_start + 1]) == 107 * T + 1 and int(offs[run_start]) == 108 * T
    assert ((offs[1:] - offs[:-1]).astype(np.int64) > 2 * T).sum() > 100      # strings over several tiles of other runs, too
    for field, rest in ((0, False), (1, False), (2, True), (3, False), (4, False), (6, False), (7, False)):
        exp = restate(text, offs, field, rest=rest)
        got = DevFields(torch_cuda, text, offs, field, rest=rest).run().fetch()
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert not len(bad), (field, rest, bad[:5].tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())
        if 1 <= field <= 6:
            assert int(exp[long_i][0]) == marks[field - 1] + 1 and (rest or int(exp[long_i][1]) == marks[field])
    assert restate(text, offs, 1)[inner_start].tolist() == [107 * T + 1, 107 * T + 1]


@gpu
def test_many_empty_strings_between_two_separators_of_one_lane(torch_cuda):
    """"a<TAB>", 5 000 empty strings, "<TAB>b": both separators in one lane's 16 bytes, more strings in the tile than its
    boundaries' stage holds."""
    for pad in (0, 21, T - 2):
        strings = ([b"p" * pad] if pad else []) + [b"a\t"] + [b""] * 5000 + [b"\tb", b"c\td", b""]
        text, offs = H.pack(strings)
        check_fields(torch_cuda, text, offs, fields=[0, 1, 2])


@gpu
@pytest.mark.parametrize("sep", [0x00, 0x09, 0xFF])
def test_separator_values_on_random_bytes(torch_cuda, sep):
    rng = np.random.RandomState(sep)
    text = rng.randint(0, 256, size=3 * T + 5).astype(np.uint8)
    text[rng.rand(len(text)) < 1 / 20] = sep
    offs = cut(text, random_cut(rng, len(text), 60))
    check_fields(torch_cuda, text, offs, fields=[0, 1, 2], seps=(sep,))
    # bytes that differ from the separator in one bit only are none
    near = np.tile(np.array([sep ^ (1 << b) for b in range(8)], dtype=np.uint8), 500)
    check_fields(torch_cuda, near, cut(near, [1000, 3000]), fields=[0, 1], seps=(sep,))


@gpu
@pytest.mark.parametrize("text_off", [1, 17, 127])
def test_misaligned_text_in_poisoned_surroundings(torch_cuda, text_off):
    """text at any distance from a 16-byte boundary, the bytes around it being separators that no lane may count; out_spans
    with a poisoned guard behind entry 2n (DevFields.fetch looks)."""
    rng = np.random.RandomState(text_off)
    for size in (3 * T + 5, T - text_off, T - text_off + 1, 40, 5):
        text = with_seps(rng, size, 1 / 10)
        for at in (0, 15 - text_off % 16, 16 - text_off % 16, T - text_off - 1, T - text_off, size - 1):   # the edges of the grid
            if 0 <= at < size:
                text[at] = 9
        check_fields(torch_cuda, text, cut(text, random_cut(rng, size, 30)), fields=[0, 1, 2, 7], text_off=text_off)
        check_fields(torch_cuda, text, cut(text, [size]), fields=[0, 1, 7], text_off=text_off)


@gpu
def test_host_pointers_against_device_pointers_and_two_calls_bit_identical(torch_cuda):
    rng = np.random.RandomState(11)
    text = with_seps(rng, 5 * T + 77, 1 / 12)
    offs = cut(text, random_cut(rng, len(text), 50))
    for field in (0, 2, 7):
        for rest in (False, True):
            exp = restate(text, offs, field, rest=rest)
            a = DevFields(torch_cuda, text, offs, field, rest=rest, text_off=3).run()
            b = DevFields(torch_cuda, text, offs, field, rest=rest, text_off=3).run()
            got = a.fetch()
            assert (got == exp).all() and (pb.fields_host(text, offs, field, rest=rest) == exp).all()
            assert a.spans.cpu().numpy().tobytes() == b.spans.cpu().numpy().tobytes()
    # the host form in its caller's poisoned array: nothing behind entry 2n; all strings empty: no text needed
    n = len(offs) - 1
    spans = np.full(2 * n + GUARD, POISON64, dtype=np.uint64)
    assert pb.lib().pire_hip_fields(text.ctypes.data, offs.ctypes.data, n, 9, 1, 0, 0, spans.ctypes.data, None) == 0
    assert (spans[:2 * n].reshape(n, 2) == restate(text, offs, 1)).all() and (spans[2 * n:] == np.uint64(POISON64)).all()
    assert pb.fields_host(np.zeros(0, np.uint8), np.zeros(6, np.uint64), 0).tolist() == [[0, 0]] * 5
    # offsets that do not begin at 0: the bytes in front of them are not the batch's
    shifted = offs[40:].copy()
    assert int(shifted[0]) > 0
    assert (pb.fields_host(text, shifted, 1) == restate(text, shifted, 1)).all()
    got = DevFields(torch_cuda, text, shifted, 1, text_off=9).run().fetch()
    assert (got == restate(text, shifted, 1)).all()


@gpu
def test_fields_chained_into_gather_spans_on_the_device(torch_cuda):
    """pire_hip_fields -> pire_hip_gather_spans, device pointers only: the fields back to back, string i the field of string i."""
    torch = torch_cuda
    rng = np.random.RandomState(17)
    text = with_seps(rng, 4 * T + 9, 1 / 15)
    offs = cut(text, random_cut(rng, len(text), 45))
    n = len(offs) - 1
    stream = torch.cuda.current_stream().cuda_stream
    for field, rest in ((0, False), (1, False), (2, True)):
        call = DevFields(torch, text, offs, field, rest=rest, text_off=1).run()
        out = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
        out_offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        pb.gather_spans_device(call.text_ptr, len(text), call.spans.data_ptr(), total.data_ptr(), span_cap=n,
                               out_text_ptr=out.data_ptr(), text_cap=len(text), out_offsets_ptr=out_offs.data_ptr(), stream=stream)
        exp = restate(text, offs, field, rest=rest)
        assert (call.fetch() == exp).all()
        cols = [text[int(b):int(e)].tobytes() for b, e in exp]
        et, eo = H.pack(cols)
        assert int(total.cpu()[0]) == len(et) and (out_offs.cpu().numpy().view(np.uint64) == eo).all()
        assert (out.cpu().numpy()[:len(et)] == et).all()


# ---- GPU: pire_hip_run_lines_field_select / _gather ------------------------------------------------------------------------

LINES = 600
FIELD = 2
NOISE = np.frombuffer(b"0123456789_", dtype=np.uint8)


def column_raw(big, seed, last_terminated=True):
    """LINES lines of 3-5 TAB-separated columns of noise.  Kinds, by line number modulo 6: 0, 1 a witness IS column FIELD or
    ends it (these must hit); 2 a witness ends ANOTHER column and the line (these must not hit: a whole-line scan selects
    them); 3 noise only; 4 too few columns (the empty field is scanned); 5 a witness is column FIELD of a line of FIELD + 1
    columns -- the column ends where the line does."""
    rng = np.random.RandomState(seed)
    witnesses = [w for w in (bytes.fromhex(h) for h in big["witnesses_hex"]) if b"\t" not in w and b"\n" not in w]
    kinds, lines = [], []

    def noise():
        return NOISE[rng.randint(0, len(NOISE), size=rng.randint(0, 30))].tobytes()

    for i in range(LINES):
        kind = i % 6
        w = witnesses[rng.randint(0, len(witnesses))]
        cols = [noise() for _ in range(rng.randint(3, 6))]
        if kind == 0:
            cols[FIELD] = w
        elif kind == 1:
            cols[FIELD] = noise() + b" " + w
        elif kind == 2:
            cols = cols[:FIELD + 1] + [noise(), noise() + b" " + w]
            cols[0] = w
        elif kind == 4:
            cols = cols[:rng.randint(0, FIELD + 1)]
        elif kind == 5:
            cols = cols[:FIELD] + [w]
        kinds.append(kind)
        lines.append(b"\t".join(cols))
    raw = u8(b"\n".join(lines) + (b"\n" if last_terminated else b""))
    return raw, np.array(kinds), lines


_expect_cache = {}


def expected(name, t, o, lines, column, flags, want):
    """From the restatement and the oracle on the cut column: hits, masks, count."""
    key = (name, column, flags)
    if key not in _expect_cache:
        text, offs = H.pack(lines)
        spans = restate(text, offs, *column)
        ftext, foffs = H.pack([text[int(b):int(e)].tobytes() for b, e in spans])
        idx = o.run(ftext, foffs, flags=flags, threads=4)[0] if lines else np.zeros(0, dtype=np.uint32)
        rec = {}
        for s in np.unique(idx).tolist():
            m = 0
            for r in t.AcceptedRegexps(s):
                if r < t.RegexpsCount:
                    m |= 1 << r
            rec[s] = (m, bool(t.Final(s)) and t.RegexpsCount > 0)
        _expect_cache[key] = (np.array([rec[s][0] for s in idx.tolist()], dtype=np.uint64),
                              np.array([rec[s][1] for s in idx.tolist()], dtype=bool))
    masks, fin = _expect_cache[key]
    sel = fin if want is None else (masks & np.uint64(sum(1 << r for r in want))) != 0
    hits = np.flatnonzero(sel).astype(np.uint64)
    return {"lines": len(lines), "hits": hits, "count": len(hits), "hit_masks": masks[sel], "bytes": [lines[i] for i in hits.tolist()]}


def dev_field_select(torch, t, raw, column, flags, want=None, cap=None, raw_off=0, gather=False):
    size = len(raw)
    cap = size if cap is None else cap
    host = np.full(raw_off + size + 256, 10, dtype=np.uint8)
    host[raw_off:raw_off + size] = raw
    d = torch.as_tensor(host, device="cuda")
    poison = int(np.uint64(POISON64).astype(np.int64))
    hits = torch.full((cap + GUARD,), poison, dtype=torch.int64, device="cuda")
    spans = torch.full(((cap + GUARD) * 2,), poison, dtype=torch.int64, device="cuda")
    masks = torch.full((cap + GUARD,), poison, dtype=torch.int64, device="cuda")
    counts = torch.full((3,), poison, dtype=torch.int64, device="cuda")
    wm = t.want_mask(want)
    dw = None if wm is None else torch.as_tensor(wm.view(np.int64), device="cuda")
    assert t.mask_words == 1
    field, sep, rest = column
    stream = torch.cuda.current_stream().cuda_stream
    rp = d.data_ptr() + raw_off if size else 0
    if gather:
        out = torch.full((size + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out_offs = torch.full((cap + 1 + GUARD,), poison, dtype=torch.int64, device="cuda")
        t.run_lines_field_gather_device(rp, size, field, flags, counts.data_ptr(), counts.data_ptr() + 8, counts.data_ptr() + 16, sep=sep,
                                        rest=rest, want_ptr=0 if dw is None else dw.data_ptr(), out_hits_ptr=hits.data_ptr() if cap else 0,
                                        hit_cap=cap, out_text_ptr=out.data_ptr(), text_cap=size + cap, out_offsets_ptr=out_offs.data_ptr(),
                                        stream=stream)
    else:
        t.run_lines_field_select_device(rp, size, field, flags, counts.data_ptr(), counts.data_ptr() + 8, sep=sep, rest=rest,
                                        want_ptr=0 if dw is None else dw.data_ptr(), out_hits_ptr=hits.data_ptr() if cap else 0,
                                        out_hit_spans_ptr=spans.data_ptr() if cap else 0, out_hit_masks_ptr=masks.data_ptr() if cap else 0,
                                        hit_cap=cap, stream=stream)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64)
    k = min(int(c[1]), cap)
    h, s, m = (b.cpu().numpy().view(np.uint64) for b in (hits, spans, masks))
    assert (h[k:] == np.uint64(POISON64)).all()
    res = {"lines": int(c[0]), "count": int(c[1]), "hits": h[:k]}
    if gather:
        oo, ot = out_offs.cpu().numpy().view(np.uint64), out.cpu().numpy()
        total = int(c[2])
        assert (oo[k + 1:] == np.uint64(POISON64)).all() and (ot[total:] == 0xA5).all()
        res.update(text=ot[:total], offsets=oo[:k + 1], bytes=total)
    else:
        assert (s[2 * k:] == np.uint64(POISON64)).all() and (m[k:] == np.uint64(POISON64)).all()
        res.update(spans=s[:2 * k].reshape(k, 2), hit_masks=m[:k])
    return res


def check_select(got, exp, raw, cap=None):
    assert got["lines"] == exp["lines"] and got["count"] == exp["count"], (got["lines"], got["count"], exp["lines"], exp["count"])
    k = exp["count"] if cap is None else min(cap, exp["count"])
    assert len(got["hits"]) == k and (got["hits"] == exp["hits"][:k]).all()
    assert (got["hit_masks"].reshape(-1) == exp["hit_masks"][:k]).all()
    assert got["spans"].shape == (k, 2)
    assert [raw[int(b):int(e)].tobytes() for b, e in got["spans"]] == exp["bytes"][:k]       # the WHOLE lines


def check_gather(got, exp, cap=None, tail=b"\n"):
    assert got["lines"] == exp["lines"] and got["count"] == exp["count"]
    k = exp["count"] if cap is None else min(cap, exp["count"])
    assert len(got["hits"]) == k and (got["hits"] == exp["hits"][:k]).all()
    want = [b + tail for b in exp["bytes"][:k]]
    assert got["bytes"] == sum(len(b) for b in want) and bytes(got["text"]) == b"".join(want)
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(b) for b in want])]).astype(np.uint64).tolist()


@gpu
@pytest.mark.parametrize("name", ["set_a", "c2_single"])     # set_a: eight regexps glued into one scanner
def test_lines_whose_column_matches_against_oracle_and_restatement(torch_cuda, name):
    big = [b for b in H.big_sets() if b["name"] == name][0]
    blob = H.load_blob(big["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    raw, kinds, lines = column_raw(big, seed=77, last_terminated=(name == "set_a"))
    col = (FIELD, 9, False)
    full = expected(name, t, o, lines, col, BE, None)
    hit = np.zeros(LINES, dtype=bool)
    hit[full["hits"].astype(np.int64)] = True
    # what the oracle says about the kinds: planted columns hit, a witness in another column does not, noise does not
    assert hit[(kinds == 0) | (kinds == 1) | (kinds == 5)].all() and not hit[(kinds == 2) | (kinds == 3)].any()
    # ... and a whole-line scan would have selected the lines of kind 2
    wt, wo = H.pack(lines)
    assert np.asarray(o.run(wt, wo, flags=BE, threads=4)[1], dtype=bool)[kinds == 2].all()
    for flags in (0, pb.FLAG_BEGIN, pb.FLAG_END, BE):
        for want in (None, [0]):
            exp = expected(name, t, o, lines, col, flags, want)
            check_select(dev_field_select(torch_cuda, t, raw, col, flags, want, raw_off=flags), exp, raw)
    # too few columns: the empty field is scanned -- under every flag combination the lines of kind 4 go the way the empty string goes
    et, eo = H.pack([b""])
    for flags in (0, BE):
        exp = expected(name, t, o, lines, col, flags, None)
        got = np.zeros(LINES, dtype=bool)
        got[exp["hits"].astype(np.int64)] = True
        assert (got[kinds == 4] == bool(o.run(et, eo, flags=flags, threads=1)[1][0])).all()
    # REST, another column, a column no line has
    for column in ((FIELD, 9, True), (0, 9, False), (9, 9, False)):
        check_select(dev_field_select(torch_cuda, t, raw, column, BE), expected(name, t, o, lines, column, BE, None), raw)
    assert expected(name, t, o, lines, (0, 9, False), BE, None)["count"] >= (kinds == 2).sum()
    # room for fewer hits than there are; no room at all
    for cap in (full["count"] - 3, 1, 0):
        check_select(dev_field_select(torch_cuda, t, raw, col, BE, None, cap=cap), full, raw, cap=cap)
    assert pb.last_kernel() not in ("", None)
    # the gather form: the bytes of the whole lines, the delimiter behind each
    check_gather(dev_field_select(torch_cuda, t, raw, col, BE, gather=True, raw_off=3), full)
    check_gather(dev_field_select(torch_cuda, t, raw, col, BE, [0], cap=7, gather=True), expected(name, t, o, lines, col, BE, [0]), cap=7)
    # host pointers: the same answers
    check_select(t.run_lines_field_select_host(raw, FIELD), full, raw)
    check_select(t.run_lines_field_select_host(raw, FIELD, want=[0], hit_cap=5), expected(name, t, o, lines, col, BE, [0]), raw, cap=5)
    got = t.run_lines_field_gather_host(raw, FIELD)
    check_gather(got, full)
    got = t.run_lines_field_gather_host(raw, FIELD, rest=True, tail=None, hit_cap=9)
    check_gather(got, expected(name, t, o, lines, (FIELD, 9, True), BE, None), cap=9, tail=b"")


@gpu
def test_field_select_on_empty_and_delimiter_only_buffers(torch_cuda):
    big = [b for b in H.big_sets() if b["name"] == "c2_single"][0]
    blob = H.load_blob(big["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    col = (1, 9, False)
    for i, raw in enumerate((np.zeros(0, dtype=np.uint8), np.full(1, 10, dtype=np.uint8), np.full(T + 3, 10, dtype=np.uint8))):
        exp = expected("empty%d" % i, t, o, [b""] * len(raw), col, BE, None)
        assert exp["lines"] == len(raw) and exp["count"] == 0
        check_select(dev_field_select(torch_cuda, t, raw, col, BE, cap=4), exp, raw, cap=4)
        check_select(t.run_lines_field_select_host(raw, 1, hit_cap=4), exp, raw, cap=4)
        check_gather(dev_field_select(torch_cuda, t, raw, col, BE, cap=4, gather=True), exp, cap=4)
        check_gather(t.run_lines_field_gather_host(raw, 1, hit_cap=4), exp, cap=4)
    # a scanner that accepts the empty string: every line whose column is empty or missing is a hit; no final delimiter
    star = [c for c in H.all_cases() if c["name"] == "misc_1"][0]     # ^[^\s=/>]*$
    blob = H.load_blob(star["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    lines = [b""] * 70 + [b"a\txx", b"a\t", b"a", b"\t", b"a\tx y", b"", b"a\tb\tc d", b"q\tlast"]
    raw = u8(b"\n".join(lines))
    exp = expected("star", t, o, lines, col, BE, None)
    assert exp["count"] == 70 + 7 and 74 not in exp["hits"].tolist()
    check_select(dev_field_select(torch_cuda, t, raw, col, BE), exp, raw)
    check_gather(dev_field_select(torch_cuda, t, raw, col, BE, gather=True), exp)
    check_select(t.run_lines_field_select_host(raw, 1), exp, raw)
    exp = expected("star_rest", t, o, lines, (1, 9, True), BE, None)
    assert 76 not in exp["hits"].tolist()
    check_select(dev_field_select(torch_cuda, t, raw, (1, 9, True), BE), exp, raw)
