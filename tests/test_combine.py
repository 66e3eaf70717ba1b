"""pire_hip_combine and the two lines forms on top of it: boolean queries over hit lists -- grep a | grep -v b, two columns,
a Scanner term and a SlowScanner term on the same lines -- on the device (combine.hip).

Exact equality everywhere.  The expected values come from `model_combine` -- the formula of include/pire_hip.h written down
with numpy: np.isin per list, then the truth table lookup --, held against a hand-written table and, where there is one,
against grep a | grep -v b; for the lines forms it is applied to what the C oracle says of Python's own split and cut of every
line.  Nothing expected comes from the library (the route chain excepted, which is held against the masks of pire_hip_select,
an older pass with tests of its own).  Every output of a GPU call sits between poisoned guard bytes and is compared bytewise,
what the call had no business writing included."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
GUARD = 64                     # poisoned bytes around every output
EINVAL = -1
BE = ob.FLAG_BEGIN | ob.FLAG_END
ZERO = pb.FINAL_SELECT_ZERO
LINE = pb.TERM_LINE
gpu = pytest.mark.gpu
NAMES = ("pire_hip_combine", "pire_hip_lines_combine_select", "pire_hip_lines_combine_gather")
LINES_FORMS = NAMES[1:]


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def one(v):
    return np.array([v], dtype=np.uint64)


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_combine(lists, n, truth):
    """include/pire_hip.h: m(i) = sum of [i in list j] << j; selected(i) <=> (truth >> m(i)) & 1.  Hits, members, count."""
    i = np.arange(n, dtype=np.int64)
    m = np.zeros(n, dtype=np.int64)
    for j, l in enumerate(lists):
        m |= np.isin(i, np.asarray(l, dtype=np.int64)).astype(np.int64) << j
    table = np.array([(truth >> b) & 1 for b in range(1 << len(lists))], dtype=bool)
    hits = np.flatnonzero(table[m])
    return {"hits": hits.astype(np.uint64), "members": m[hits].astype(np.uint8), "count": int(hits.size)}


def model_context(hits, n, before, after):
    """pire_hip_context's formula (include/pire_hip.h), for the chain: the lines within `before` in front of or `after` behind a
    hit, and how many runs they form"""
    sel = np.zeros(n, dtype=bool)
    for h in np.asarray(hits, dtype=np.int64).tolist():
        sel[max(h - before, 0):h + after + 1] = True
    group = sel & ~np.concatenate([[False], sel[:-1]])
    return {"lines": np.flatnonzero(sel).astype(np.uint64), "count": int(sel.sum()), "groups": int(group.sum())}


def py_lines(raw, delim=b"\n"):
    """getline: the runs between delimiters; no extra empty line behind a trailing delimiter.  (lines, [begin, end) of every line)"""
    parts = bytes(raw).split(delim)
    if parts and parts[-1] == b"":
        parts.pop()
    spans, pos = [], 0
    for s in parts:
        spans.append((pos, pos + len(s)))
        pos += len(s) + 1
    return parts, np.array(spans, dtype=np.uint64).reshape(-1, 2)


def py_column(line, column, sep=b"\t", rest=False):
    """cut -f column+1 (rest: column+1-): a line with too few separators has an empty column"""
    parts = line.split(sep)
    if column >= len(parts):
        return b""
    return sep.join(parts[column:]) if rest else parts[column]


# (lists, n, truth) -> (hits, members)
TABLE = [
    (([[1, 3]], 5, 0b10), ([1, 3], [1, 1])),                                      # truth = 2 gives the list back
    (([[1, 3]], 5, 0b01), ([0, 2, 4], [0, 0, 0])),                                # truth = 1: the complement, grep -v
    (([[1, 3]], 5, 0b11), ([0, 1, 2, 3, 4], [0, 1, 0, 1, 0])),
    (([[1, 3]], 5, 0b00), ([], [])),
    (([[1, 3]], 5, 0b110), ([1, 3], [1, 1])),                                     # bits at or above 2^k are ignored
    (([[0, 1, 2], [1, 2, 3]], 5, 0b1000), ([1, 2], [3, 3])),                      # and
    (([[0, 1, 2], [1, 2, 3]], 5, 0b1110), ([0, 1, 2, 3], [1, 3, 3, 2])),          # or
    (([[0, 1, 2], [1, 2, 3]], 5, 0b0010), ([0], [1])),                            # a and not b
    (([[0, 1, 2], [1, 2, 3]], 5, 0b0110), ([0, 3], [1, 2])),                      # xor
    (([[0, 1, 2], [1, 2, 3]], 5, 0b0001), ([4], [0])),                            # neither
    (([[], []], 3, 0b0001), ([0, 1, 2], [0, 0, 0])),                              # all lists empty, bit 0: every line
    (([[], []], 3, 0b1110), ([], [])),
    (([[2], [2]], 4, 0b1000), ([2], [3])),                                        # the same list twice
    (([[2], [2]], 4, 0b0110), ([], [])),
    (([[0], [1], [2]], 4, 0b00010110), ([0, 1, 2], [1, 2, 4])),                   # exactly one of three
    (([[5]], 0, 0b11), ([], [])),                                                 # no lines
]


def test_the_model_against_a_hand_written_table():
    for (lists, n, truth), (hits, members) in TABLE:
        got = model_combine(lists, n, truth)
        assert got["hits"].tolist() == hits and got["members"].tolist() == members and got["count"] == len(hits), (lists, n, truth)
    assert py_column(b"a\tb\tc", 1) == b"b" and py_column(b"a\tb\tc", 1, rest=True) == b"b\tc" and py_column(b"a", 1) == b"" and py_column(b"", 0) == b""
    assert pb.truth(2, lambda m: m == 1) == 0b0010 and pb.truth(1, lambda m: not m) == 1 and pb.truth(3, lambda m: bin(m).count("1") == 1) == 0b00010110
    assert pb.truth(6, lambda m: True) == (1 << 64) - 1
    for k in (0, 7):
        with pytest.raises(ValueError):
            pb.truth(k, lambda m: True)


@pytest.mark.skipif(shutil.which("grep") is None, reason="no grep")
def test_the_model_against_grep_a_then_grep_v_b(tmp_path):
    rng = np.random.RandomState(11)
    text = [b"line %d%s%s" % (i, b" alpha" if rng.randint(2) else b"", b" beta" if rng.randint(3) == 0 else b"") for i in range(200)]
    path = tmp_path / "lines.txt"
    path.write_bytes(b"\n".join(text) + b"\n")
    a = [i for i, s in enumerate(text) if b"alpha" in s]
    b = [i for i, s in enumerate(text) if b"beta" in s]
    first = subprocess.run(["grep", "alpha", str(path)], stdout=subprocess.PIPE, check=True).stdout
    out = subprocess.run(["grep", "-v", "beta"], input=first, stdout=subprocess.PIPE, check=True).stdout
    exp = model_combine([a, b], 200, pb.truth(2, lambda m: m == 1))
    assert 10 < exp["count"] < 190 and out == b"".join(text[i] + b"\n" for i in exp["hits"].tolist())
    out = subprocess.run(["grep", "-v", "alpha", str(path)], stdout=subprocess.PIPE, check=True).stdout
    assert out == b"".join(text[i] + b"\n" for i in model_combine([a], 200, 1)["hits"].tolist())


# ---- CPU: the surface and what it refuses -----------------------------------------------------------------------------------------

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
    assert re.search(r"#define PIRE_HIP_COMBINE_MAX_LISTS +6u", src) and re.search(r"#define PIRE_HIP_TERM_LINE +\(~0u\)", src)
    assert "typedef struct pire_hip_line_term {" in src
    assert (pb.COMBINE_MAX_LISTS, pb.TERM_LINE) == (6, 0xFFFFFFFF)
    assert C.sizeof(pb.LineTerm) == 48                    # three pointers, five 32-bit words, padded to the pointers' alignment
    assert "combine" not in " ".join(pb.selftested_kernels()).lower()
    for name in ("combine_host", "combine_device", "lines_combine_host", "lines_combine_device", "truth"):
        assert callable(getattr(pb, name)), name


def _guarded(names=("hits", "members", "spans", "text", "offsets", "terms")):
    return {k: np.full(256, POISON, dtype=np.uint8) for k in names}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def _arrays(ptrs, counts, caps):
    k = max(len(ptrs), len(caps), 1)
    return ((C.c_void_p * k)(*ptrs), None if counts is None else (C.c_void_p * k)(*counts), (C.c_uint64 * k)(*caps))


def test_combine_refuses_before_any_device_is_touched():
    L = pb.lib()
    a, b = u64([1, 4, 6]), u64([2, 4])
    bufs, cnt = _guarded(), C.c_uint64(77)
    o, m, c = bufs["hits"].ctypes.data, bufs["members"].ctypes.data, C.addressof(cnt)
    pa, pb_ = a.ctypes.data, b.ctypes.data
    two = _arrays([pa, pb_], None, [3, 2])
    seven = _arrays([pa] * 7, None, [3] * 7)
    # (lists, list_counts, list_caps, k_lists, n, out_hits, out_hit_members, hit_cap, out_hit_count)
    cases = {
        "k_lists == 0": (two[0], None, two[2], 0, 8, o, m, 4, c),
        "more than 6 lists": (seven[0], None, seven[2], 7, 8, o, m, 4, c),
        "null lists": (None, None, two[2], 2, 8, o, m, 4, c),
        "null list_caps": (two[0], None, None, 2, 8, o, m, 4, c),
        "list_caps[1] > 0 with null lists[1]": (_arrays([pa, None], None, [3, 2])[0], None, two[2], 2, 8, o, m, 4, c),
        "null out_hit_count": (two[0], None, two[2], 2, 8, o, m, 4, None),
        "hit_cap > 0 with null out_hits": (two[0], None, two[2], 2, 8, None, None, 4, c),
        "out_hit_members without out_hits": (two[0], None, two[2], 2, 8, None, m, 0, c),
        "2^32 lines or more": (two[0], None, two[2], 2, 1 << 32, o, m, 4, c),
        "2^32 entries or more in list 1": (two[0], None, _arrays([], None, [3, 1 << 32])[2], 2, 8, o, m, 4, c),
    }
    for what, (a_l, a_k, a_c, k, n, a_o, a_m, cap, a_cnt) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            for truth in (0b0010, (1 << 64) - 1):
                assert L.pire_hip_combine(a_l, a_k, a_c, k, n, truth, flags, a_o, a_m, cap, a_cnt, None) == EINVAL, what
                msg = L.pire_hip_last_error().decode()
                assert what in msg and msg.startswith("pire_hip_combine: "), (what, msg)
    # host pointers: the lists themselves, before anything is written (k_j follows *list_counts[j] where it is smaller)
    for what, bad, n in (("list 1 must be strictly ascending", [4, 1, 6], 8), ("list 1 must be strictly ascending", [1, 1, 6], 8),
                         ("list 1 names a line out of range", [1, 4, 8], 8), ("list 1 names a line out of range", [0], 0)):
        bad = u64(bad)
        arr = _arrays([pa, bad.ctypes.data], None, [0 if n == 0 else 3, len(bad)])
        assert L.pire_hip_combine(arr[0], None, arr[2], 2, n, 0b1110, 0, o, m, 4, c, None) == EINVAL, what
        msg = L.pire_hip_last_error().decode()
        assert what in msg and msg.startswith("pire_hip_combine: "), (what, msg)
    assert cnt.value == 77 and _untouched(bufs)
    # no lines -- and a count of 0 in front of a list that would be refused --: a count of 0, and no device
    none, nines = C.c_uint64(0), u64([9, 9])
    arr = _arrays([nines.ctypes.data], [C.addressof(none)], [2])
    for a_l, a_k, a_c in ((arr[0], arr[1], arr[2]), (_arrays([None], None, [0])[0], None, _arrays([], None, [0])[2])):
        cnt.value = 77
        assert L.pire_hip_combine(a_l, a_k, a_c, 1, 0, 3, 0, o, m, 4, c, None) == 0, L.pire_hip_last_error()
        assert cnt.value == 0 and _untouched(bufs)
    with pytest.raises(pb.PireHipError, match="strictly ascending"):   # (the wrappers raise what the library refuses)
        pb.combine_host([[3, 2]], 10, 2)
    got = pb.combine_host([[], []], 0, 1)
    assert got["count"] == 0 and got["hits"].size == 0 and got["members"].size == 0


def _slow_blob(name):
    return H.load_blob([c for c in H.golden()["slow"] if c["name"] == name][0]["blob"])


def _big(name):
    big = [b for b in H.big_sets() if b["name"] == name][0]
    return big, H.load_blob(big["blob"])


_tables = {}


def table_of(name):
    if name not in _tables:
        _tables[name] = pb.SlowTable(_slow_blob(name)) if name.startswith("slow_") else pb.Table(_big(name)[1])
    return _tables[name]


def lines_form(who, terms, truth, raw_ptr, size, delim, flags, a_n, a_hits, a_spans, a_members, cap, a_cnt, a_terms, gather, stream=None):
    """one of the two C calls; gather: (tail, out_text, text_cap, out_offsets, out_bytes) in the _gather form"""
    assert who.endswith("gather") == (gather is not None)
    arr = None if terms is None else (pb.LineTerm * max(len(terms), 1))(*terms)
    return getattr(pb.lib(), who)(arr, 0 if terms is None else len(terms), truth, raw_ptr, size, delim, flags, a_n, a_hits, a_spans, a_members, cap,
                                  a_cnt, a_terms, *(tuple(gather) if gather else ()), stream)


def test_the_lines_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"ab" * 20 + b"\nb\n").copy()
    fast, slow = table_of("set_a"), table_of("slow_a30")
    good = [pb.line_term(table=fast), pb.line_term(slow_table=slow, invert=True, column=2)]
    bufs = _guarded()
    n, cnt, total = (C.c_uint64(70 + k) for k in range(3))
    r, o, s, m, tc = raw.ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, bufs["members"].ctypes.data, bufs["terms"].ctypes.data
    np_, cp, bp = (C.addressof(v) for v in (n, cnt, total))
    x, xo = bufs["text"].ctypes.data, bufs["offsets"].ctypes.data
    both = pb.line_term(table=fast, slow_table=slow)
    for who in LINES_FORMS:
        gathers = who.endswith("gather")
        ok_g = (10, x, 32, xo, bp) if gathers else None
        # (terms, raw, size, delim, out_line_count, out_hits, out_hit_spans, out_hit_members, hit_cap, out_hit_count, gather)
        cases = {
            "null terms": (None, r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "k_terms == 0": ([], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "more than 6 terms": (good * 4, r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "term 1: both table and slow_table": ([good[0], both], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "term 0: neither table nor slow_table": ([pb.line_term(), good[1]], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "term 1: sep == delim": ([good[0], pb.line_term(table=fast, column=0, sep=10)], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "sep > 255": ([pb.line_term(table=fast, column=0, sep=256)], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "delim > 255": (good, r, raw.size, 256, np_, o, s, m, 4, cp, ok_g),
            "null out_line_count": (good, r, raw.size, 10, None, o, s, m, 4, cp, ok_g),
            "size > 0 with null raw": (good, None, raw.size, 10, np_, o, s, m, 4, cp, ok_g),
            "null out_hit_count": (good, r, raw.size, 10, np_, o, s, m, 4, None, ok_g),
            "out_hit_members without out_hits": (good, r, raw.size, 10, np_, None, None, m, 0, cp, ok_g),
            "out_hit_spans without out_hits": (good, r, raw.size, 10, np_, None, s, None, 0, cp, ok_g),
        }
        bad_mode, bad_field, bad_flags = pb.line_term(slow_table=slow), pb.line_term(table=fast, column=1), pb.line_term(table=fast)
        bad_mode.mode, bad_field.field_mode, bad_flags.run_flags = 2, 2, BE | pb.FLAG_ON_DEVICE
        cases["term 1: unknown mode"] = ([good[0], bad_mode], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g)
        cases["unknown bits in mode"] = ([bad_field], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g)
        cases["term 0: unknown bits in run_flags"] = ([bad_flags], r, raw.size, 10, np_, o, s, m, 4, cp, ok_g)
        if gathers:
            cases.update({
                "null out_bytes": (good, r, raw.size, 10, np_, o, s, m, 4, cp, (10, x, 32, xo, None)),
                "tail > 255": (good, r, raw.size, 10, np_, o, s, m, 4, cp, (256, x, 32, xo, bp)),
                "idx_cap > 0 with null out_offsets (idx_cap = hit_cap)": (good, r, raw.size, 10, np_, o, s, m, 4, cp, (10, x, 32, None, bp)),
                "text_cap > 0 with null out_text": (good, r, raw.size, 10, np_, o, s, m, 4, cp, (10, None, 32, xo, bp)),
                "out_text overlaps the source": (good, r, raw.size, 10, np_, o, s, m, 4, cp, (10, r + 8, 16, xo, bp)),
            })
        else:
            cases["hit_cap > 0 with null out_hits"] = (good, r, raw.size, 10, np_, None, None, None, 4, cp, ok_g)
        for what, (terms, a_r, size, delim, a_n, a_o, a_s, a_m, cap, a_cnt, g) in cases.items():
            for flags in (0, pb.FLAG_ON_DEVICE):
                rc = lines_form(who, terms, 0b10, a_r, size, delim, flags, a_n, a_o, a_s, a_m, cap, a_cnt, tc, g)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (who, what, rc, msg)
        # BEGIN / END are each term's own: the call's flags carry PIRE_HIP_RUN_ON_DEVICE and nothing else
        for flags in (BE, BE | pb.FLAG_ON_DEVICE):
            rc = lines_form(who, good, 0b10, r, raw.size, 10, flags, np_, o, s, m, 4, cp, tc, ok_g)
            msg = L.pire_hip_last_error().decode()
            assert rc == EINVAL and "flags other than PIRE_HIP_RUN_ON_DEVICE" in msg and msg.startswith(who + ": "), (who, rc, msg)
    assert [v.value for v in (n, cnt, total)] == [70, 71, 72] and _untouched(bufs)
    assert (raw == u8(b"ab" * 20 + b"\nb\n")).all()


def test_empty_host_buffers_answer_zeros_without_a_device():
    terms = [pb.line_term(table=table_of("set_a"), column=1), pb.line_term(slow_table=table_of("slow_a30"), invert=True)]
    for who in LINES_FORMS:
        for truth in (0b0001, 0b1000):
            bufs = _guarded()
            n, cnt, total = (C.c_uint64(70 + k) for k in range(3))
            g = (10, bufs["text"].ctypes.data, 32, bufs["offsets"].ctypes.data, C.addressof(total)) if who.endswith("gather") else None
            rc = lines_form(who, terms, truth, None, 0, 10, 0, C.addressof(n), bufs["hits"].ctypes.data, bufs["spans"].ctypes.data,
                            bufs["members"].ctypes.data, 4, C.addressof(cnt), bufs["terms"].ctypes.data, g)
            assert rc == 0, pb.lib().pire_hip_last_error()
            assert [v.value for v in (n, cnt)] == [0, 0]
            assert bufs["terms"].view(np.uint64)[:2].tolist() == [0, 0] and (bufs["terms"][16:] == POISON).all()
            bufs["terms"][:16] = POISON
            if g:
                assert total.value == 0 and bufs["offsets"].view(np.uint64)[0] == 0 and (bufs["offsets"][8:] == POISON).all()
                bufs["offsets"][:8] = POISON
            assert _untouched(bufs)
    got = pb.lines_combine_host(terms, 1, b"", gather=True)   # the wrapper on nothing
    assert (got["lines"], got["count"], got["bytes"]) == (0, 0, 0) and got["offsets"].tolist() == [0] and got["term_counts"].tolist() == [0, 0]
    assert got["hits"].size == 0 and got["spans"].shape == (0, 2) and got["members"].size == 0


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """combine.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "combine.hip" in ba.NO_SCRATCH and "combine.hip" in ba.UNITS and "combine" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bcombine\.hip\b", mk)) == 2                            # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("combine.hip")
    assert not fails, fails
    assert len(seen) == 2 and all("Combine" in k for k in seen), seen              # classify, scatter


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "combine.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "asm" not in src
    assert "atomic" not in src.lower().replace("no atomics", "").replace("no atomic", "")
    # its own classify kernel between the shared launcher's front and tail, the shared search and stage
    for shared in ('#include "tile_pass.h"', "TilePass t(", "t.Front(", "TileBallot(", "t.Tail(", "WaveBound<false>(", "LoadU64(",
                   "list.Count(", "list.List(", "list.Back()"):
        assert shared in src, shared
    assert "BlockExclusive" not in src                                             # (the scan is select.hip's, not a copy)
    assert src.count("__global__") == 1 and src.count("hipLaunchKernelGGL") == 1   # (the classify kernel; the scatter is the shared one)
    for copy in ("TileRank(", "TileCompaction(", "LaunchTileScan(", "__shfl", "__ballot", "UnalignedU64", "hipGetLastError", "hipMemcpyDeviceToHost"):
        assert copy not in src, copy


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class Outs:
    """The outputs of one call, host or device, each `bytes` long between GUARD poisoned bytes (and `shift` bytes further in,
    for an output off its natural alignment); check() compares every one of them bytewise with what the model says the call
    writes -- and leaves alone."""

    def __init__(self, torch, device, sizes, shift=None):
        self.torch, self.device, self.shift = torch, device, shift or {}
        self.host = {k: np.full(2 * GUARD + s + 8, POISON, dtype=np.uint8) for k, s in sizes.items() if s is not None}
        self.dev = {k: torch.as_tensor(v, device="cuda") for k, v in self.host.items()} if device else {}

    def ptr(self, name):
        if name not in self.host:
            return None
        return (self.dev[name].data_ptr() if self.device else self.host[name].ctypes.data) + GUARD + self.shift.get(name, 0)

    def put(self, name, payload):
        payload = u8(np.ascontiguousarray(payload).tobytes()).copy()
        at = GUARD + self.shift.get(name, 0)
        if self.device:
            self.dev[name][at:at + len(payload)] = self.torch.as_tensor(payload, device="cuda")
        else:
            self.host[name][at:at + len(payload)] = payload

    def read(self):
        if self.device:
            self.torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in self.dev.items()}
        return {k: v.copy() for k, v in self.host.items()}

    def check(self, want, what=""):
        """want: the payload of every output"""
        now = self.read()
        assert set(want) >= set(now), (set(now), set(want))
        for name, got in now.items():
            payload = want[name] if isinstance(want[name], bytes) else np.ascontiguousarray(want[name]).tobytes()
            full = np.full(len(got), POISON, dtype=np.uint8)
            at = GUARD + self.shift.get(name, 0)
            full[at:at + len(payload)] = u8(payload)
            bad = np.flatnonzero(got != full)
            assert bad.size == 0, (what, name, "first differing byte %d of %d (payload %d bytes)" % (bad[0] - at, len(got) - 2 * GUARD - 8, len(payload)))
        return now


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream or None


class Hits:
    """a hit list on the host and on the device, `shift` bytes off its natural alignment, poisoned around"""

    def __init__(self, torch, hits, shift=0):
        hits = u64(hits)
        self.hits, self.k = hits, len(hits)
        self.room = np.full(8 * self.k + 2 * GUARD, POISON, dtype=np.uint8)
        lead = (-self.room.ctypes.data) % 8 + 8 + shift
        self.room[lead:lead + 8 * self.k] = hits.view(np.uint8)
        self.host = self.room.ctypes.data + lead
        self.dev_room = torch.full((8 * self.k + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.dev_lead = (-self.dev_room.data_ptr()) % 8 + 8 + shift
        self.dev_room[self.dev_lead:self.dev_lead + 8 * self.k] = torch.as_tensor(hits.view(np.uint8).copy(), device="cuda")
        self.dev = self.dev_room.data_ptr() + self.dev_lead
        assert self.host % 8 == shift % 8 == self.dev % 8

    def ptr(self, device):
        return (self.dev if device else self.host) if self.k else None

    def intact(self):
        got = self.dev_room.cpu().numpy()
        assert got[self.dev_lead:self.dev_lead + 8 * self.k].tobytes() == self.hits.tobytes(), "the list was written to"
        assert (got[:self.dev_lead] == POISON).all() and (got[self.dev_lead + 8 * self.k:] == POISON).all(), "the list's surroundings were written to"


def call_pass(torch, device, hls, n, truth, hit_cap, counts=None, caps=None, hits=True, members=True, members_shift=0):
    """pire_hip_combine on Hits lists; counts: None (a null list_counts), or one entry per list (None: a null pointer).  (rc, Outs)"""
    k = len(hls)
    sizes = {"count": 8, "hits": 8 * hit_cap if hits else None, "members": hit_cap if hits and members else None}
    for j in range(k):
        sizes["k%d" % j] = 8 if counts is not None and counts[j] is not None else None
    out = Outs(torch, device, sizes, {"members": members_shift})
    for j in range(k):
        if sizes["k%d" % j]:
            out.put("k%d" % j, one(counts[j]))
    arr = _arrays([h.ptr(device) for h in hls], None if counts is None else [out.ptr("k%d" % j) for j in range(k)],
                  [h.k for h in hls] if caps is None else caps)
    rc = pb.lib().pire_hip_combine(arr[0], arr[1], arr[2], k, n, truth, pb.FLAG_ON_DEVICE if device else 0, out.ptr("hits") if hit_cap else None,
                                   out.ptr("members") if hit_cap else None, hit_cap if hits else 0, out.ptr("count"),
                                   stream_of(torch) if device else None)
    return rc, out


def run_pass(torch, device, hls, n, truth, hit_cap, exp, what, counts=None, caps=None, hits=True, members=True, members_shift=0):
    """... and its outputs against exp -- the model's answer for the k_j the call was given"""
    rc, out = call_pass(torch, device, hls, n, truth, hit_cap, counts, caps, hits, members, members_shift)
    assert rc == 0, (what, pb.lib().pire_hip_last_error())
    m = min(exp["count"], hit_cap)
    want = {"count": one(exp["count"]), "hits": exp["hits"][:m], "members": exp["members"][:m]}
    for j in range(len(hls)):
        if counts is not None and counts[j] is not None:
            want["k%d" % j] = one(counts[j])
    return out.check(want, what)


# ---- GPU: the pass alone -----------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 17)


def hit_lists(n):
    rng = np.random.RandomState(n)
    lists = {"empty": [], "every line": np.arange(n), "tile edges": [h for h in (1023, 1024, 2047, 2048) if h < n], "only line n - 1": [n - 1]}
    for d in (2, 7, 50):
        lists["density 1/%d" % d] = np.flatnonzero(rng.randint(0, d, size=n) == 0)
    return lists


def random_truth(rng, k):
    return int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32) if k == 6 else int(rng.randint(0, 1 << (1 << k)))


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_pass_alone_from_host_pointers_and_on_the_device(torch_cuda, n):
    """k_lists = 1 .. 6 drawn from the seven kinds of list, under seeded truth tables (k = 1: all four)"""
    torch = torch_cuda
    pool = hit_lists(n)
    hls = {name: Hits(torch, l) for name, l in pool.items()}
    names = list(pool)
    rng = np.random.RandomState(7 * n)
    calls = 0
    for name in names:                                             # every kind of list alone: itself, its complement, all, none
        for truth in range(4):
            exp = model_combine([pool[name]], n, truth)
            if truth == 2:
                assert exp["hits"].tolist() == list(pool[name])
            for device in (True, False):
                run_pass(torch, device, [hls[name]], n, truth, n, exp, (n, name, truth, device))
                calls += 1
    for k in range(2, 7):
        for _ in range(3):
            pick = [names[j] for j in rng.randint(0, len(names), size=k)]
            truth = random_truth(rng, k)
            exp = model_combine([pool[p] for p in pick], n, truth)
            for device in (True, False):
                run_pass(torch, device, [hls[p] for p in pick], n, truth, n, exp, (n, pick, hex(truth), device))
                calls += 1
    # all lists empty: every line under bit 0, none without it; bits at or above 2^k are not looked at
    for k in (1, 3, 6):
        for truth, count in ((1, n), (((1 << 64) - 1) & ~1, 0), (1 | (1 << (1 << k) if k < 6 else 0), n)):
            exp = model_combine([[]] * k, n, truth & ((1 << (1 << k)) - 1))
            assert exp["count"] == count
            run_pass(torch, True, [hls["empty"]] * k, n, truth, n, exp, (n, "empty", k, hex(truth)))
    for hl in hls.values():
        hl.intact()
    assert calls == 7 * 4 * 2 + 5 * 3 * 2


@gpu
def test_no_lines_from_host_pointers_and_on_the_device(torch_cuda):
    """n == 0: a count of 0 under any truth table, whatever the capacity; no list is touched, on either side.  On the device a
    list may stand there all the same (nothing of it is read)."""
    torch = torch_cuda
    empty, some = Hits(torch, []), Hits(torch, [0, 5, 9])
    for k in (1, 3, 6):
        for truth in (1, 2, (1 << (1 << k)) - 1):
            exp = model_combine([[]] * k, 0, truth)
            assert exp["count"] == 0
            for hit_cap in (0, 4):
                for members in (True, False):
                    for device in (True, False):
                        run_pass(torch, device, [empty] * k, 0, truth, hit_cap, exp, (k, hex(truth), hit_cap, members, device), members=members)
                    run_pass(torch, True, [some] + [empty] * (k - 1), 0, truth, hit_cap, exp, (k, hex(truth), hit_cap, members, "a list"), members=members)
    empty.intact()
    some.intact()


@gpu
def test_every_truth_table_of_one_and_two_lists(torch_cuda):
    torch = torch_cuda
    n = 1025
    rng = np.random.RandomState(3)
    a, b = (np.flatnonzero(rng.randint(0, 3, size=n) == 0) for _ in range(2))
    ha, hb = Hits(torch, a), Hits(torch, b)
    seen = set()
    for truth in range(16):
        exp = model_combine([a, b], n, truth)
        seen.add(exp["count"])
        for device in (True, False):
            run_pass(torch, device, [ha, hb], n, truth, n, exp, ("two", truth, device))
    assert len(seen) > 8 and 0 in seen and n in seen
    for truth in range(4):
        exp = model_combine([a], n, truth)
        for device in (True, False):
            run_pass(torch, device, [ha], n, truth, n, exp, ("one", truth, device))
    # the same pointer twice: masks 1 and 2 do not occur
    for truth, like in ((0b1000, 2), (0b0110, 0), (0b0001, 1), (0b1001, 3)):
        exp = model_combine([a, a], n, truth)
        assert exp["hits"].tolist() == model_combine([a], n, like)["hits"].tolist()
        for device in (True, False):
            run_pass(torch, device, [ha, ha], n, truth, n, exp, ("twice", truth, device))


@gpu
def test_counts_caps_and_k(torch_cuda):
    torch = torch_cuda
    n = 2049
    rng = np.random.RandomState(5)
    a, b, c = (np.flatnonzero(rng.randint(0, d, size=n) == 0) for d in (2, 3, 40))
    hls = [Hits(torch, l) for l in (a, b, c)]
    truth = pb.truth(3, lambda m: m in (1, 3, 6, 7))
    exp = model_combine([a, b, c], n, truth)
    count = exp["count"]
    assert 100 < count < n - 100 and len(set(exp["members"].tolist())) == 4
    for device in (True, False):
        for cap in (0, 1, count - 1, count, count + 5):
            run_pass(torch, device, hls, n, truth, cap, exp, ("cap", cap, device))
        # the count only (null out_hits, with and without a hit_cap of 0), hits without members
        run_pass(torch, device, hls, n, truth, 0, exp, ("count only", device), hits=False)
        run_pass(torch, device, hls, n, truth, count, exp, ("no members", device), members=False)
        # k_j: *list_counts[j] where it is smaller than the cap, the cap where it is not, the cap where there is no pointer
        ha, hb = len(a) // 2, len(b) // 3
        part = model_combine([a[:ha], b, c], n, truth)
        run_pass(torch, device, hls, n, truth, n, part, ("k = *count", device), counts=[ha, len(b), None])
        run_pass(torch, device, hls, n, truth, n, part, ("k = cap", device), counts=[len(a) + 7, len(b) + 1, len(c)], caps=[ha, len(b), len(c)])
        run_pass(torch, device, hls, n, truth, n, part, ("no counts", device), caps=[ha, len(b), len(c)])
        part = model_combine([a[:ha], b[:hb], []], n, truth)
        run_pass(torch, device, hls, n, truth, n, part, ("mixed", device), counts=[None, hb, 0], caps=[ha, len(b), len(c)])
    # the wrappers, and the same input twice: the same bytes
    w = pb.combine_host([a, b, c], n, truth, hit_cap=5)
    assert w["count"] == count and (w["hits"] == exp["hits"][:5]).all() and (w["members"] == exp["members"][:5]).all()
    w = pb.combine_host([a, b, c], n, truth, list_counts=[len(a) // 2, None, len(c)])
    assert w["count"] == model_combine([a[:len(a) // 2], b, c], n, truth)["count"]
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    lists = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    marks = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    for k in range(2):
        pb.combine_device([h.dev for h in hls], [h.k for h in hls], n, truth, cnt[k:].data_ptr(), out_hits_ptr=lists[k].data_ptr(),
                          out_hit_members_ptr=marks[k].data_ptr(), hit_cap=n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [count] * 2
    assert (lists.cpu().numpy()[:, :count] == exp["hits"].astype(np.int64)).all() and (marks.cpu().numpy()[:, :count] == exp["members"]).all()
    for hl in hls:
        hl.intact()


@gpu
def test_host_pointers_refuse_a_list_that_is_not_ascending_or_out_of_range(torch_cuda):
    n = 1500
    good = Hits(torch_cuda, [5, 7, 1400])
    for bad in ([5, 900, 899, 1400], [5, 900, 900, 1400], [5, 900, 1400, n]):
        rc, out = call_pass(torch_cuda, False, [good, Hits(torch_cuda, bad)], n, 0b0110, n)
        assert rc == EINVAL and pb.lib().pire_hip_last_error().decode().startswith("pire_hip_combine: list 1 "), bad
        out.check({"count": b"", "hits": b"", "members": b""}, bad)
    # the same list one entry shorter is fine
    run_pass(torch_cuda, False, [good, Hits(torch_cuda, [5, 900, 1400])], n, 0b0110, n, model_combine([[5, 7, 1400], [5, 900, 1400]], n, 0b0110), "ascending")


@gpu
def test_a_list_that_does_not_ascend_on_the_device_harms_nothing(torch_cuda):
    """device pointers look at no list: the selection is unspecified, the guards hold, the call returns"""
    torch = torch_cuda
    n = 3 * 1024 + 17
    rng = np.random.RandomState(9)
    good = Hits(torch, np.flatnonzero(rng.randint(0, 3, size=n) == 0))
    for bad in (rng.randint(0, n, size=2000), np.arange(n)[::-1], np.full(1500, 1024), rng.randint(0, 1 << 62, size=500), [n, n + 1, 1 << 40]):
        hb = Hits(torch, bad)
        for truth in (0b0110, 0b1001):
            rc, out = call_pass(torch, True, [good, hb], n, truth, n)
            assert rc == 0, pb.lib().pire_hip_last_error()
            now = out.read()
            count = int(now["count"][GUARD:GUARD + 8].view(np.uint64)[0])
            assert count <= n
            for name, payload in (("count", 8), ("hits", 8 * count), ("members", count)):
                assert (now[name][:GUARD] == POISON).all() and (now[name][GUARD + payload:] == POISON).all(), (name, "guard")
            got = now["hits"][GUARD:GUARD + 8 * count].view(np.uint64)
            assert (got < n).all() and (np.diff(got.astype(np.int64)) > 0).all()      # (what any compaction gives: ascending line numbers)
        hb.intact()
    good.intact()


@gpu
@pytest.mark.parametrize("shift", range(1, 8))
def test_misaligned_lists_and_members(torch_cuda, shift):
    n = 1025
    rng = np.random.RandomState(shift)
    a, b = (np.flatnonzero(rng.randint(0, 4, size=n) == 0) for _ in range(2))
    hls = [Hits(torch_cuda, a, shift=shift), Hits(torch_cuda, b, shift=8 - shift)]
    for truth in (0b0110, 0b1011):
        exp = model_combine([a, b], n, truth)
        for device in (True, False):
            run_pass(torch_cuda, device, hls, n, truth, n, exp, (shift, truth, device), members_shift=shift)
    for hl in hls:
        hl.intact()


@gpu
def test_more_tiles_than_the_launch_has_blocks(torch_cuda):
    """8 193 full tiles and five lines: the blocks of the grid-stride loop walk a second tile, the last tile is short"""
    torch = torch_cuda
    n = 8193 * 1024 + 5
    rng = np.random.RandomState(8193)
    pool = np.unique(np.concatenate([rng.randint(0, n, size=6000), [0, 1023, 1024, 8191 * 1024 - 1, 8192 * 1024 - 1, 8192 * 1024, n - 2, n - 1]]))
    lists = [pool[rng.randint(0, 2, size=pool.size) == 1] for _ in range(3)]
    lists[0] = np.union1d(lists[0], [n - 1, 8192 * 1024])             # the last tile: line n - 1 under mask 3, its first line under mask 1
    lists[1] = np.setdiff1d(np.union1d(lists[1], [n - 1]), [8192 * 1024])
    lists[2] = np.setdiff1d(lists[2], [n - 1, 8192 * 1024])
    truth = pb.truth(3, lambda m: m in (1, 3, 6))
    exp = model_combine(lists, n, truth)
    assert 1000 < exp["count"] < 6000 and exp["hits"][-1] == n - 1 and (exp["hits"] >= 8192 * 1024).sum() >= 2
    hls = [Hits(torch, l) for l in lists]
    for device in (True, False):
        run_pass(torch, device, hls, n, truth, 6000, exp, ("many tiles", device))
    # the complement of one sparse list, counted only
    run_pass(torch, True, hls[:1], n, 1, 0, {"count": n - len(lists[0]), "hits": u64([]), "members": u8(b"")}, "complement, count only", hits=False)


# ---- GPU: chains, device pointers, no read-back in between ----------------------------------------------------------------------

@gpu
def test_route_rows_into_combine_against_the_masks_of_select(torch_cuda):
    """pire_hip_route's rows r and s as they are -- out_hits + r * hit_cap, out_hit_counts + r -- into "r and not s" """
    torch = torch_cuda
    case = [c for c in H.all_cases() if c["name"] == "glue_ccc_aaa_bbb"][0]
    tab = pb.Table(H.load_blob(case["blob"]))
    strings = H.random_strings(np.random.RandomState(21), 3000, 14, b"abcx")
    text, offs = H.pack(strings)
    n, cap = len(strings), len(strings)
    masks = tab.run_select(text, offs, flags=BE)["masks"][:, 0]
    stream = torch.cuda.current_stream().cuda_stream
    d_text = torch.as_tensor(np.array(text), device="cuda")
    d_offs = torch.as_tensor(offs.view(np.int64), device="cuda")
    d_rows = torch.zeros((3, cap), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    tab.run_route_device(d_text.data_ptr(), d_offs.data_ptr(), n, BE, d_counts.data_ptr(), out_hits_ptr=d_rows.data_ptr(), hit_cap=cap, stream=stream)
    for r, s in ((1, 2), (2, 1), (0, 1)):
        out = Outs(torch, True, {"count": 8, "hits": 8 * n, "members": n})
        pb.combine_device([d_rows.data_ptr() + 8 * r * cap, d_rows.data_ptr() + 8 * s * cap], [cap, cap], n, pb.truth(2, lambda m: m == 1),
                          out.ptr("count"), list_count_ptrs=[d_counts.data_ptr() + 8 * r, d_counts.data_ptr() + 8 * s], out_hits_ptr=out.ptr("hits"),
                          out_hit_members_ptr=out.ptr("members"), hit_cap=n, stream=stream)
        want = np.flatnonzero(((masks >> np.uint64(r)) & np.uint64(1) == 1) & ((masks >> np.uint64(s)) & np.uint64(1) == 0))
        assert want.size > 20 and (((masks >> np.uint64(r)) & (masks >> np.uint64(s)) & np.uint64(1)) == 1).sum() > 5
        out.check({"count": one(want.size), "hits": want.astype(np.uint64), "members": np.ones(want.size, dtype=np.uint8)}, (r, s))


# ---- GPU: the lines, the terms and what the oracle says of every line (shared, computed once) -------------------------------------

# what a column may end in: nothing, or a witness of one of the golden tables (set_a regexps 0, 5, 6, 7; slow_alt; slow_a30)
TAILS = (b"", b"", b"", bytes.fromhex("68656c6c6f2020776f726c64"), b"Q", b"A", b"n", b"abc", b"a" + b"b" * 30)
_corpus, _verdicts = {}, {}


def corpus():
    """about 2 500 short log-like lines of up to five tab-separated columns -- empty lines and lines with fewer columns among
    them --, with and without a trailing delimiter"""
    if not _corpus:
        rng = np.random.RandomState(2500)
        lines = []
        for i in range(2500):
            cols = int(rng.randint(1, 6))
            parts = [H.random_strings(rng, 1, 12, b"fghijk 0123xyzd")[0] + TAILS[int(rng.randint(0, len(TAILS)))] for _ in range(cols)]
            lines.append(b"\t".join(parts))
        lines[500:503] = [b""] * 3
        lines[1023], lines[1024] = b"", b"Q"
        assert not any(b"\n" in s for s in lines) and min(s.count(b"\t") for s in lines) == 0 and max(s.count(b"\t") for s in lines) == 4
        joined = b"\n".join(lines)
        _corpus["buffers"] = [u8(joined + b"\n").copy(), u8(joined).copy()]
        for b in _corpus["buffers"]:
            b.setflags(write=False)
    return _corpus["buffers"]


def verdict(k, name, pick, column, rest, flags):
    """which lines of buffer k term (name, pick, column, rest, flags) lists, from the oracle on Python's split and cut: bool[n].
    pick: the wanted regexps (None: Final) of a Scanner, invert of a SlowScanner"""
    key = (k, name, column, rest, flags)
    if key not in _verdicts:
        parts, _ = py_lines(corpus()[k])
        strings = parts if column is None else [py_column(p, column, rest=rest) for p in parts]
        if name.startswith("slow_"):
            fin, _ = ob.OracleSlowScanner(_slow_blob(name)).run_strings(strings, flags=flags)
            _verdicts[key] = np.asarray(fin) != 0
        else:
            t = table_of(name)
            text, offs = H.pack(strings)
            idx = ob.OracleScanner(_big(name)[1]).run(text, offs, flags=flags, threads=4)[0]
            states = np.unique(idx).tolist()
            accepted = {s: set(t.AcceptedRegexps(s)) for s in states}
            final = {s: t.Final(s) for s in states}
            _verdicts[key] = (np.array([[r in accepted[s] for r in range(t.RegexpsCount)] for s in idx.tolist()], dtype=bool),
                              np.array([final[s] for s in idx.tolist()], dtype=bool))
    v = _verdicts[key]
    if name.startswith("slow_"):
        return v != bool(pick)
    return v[1] if pick is None else v[0][:, list(pick)].any(axis=1)


# a term: (table, pick, column, rest, flags)
A0 = ("set_a", (0,), None, False, BE)
CASES = {
    "two whole-line terms": ([A0, ("slow_alt", False, None, False, BE)], ("and-not", "or")),
    "two columns of one table": ([("set_a", (5, 6, 7), 1, False, BE), ("set_a", (6, 7), 3, False, BE)], ("and", "xor")),
    "a column and an inverted slow term": ([("set_a", (0, 6), 2, False, BE), ("slow_a30", True, None, False, BE)], ("and", "neither")),
    "six terms": ([A0, ("set_a", None, 1, False, BE), ("slow_alt", True, 1, False, BE), ("set_a", (5, 6, 7), 2, True, BE),
                   ("slow_alt", False, None, False, ob.FLAG_BEGIN), ("slow_a30", False, 0, False, BE)], ("random", "majority")),
}
TRUTHS = {"and-not": lambda k: pb.truth(k, lambda m: m == 1), "or": lambda k: pb.truth(k, lambda m: m != 0), "and": lambda k: pb.truth(k, lambda m: m == (1 << k) - 1),
          "xor": lambda k: pb.truth(k, lambda m: bin(m).count("1") % 2 == 1), "neither": lambda k: 1,
          "random": lambda k: random_truth(np.random.RandomState(66), k), "majority": lambda k: pb.truth(k, lambda m: bin(m).count("1") >= 3)}


def test_the_terms_of_the_gpu_part_each_list_some_lines_and_not_all():
    parts, _ = py_lines(corpus()[0])
    assert len(parts) == 2500 and len(py_lines(corpus()[1])[0]) == 2500
    for name, (terms, _) in CASES.items():
        for t in terms:
            v = verdict(0, *t)
            assert v.shape == (2500,) and 20 < v.sum() < 2480, (name, t, int(v.sum()))


def make_terms(torch, terms, device):
    """the pire_hip_line_term of every term, `want` staged where the call runs; (terms, what has to stay alive)"""
    out, keep = [], []
    for name, pick, column, rest, flags in terms:
        tab = table_of(name)
        if name.startswith("slow_"):
            out.append(pb.line_term(slow_table=tab, invert=pick, flags=flags, column=column, rest=rest))
            continue
        ptr = 0
        if pick is not None:
            wm = tab.want_mask(pick)
            want = torch.as_tensor(wm.view(np.int64), device="cuda") if device else wm
            keep.append(want)
            ptr = want.data_ptr() if device else want.ctypes.data
        out.append(pb.line_term(table=tab, want_ptr=ptr, flags=flags, column=column, rest=rest))
    return out, keep


def lines_call(torch, who, terms, truth, device, raw, cap, gather=None, lists=True, term_counts=True):
    """gather: None, or (tail, text_cap)"""
    keep = torch.as_tensor(np.array(raw), device="cuda") if device and len(raw) else raw
    rp = (keep.data_ptr() if device else keep.ctypes.data) if len(raw) else None
    sizes = {"n": 8, "cnt": 8, "hits": 8 * cap if lists else None, "spans": 16 * cap if lists else None, "members": cap if lists else None,
             "terms": 8 * len(terms) if term_counts else None}
    if gather:
        sizes.update({"text": gather[1], "offsets": 8 * (cap + 1), "bytes": 8})
    out = Outs(torch, device, sizes)
    cterms, alive = make_terms(torch, terms, device)
    g = (gather[0], out.ptr("text") if gather[1] else None, gather[1], out.ptr("offsets"), out.ptr("bytes")) if gather else None
    rc = lines_form(who, cterms, truth, rp, len(raw), 10, pb.FLAG_ON_DEVICE if device else 0, out.ptr("n"), out.ptr("hits") if cap else None,
                    out.ptr("spans") if cap else None, out.ptr("members") if cap else None, cap, out.ptr("cnt"), out.ptr("terms"), g, stream_of(torch))
    assert rc == 0, (who, pb.lib().pire_hip_last_error())
    return out, keep


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_lines_in_the_lines_a_boolean_function_of_the_terms_selects_out(torch_cuda, case):
    torch = torch_cuda
    terms, truths = CASES[case]
    select, gather = LINES_FORMS
    for k, raw in enumerate(corpus()):
        parts, spans = py_lines(raw)
        lists = [np.flatnonzero(verdict(k, *t)) for t in terms]
        for tname in truths if k == 0 else truths[:1]:
            truth = TRUTHS[tname](len(terms))
            exp = model_combine(lists, len(parts), truth)
            idx, count = exp["hits"].astype(np.int64), exp["count"]
            assert 10 < count < len(parts) - 10, (case, tname, count)
            for device in (True, False):
                for cap in (len(parts), count - 1):
                    what = (case, tname, k, "device" if device else "host", cap)
                    m = min(count, cap)
                    base = {"n": one(len(parts)), "cnt": one(count), "hits": exp["hits"][:m], "spans": spans[idx][:m], "members": exp["members"][:m],
                            "terms": u64([len(l) for l in lists])}
                    out, keep = lines_call(torch, select, terms, truth, device, raw, cap)
                    now = out.check(base, what)
                    got = now["spans"][GUARD:GUARD + 16 * m].view(np.uint64).reshape(-1, 2)
                    assert [bytes(raw[b:e]) for b, e in got.tolist()] == [parts[i] for i in idx[:m].tolist()], what
                    # the bytes: tail = delim is what grep prints; m lines where the list is short
                    text = b"".join(parts[i] + b"\n" for i in idx[:m].tolist())
                    ends = np.cumsum([0] + [len(parts[i]) + 1 for i in idx[:m].tolist()]).astype(np.uint64)
                    full = dict(base, text=text, offsets=ends, bytes=one(len(text)))
                    out, keep = lines_call(torch, gather, terms, truth, device, raw, cap, gather=(10, len(raw) + cap))
                    out.check(full, what)
                    if device:
                        assert (keep.cpu().numpy() == raw).all(), "the input was written to"
            # the gather form without lists of the caller's and without term counts, no tail, a text_cap in the middle of a line
            bare = b"".join(parts[i] for i in idx.tolist())
            room = max(len(bare) - 3, 0)
            ends = np.cumsum([0] + [len(parts[i]) for i in idx.tolist()]).astype(np.uint64)
            for device in (True, False):
                out, _ = lines_call(torch, gather, terms, truth, device, raw, len(parts), gather=(pb.NO_TAIL, room), lists=False, term_counts=False)
                out.check({"n": one(len(parts)), "cnt": one(count), "text": bare[:room], "offsets": ends, "bytes": one(len(bare))}, (case, tname, k, "no tail"))
            # a hit_cap of 0 and no lists: the counts
            out, _ = lines_call(torch, select, terms, truth, True, raw, 0, lists=False)
            out.check({"n": one(len(parts)), "cnt": one(count), "terms": u64([len(l) for l in lists])}, (case, tname, k, "counts"))


@gpu
def test_the_wrappers_and_a_buffer_of_no_lines(torch_cuda):
    torch = torch_cuda
    terms, _ = CASES["two whole-line terms"]
    raw = corpus()[0]
    parts, spans = py_lines(raw)
    lists = [np.flatnonzero(verdict(0, *t)) for t in terms]
    truth = pb.truth(2, lambda m: m == 1)                          # grep a | grep -v b
    exp = model_combine(lists, len(parts), truth)
    cterms, alive = make_terms(torch, terms, False)
    w = pb.lines_combine_host(cterms, truth, raw, gather=True)
    assert (w["lines"], w["count"]) == (len(parts), exp["count"]) and w["term_counts"].tolist() == [len(l) for l in lists]
    assert (w["hits"] == exp["hits"]).all() and (w["members"] == exp["members"]).all() and (w["spans"] == spans[exp["hits"].astype(np.int64)]).all()
    assert w["text"].tobytes() == b"".join(parts[i] + b"\n" for i in exp["hits"].tolist())
    # ... on device pointers: the select form, then the gather form
    cterms, alive = make_terms(torch, terms, True)
    d_raw = torch.as_tensor(np.array(raw), device="cuda")
    words = torch.zeros(5, dtype=torch.int64, device="cuda")      # lines, selected, bytes, the terms' counts
    d_hits = torch.full((len(parts),), -1, dtype=torch.int64, device="cuda")
    d_members = torch.zeros(len(parts), dtype=torch.uint8, device="cuda")
    d_text = torch.zeros(len(raw) + len(parts), dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(len(parts) + 1, dtype=torch.int64, device="cuda")
    for out_bytes in (None, words[2:].data_ptr()):
        pb.lines_combine_device(cterms, truth, d_raw.data_ptr(), len(raw), words.data_ptr(), words[1:].data_ptr(), out_hits_ptr=d_hits.data_ptr(),
                                out_hit_members_ptr=d_members.data_ptr(), hit_cap=len(parts), out_term_counts_ptr=words[3:].data_ptr(),
                                out_bytes_ptr=out_bytes, out_text_ptr=d_text.data_ptr(), text_cap=d_text.numel(), out_offsets_ptr=d_offs.data_ptr(),
                                stream=stream_of(torch) or 0)
        torch.cuda.synchronize()
        assert words.cpu().tolist() == [len(parts), exp["count"], 0 if out_bytes is None else w["bytes"]] + [len(l) for l in lists]
        assert (d_hits.cpu().numpy()[:exp["count"]] == exp["hits"].astype(np.int64)).all() and (d_members.cpu().numpy()[:exp["count"]] == exp["members"]).all()
    assert d_text.cpu().numpy()[:w["bytes"]].tobytes() == w["text"].tobytes() and (d_offs.cpu().numpy()[:exp["count"] + 1] == w["offsets"].astype(np.int64)).all()
    # no lines: an empty buffer on the device (a buffer of delimiters only is that many empty lines) -- zeros, under any truth table
    for who in LINES_FORMS:
        for t in (1, 0b1110):
            g = (10, 16) if who.endswith("gather") else None
            out, _ = lines_call(torch, who, terms, t, True, u8(b""), 4, gather=g)
            want = {"n": one(0), "cnt": one(0), "hits": b"", "spans": b"", "members": b"", "terms": u64([0, 0])}
            if g:
                want.update({"text": b"", "offsets": one(0), "bytes": one(0)})
            out.check(want, (who, t, "empty"))
    # ... and delimiters only: seventy empty lines, which bit 0 selects
    blank = u8(b"\n" * 70)
    none = [int(verdict_of_empty(t)) for t in terms]
    mask = none[0] + 2 * none[1]                                   # the member mask of an empty line
    for device in (True, False):
        out, _ = lines_call(torch, LINES_FORMS[0], terms, 1 << mask, device, blank, 70)
        out.check({"n": one(70), "cnt": one(70), "hits": u64(np.arange(70)), "spans": u64([[i, i] for i in range(70)]),
                   "members": np.full(70, mask, dtype=np.uint8), "terms": u64([70 * v for v in none])}, ("blank", device))
        out, _ = lines_call(torch, LINES_FORMS[0], terms, 0b1111 & ~(1 << mask), device, blank, 70)
        out.check({"n": one(70), "cnt": one(0), "hits": b"", "spans": b"", "members": b"", "terms": u64([70 * v for v in none])}, ("blank, none", device))


def verdict_of_empty(term):
    """whether the term lists an empty line, from the oracle"""
    name, pick, _, _, flags = term
    if name.startswith("slow_"):
        fin, _ = ob.OracleSlowScanner(_slow_blob(name)).run_strings([b""], flags=flags)
        return (np.asarray(fin)[0] != 0) != bool(pick)
    t = table_of(name)
    text, offs = H.pack([b""])
    s = int(ob.OracleScanner(_big(name)[1]).run(text, offs, flags=flags, threads=1)[0][0])
    return t.Final(s) if pick is None else bool(set(t.AcceptedRegexps(s)) & set(pick))


@gpu
@pytest.mark.parametrize("k", (0, 1))
def test_the_chain_with_device_pointers_and_no_read_back(torch_cuda, k):
    """pire_hip_split with out_text == NULL for the offsets, a Scanner list and a SlowScanner list over the same lines,
    pire_hip_combine (in the first and not in the second), pire_hip_context, pire_hip_gather with NO_TAIL over raw and the split's
    offsets: grep a | grep -v b with a line of context, delimiters included"""
    torch = torch_cuda
    fast, slow = table_of("set_a"), table_of("slow_alt")
    raw = corpus()[k]
    parts, _ = py_lines(raw)
    n, size = len(parts), len(raw)
    a, b = np.flatnonzero(verdict(k, "set_a", (5, 6, 7), None, False, BE)), np.flatnonzero(verdict(k, "slow_alt", False, None, False, BE))
    comb = model_combine([a, b], n, 0b0010)
    exp = model_context(comb["hits"], n, 1, 1)
    assert 50 < comb["count"] < exp["count"] < n - 50
    stream = torch.cuda.current_stream().cuda_stream
    d_raw = torch.as_tensor(np.array(raw), device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(9, dtype=torch.int64, device="cuda")      # n, lines of scan a, hits a, lines of scan b, hits b, combined, selected, groups, bytes
    d_a, d_b, d_c, d_lines = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(4))
    d_text = torch.full((size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d_ends = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    want = torch.as_tensor(fast.want_mask([5, 6, 7]).view(np.int64), device="cuda")
    pb.split_device(d_raw.data_ptr(), size, d_cnt[0:].data_ptr(), out_offsets_ptr=d_off.data_ptr(), offsets_cap=n, stream=stream)
    fast.run_lines_select_device(d_raw.data_ptr(), size, BE, d_cnt[1:].data_ptr(), d_cnt[2:].data_ptr(), want_ptr=want.data_ptr(),
                                 out_hits_ptr=d_a.data_ptr(), hit_cap=n, stream=stream)
    slow.lines_select_device(d_raw.data_ptr(), size, BE, d_cnt[3:].data_ptr(), d_cnt[4:].data_ptr(), out_hits_ptr=d_b.data_ptr(), hit_cap=n, stream=stream)
    pb.combine_device([d_a.data_ptr(), d_b.data_ptr()], [n, n], n, 0b0010, d_cnt[5:].data_ptr(), list_count_ptrs=[d_cnt[2:].data_ptr(), d_cnt[4:].data_ptr()],
                      out_hits_ptr=d_c.data_ptr(), hit_cap=n, stream=stream)
    pb.context_device(d_c.data_ptr(), n, n, d_cnt[6:].data_ptr(), 1, 1, hit_count_ptr=d_cnt[5:].data_ptr(), out_lines_ptr=d_lines.data_ptr(),
                      line_cap=n, out_group_count_ptr=d_cnt[7:].data_ptr(), stream=stream)
    pb.gather_device(d_raw.data_ptr(), d_off.data_ptr(), n, d_cnt[8:].data_ptr(), idx_ptr=d_lines.data_ptr(), idx_count_ptr=d_cnt[6:].data_ptr(),
                     idx_cap=n, tail=None, out_text_ptr=d_text.data_ptr(), text_cap=size, out_offsets_ptr=d_ends.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ends = np.cumsum([0] + [len(p) + 1 for p in parts])
    ends[-1] = size                                                # (the last line of buffer 1 has no delimiter behind it)
    joined = b"".join(bytes(raw[ends[i]:ends[i + 1]]) for i in exp["lines"].tolist())
    assert d_cnt.cpu().tolist() == [n, n, len(a), n, len(b), comb["count"], exp["count"], exp["groups"], len(joined)]
    got = d_text.cpu().numpy()
    assert got[:len(joined)].tobytes() == joined and (got[len(joined):] == POISON).all()
    assert (d_c.cpu().numpy()[:comb["count"]] == comb["hits"].astype(np.int64)).all()
    assert (d_lines.cpu().numpy()[:exp["count"]] == exp["lines"].astype(np.int64)).all()
