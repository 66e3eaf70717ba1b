"""The hit passes on the inputs of the two C++ shim programs (tests/cpp/select_shim_test.cpp, tests/cpp/route_shim_test.cpp),
against answers recorded from the reference library alone (tests/golden/shim_inputs, tests/golden/make_shim_inputs.py).

The shim programs check three layers at once -- the library, include/pire_hip/batch_runner.hpp and themselves -- and need
the reference tree to build.  These tests make the shim's C calls from Python, on the shim's scanners and string lists, so
that a failure of a shim program can be pinned to a layer: what fails here is the library's.

The expectation is always the fixture: the reference's end StateIndex, Final and AcceptedRegexps per string.  No library
call and no oracle call goes into it.  The CPU part checks that the oracle and the library's host table agree with the
fixture, the GPU part that every call sequence of the shim does.  Every comparison is exact; host arrays and device
buffers are poisoned and have guard words behind them.
"""
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H
from tests import test_route as TR
from tests import test_select as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(H.GOLDEN, "shim_inputs")
POISON = TR.POISON
P64 = np.uint64(POISON)
GUARD = 8
gpu = pytest.mark.gpu


def _generator():
    spec = importlib.util.spec_from_file_location("make_shim_inputs", os.path.join(H.GOLDEN, "make_shim_inputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
PAIRS = [G.pair_name(*p) for p in G.PAIRS]
LONG_AT = 9   # where route_text has its 3 073-byte string


# ---- a fixture and what it expects --------------------------------------------------------------------------------------

class Case:
    """One (scanner, list, flags): the strings rebuilt from the generator's formulas, the reference's answers from the JSON.
    `order`: the case on a sub-list -- entries of the recorded list dropped or moved, the recorded answers with them."""

    def __init__(self, name, order=None):
        with open(os.path.join(DIR, name + ".json")) as f:
            rec = json.load(f)
        self.name, self.rec, self.scanner, self.flags, self.regexps = name, rec, rec["scanner"], rec["flags"], rec["regexps"]
        strings = G.LISTS[rec["list"]]()
        assert len(strings) == rec["n"] == len(rec["idx"]) == len(rec["final"]) == len(rec["masks"])
        self.words = max(1, (self.regexps + 63) // 64)
        idx = np.array(rec["idx"], dtype=np.uint32)
        fin = np.array(rec["final"], dtype=np.uint8)
        masks = np.array([[(int(m, 16) >> (64 * w)) & (2 ** 64 - 1) for w in range(self.words)] for m in rec["masks"]], dtype=np.uint64)
        if order is not None:
            strings, idx, fin, masks = [strings[i] for i in order], idx[order], fin[order], masks[order]
        self.strings, self.idx, self.fin, self.masks, self.n = strings, idx, fin, masks, len(strings)
        self.text, self.offs = H.pack(strings)
        self.raw = np.frombuffer(b"".join(s + b"\n" for s in strings), dtype=np.uint8)
        begins = self.offs[:-1] + np.arange(self.n, dtype=np.uint64)
        self.line_spans = np.stack([begins, begins + (self.offs[1:] - self.offs[:-1])], axis=1)

    @property
    def blob(self):
        return _blob(self.scanner)

    @property
    def table(self):
        return _table(self.scanner)

    def member(self, r):
        return ((self.masks[:, r // 64] >> np.uint64(r % 64)) & np.uint64(1)).astype(bool)

    def route(self):
        hits = [np.nonzero(self.member(r))[0].astype(np.uint64) for r in range(self.regexps)]
        return {"counts": np.array([len(h) for h in hits], dtype=np.uint64), "hits": hits}

    def select(self, want):
        """The host loop of select_shim_test.cpp on the recorded answers: no want = Final, else any wanted regexp < R accepted"""
        if not want:
            sel = self.fin.astype(bool)
        else:
            sel = np.zeros(self.n, dtype=bool)
            for r in want:
                if r < self.regexps:
                    sel |= self.member(r)
        return {"masks": self.masks, "hits": np.nonzero(sel)[0].astype(np.uint64), "hit_masks": self.masks[sel], "count": int(sel.sum())}

    def wants(self):
        r = self.regexps
        return [[], [0], [r - 1], [0, 1, 2], [r + 5]]


@functools.lru_cache(maxsize=None)
def _blob(scanner):
    with open(os.path.join(DIR, scanner + ".blob"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def _table(scanner):
    return pb.Table(_blob(scanner))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def isolation_cases():
    """The four-regexp scanner on route_text: the smallest lists that tell "a long string in the batch" from "more than one
    tile of the pass" from "more than two" """
    n = len(G.route_text())
    rest = [i for i in range(n) if i != LONG_AT]
    return {"long_string_removed": rest, "long_string_first": [LONG_AT] + rest, "long_string_last": rest + [LONG_AT],
            "first_1024": list(range(1024)), "first_1025": list(range(1025))}


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_the_fixtures_are_the_pairs_of_the_shim_programs_and_none_is_vacuous():
    assert sorted(os.listdir(DIR)) == sorted([p + ".json" for p in PAIRS] + [s + ".blob" for s in G.SCANNERS])
    for p, (scanner, which, flags) in zip(PAIRS, G.PAIRS):
        c = case(p)
        counts = c.route()["counts"]
        assert counts.tolist() == c.rec["row_counts"] and (c.scanner, c.rec["list"], c.flags) == (scanner, which, flags)
        if (scanner, which, flags) in G.ALL_EMPTY:
            assert not counts.any()   # (the reference's answer under Begin(): see the generator)
        else:
            assert counts.any(), p
    assert (case("aaa_bbb_ccc_abc__route_text").route()["counts"] > 0).all()
    wide = case("two_letters_70__pairs__unmarked")
    assert wide.words == 2 and wide.masks[:, 0].any() and wide.masks[:, 1].any()
    long_one = G.route_text()[LONG_AT]
    assert len(long_one) == 3073 and G.select_text()[17] == long_one


@pytest.mark.parametrize("name", PAIRS)
def test_the_list_rebuilt_from_the_formulas_is_the_recorded_one(name):
    c = case(name)
    assert G.list_sha256(c.strings) == c.rec["sha256"]


@pytest.mark.parametrize("name", PAIRS)
def test_oracle_reproduces_the_recorded_answers(name):
    c = case(name)
    o = ob.OracleScanner(c.blob)
    assert o.regexps == c.regexps
    idx, fin = o.run(c.text, c.offs, flags=c.flags)
    assert (idx == c.idx).all() and (fin == c.fin).all()
    for s in np.unique(c.idx).tolist():
        mask = sum(1 << r for r in o.accepted(int(s)))
        assert "%x" % mask == c.rec["masks"][int(np.nonzero(c.idx == s)[0][0])], s
        assert o.final(int(s)) == bool(c.fin[c.idx == s][0])


@pytest.mark.parametrize("name", PAIRS)
def test_host_table_reproduces_the_recorded_answers(name):
    c = case(name)
    t = c.table
    assert t.RegexpsCount == c.regexps == G.SCANNERS[c.scanner][2] and t.mask_words == c.words and not t.Empty
    for s in np.unique(c.idx).tolist():
        at = int(np.nonzero(c.idx == s)[0][0])
        assert s < t.Size
        assert "%x" % sum(1 << r for r in t.AcceptedRegexps(int(s))) == c.rec["masks"][at], s
        assert t.Final(int(s)) == bool(c.fin[at]), s


@pytest.mark.skipif(not ob.ref_available(), reason="the reference library is not built here")
def test_the_generator_reproduces_the_committed_files_byte_for_byte():
    files = G.generate()
    assert sorted(files) == sorted(os.listdir(DIR))
    for name, data in files.items():
        with open(os.path.join(DIR, name), "rb") as f:
            assert f.read() == data, name


def test_isolation_lists_keep_their_recorded_answers():
    whole = case("aaa_bbb_ccc_abc__route_text")
    o = ob.OracleScanner(whole.blob)
    for which, order in isolation_cases().items():
        c = Case(whole.name, order)
        idx, fin = o.run(c.text, c.offs)
        assert (idx == c.idx).all() and (fin == c.fin).all(), which
        assert (c.route()["counts"] > 0).all(), which
    assert len(Case(whole.name, isolation_cases()["long_string_removed"]).strings) == whole.n - 1


# ---- GPU: poisoned outputs -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def ok(rc):
    assert rc == 0, pb.lib().pire_hip_last_error()


def poisoned(count):
    return np.full(count + GUARD, P64, dtype=np.uint64)


def guard_intact(a, count):
    assert (a[count:] == P64).all(), "written behind the array"


def to_dev(torch, a, slack=0):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    src = torch.as_tensor(a.view(signed) if signed else a)
    if not slack and a.size:
        return src.to("cuda")
    out = torch.zeros(a.size + max(slack, 16), dtype=src.dtype, device="cuda")
    out[:a.size] = src
    return out


class DevStates:
    """Poisoned state indices and finals on the device, guard entries behind them"""

    def __init__(self, torch, n):
        self.n = n
        self.idx = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
        self.fin = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def check(self, c):
        idx, fin = self.idx.cpu().numpy().view(np.uint32), self.fin.cpu().numpy()
        assert (idx[self.n:] == 0xFFFFFFFF).all() and (fin[self.n:] == 0xA5).all(), "written behind the array"
        assert (idx[:self.n] == c.idx).all(), np.nonzero(idx[:self.n] != c.idx)[0][:8]
        assert (fin[:self.n] == c.fin).all(), np.nonzero(fin[:self.n] != c.fin)[0][:8]


def host_states(c):
    idx = np.full(c.n + GUARD, 0xFFFFFFFF, dtype=np.uint32)
    fin = np.full(c.n + GUARD, 0xA5, dtype=np.uint8)
    return idx, fin


def check_host_states(c, idx, fin):
    assert (idx[c.n:] == 0xFFFFFFFF).all() and (fin[c.n:] == 0xA5).all(), "written behind the array"
    assert (idx[:c.n] == c.idx).all(), np.nonzero(idx[:c.n] != c.idx)[0][:8]
    assert (fin[:c.n] == c.fin).all(), np.nonzero(fin[:c.n] != c.fin)[0][:8]


def check_host_rows(c, counts, flat, pitch, exp, width=1, expected_rows=None):
    """counts u64[R + guard], flat u64[R * pitch * width + guard]: full counts, min(count, pitch) entries per row, poison behind"""
    r = c.regexps
    guard_intact(counts, r)
    guard_intact(flat, r * pitch * width)
    assert counts[:r].tolist() == exp["counts"].tolist()
    rows = flat[:r * pitch * width].reshape(r, pitch, width)
    want_rows = exp["hits"] if expected_rows is None else expected_rows
    for k in range(r):
        m = min(int(counts[k]), pitch)
        assert (rows[k, :m] == np.asarray(want_rows[k][:m]).reshape(m, width)).all(), "row %d" % k
        assert (rows[k, m:] == P64).all(), "row %d written behind min(count, pitch)" % k


def check_host_select(c, count, hits, hit_masks, cap, exp, masks=None):
    w = c.words
    assert int(count.value) == exp["count"]
    k = min(exp["count"], cap)
    guard_intact(hits, cap)
    guard_intact(hit_masks, cap * w)
    assert (hits[:k] == exp["hits"][:k]).all() and (hits[k:cap] == P64).all()
    assert (hit_masks[:k * w].reshape(k, w) == exp["hit_masks"][:k]).all() and (hit_masks[k * w:cap * w] == P64).all()
    if masks is not None:
        guard_intact(masks, c.n * w)
        assert (masks[:c.n * w].reshape(c.n, w) == exp["masks"]).all()


def want_ptr(c, want):
    """(host mask or None, what keeps it alive): the shim's Select(): no want = a null pointer, numbers behind the mask words dropped"""
    if not want:
        return None
    m = np.zeros(c.words, dtype=np.uint64)
    for r in want:
        if r < 64 * c.words:
            m[r // 64] |= np.uint64(1 << (r % 64))
    return m


# ---- GPU: the scan ---------------------------------------------------------------------------------------------------------

def run_both_ways(torch, c):
    """pire_hip_run on host pointers and with ON_DEVICE: state indices and finals against the fixture"""
    L, t = pb.lib(), c.table
    idx, fin = host_states(c)
    ok(L.pire_hip_run(t._h, c.text.ctypes.data, c.offs.ctypes.data, c.n, c.flags, None, idx.ctypes.data, fin.ctypes.data, None, None))
    check_host_states(c, idx, fin)
    dt, do, out = to_dev(torch, c.text, 256), to_dev(torch, c.offs), DevStates(torch, c.n)
    ok(L.pire_hip_run(t._h, dt.data_ptr(), do.data_ptr(), c.n, c.flags | pb.FLAG_ON_DEVICE, None, out.idx.data_ptr(), out.fin.data_ptr(),
                      None, None))
    torch.cuda.synchronize()
    out.check(c)


@gpu
@pytest.mark.parametrize("name", PAIRS)
def test_run(torch_cuda, name):
    run_both_ways(torch_cuda, case(name))


# ---- GPU: select -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", PAIRS)
def test_select(torch_cuda, name):
    """pire_hip_select on the recorded end states and pire_hip_run_select on the text, host and device, the shim's five wants"""
    torch, L, c = torch_cuda, pb.lib(), case(name)
    t, n, w = c.table, c.n, c.words
    dt, do, di = to_dev(torch, c.text, 256), to_dev(torch, c.offs), to_dev(torch, c.idx)
    for want in c.wants():
        exp = c.select(want)
        wm = want_ptr(c, want)
        wp = None if wm is None else wm.ctypes.data
        # host pointers: the select pass alone, then scan + pass
        count, hits, hm, masks = C.c_uint64(POISON), poisoned(n), poisoned(n * w), poisoned(n * w)
        ok(L.pire_hip_select(t._h, c.idx.ctypes.data, n, wp, 0, masks.ctypes.data, hits.ctypes.data, hm.ctypes.data, n, C.byref(count), None))
        check_host_select(c, count, hits, hm, n, exp, masks)
        count, hits, hm = C.c_uint64(POISON), poisoned(n), poisoned(n * w)
        idx, fin = host_states(c)
        ok(L.pire_hip_run_select(t._h, c.text.ctypes.data, c.offs.ctypes.data, n, c.flags, None, idx.ctypes.data, fin.ctypes.data, None, wp,
                                 None, hits.ctypes.data, hm.ctypes.data, n, C.byref(count), None))
        check_host_select(c, count, hits, hm, n, exp)
        check_host_states(c, idx, fin)
        # ... and on the device
        dw = None if wm is None else to_dev(torch, wm)
        out = TS.DevOut(torch, t, n, n)
        t.select_device(di.data_ptr(), n, want_ptr=0 if dw is None else dw.data_ptr(), **out.ptrs())
        torch.cuda.synchronize()
        TS.check(out.fetch(), exp)
        out, st = TS.DevOut(torch, t, n, n), DevStates(torch, n)
        t.run_select_device(dt.data_ptr(), do.data_ptr(), n, c.flags, want_ptr=0 if dw is None else dw.data_ptr(),
                            out_idx_ptr=st.idx.data_ptr(), out_final_ptr=st.fin.data_ptr(), **out.ptrs())
        torch.cuda.synchronize()
        TS.check(out.fetch(), exp)
        st.check(c)


# ---- GPU: route ------------------------------------------------------------------------------------------------------------

def route_every_way(torch, c):
    """pire_hip_route on the recorded end states, pire_hip_run_route on the text -- once with out_idx, once with the four
    optional outputs null, which is how the shim calls it --, host and device, pitch n"""
    L, t, n, r = pb.lib(), c.table, c.n, c.regexps
    exp = c.route()
    counts, hits = poisoned(r), poisoned(r * n)
    ok(L.pire_hip_route(t._h, c.idx.ctypes.data, n, 0, hits.ctypes.data, n, counts.ctypes.data, None))
    check_host_rows(c, counts, hits, n, exp)
    for states in (True, False):
        counts, hits = poisoned(r), poisoned(r * n)
        idx, fin = host_states(c)
        ok(L.pire_hip_run_route(t._h, c.text.ctypes.data, c.offs.ctypes.data, n, c.flags, None, idx.ctypes.data if states else None,
                                fin.ctypes.data if states else None, None, hits.ctypes.data, n, counts.ctypes.data, None))
        check_host_rows(c, counts, hits, n, exp)
        if states:
            check_host_states(c, idx, fin)
    di = to_dev(torch, c.idx)
    out = TR.DevOut(torch, t, n)
    t.route_device(di.data_ptr(), n, **out.ptrs())
    torch.cuda.synchronize()
    TR.check(out.fetch(), exp)
    dt, do = to_dev(torch, c.text, 256), to_dev(torch, c.offs)
    for states in (True, False):
        out, st = TR.DevOut(torch, t, n), DevStates(torch, n)
        t.run_route_device(dt.data_ptr(), do.data_ptr(), n, c.flags, out_idx_ptr=st.idx.data_ptr() if states else 0,
                           out_final_ptr=st.fin.data_ptr() if states else 0, **out.ptrs())
        torch.cuda.synchronize()
        TR.check(out.fetch(), exp)
        if states:
            st.check(c)


@gpu
@pytest.mark.parametrize("name", PAIRS)
def test_route(torch_cuda, name):
    route_every_way(torch_cuda, case(name))


# ---- GPU: the lines forms --------------------------------------------------------------------------------------------------

def lines_route(c, pitch, exp):
    L, t, r = pb.lib(), c.table, c.regexps
    lines, counts, hits, spans = C.c_uint64(POISON), poisoned(r), poisoned(r * pitch), poisoned(r * pitch * 2)
    ok(L.pire_hip_run_lines_route(t._h, c.raw.ctypes.data, c.raw.size, 10, c.flags, C.byref(lines), hits.ctypes.data, spans.ctypes.data, pitch,
                                  counts.ctypes.data, None))
    assert int(lines.value) == c.n
    check_host_rows(c, counts, hits, pitch, exp)
    check_host_rows(c, counts, spans, pitch, exp, 2, [c.line_spans[h.astype(np.int64)] for h in exp["hits"]])
    return int(counts[:r].max())


def lines_select(c, want, cap, exp):
    L, t, w = pb.lib(), c.table, c.words
    wm = want_ptr(c, want)
    lines, count, hits, spans, hm = C.c_uint64(POISON), C.c_uint64(POISON), poisoned(cap), poisoned(cap * 2), poisoned(cap * w)
    ok(L.pire_hip_run_lines_select(t._h, c.raw.ctypes.data, c.raw.size, 10, c.flags, None if wm is None else wm.ctypes.data, C.byref(lines),
                                   hits.ctypes.data, spans.ctypes.data, hm.ctypes.data, cap, C.byref(count), None))
    assert int(lines.value) == c.n
    check_host_select(c, count, hits, hm, cap, exp)
    k = min(exp["count"], cap)
    guard_intact(spans, cap * 2)
    assert (spans[:2 * k].reshape(k, 2) == c.line_spans[exp["hits"][:k].astype(np.int64)]).all() and (spans[2 * k:2 * cap] == P64).all()
    return int(count.value)


def lines_every_way(c):
    """pire_hip_run_lines_route / _select on the list joined with newlines, host pointers: at pitch n, then the way the shim's
    RunLines() does it -- pitch size / 64 + 1024 and, where a list is longer, a second call at that length"""
    exp = c.route()
    first = c.raw.size // 64 + 1024
    assert lines_route(c, c.n, exp) == int(exp["counts"].max())
    longest = lines_route(c, first, exp)
    if longest > first:
        assert lines_route(c, longest, exp) == longest
    for want in c.wants():
        sel = c.select(want)
        assert lines_select(c, want, c.n, sel) == sel["count"]
        count = lines_select(c, want, first, sel)
        if count > first:
            assert lines_select(c, want, count, sel) == count


@gpu
@pytest.mark.parametrize("name", PAIRS)
def test_lines(torch_cuda, name):
    c = case(name)
    if c.rec["list"] == "dense":   # the list that makes the shim call twice: 3 000 hits, first pitch 1 211
        assert c.raw.size == 12000 and c.raw.size // 64 + 1024 == 1211 < int(c.route()["counts"].max()) == 3000
    lines_every_way(c)


# ---- GPU: the shim's device sequence ------------------------------------------------------------------------------------------

class DeviceBuffers:
    """pire_hip_device_alloc / pire_hip_device_free, the shim's DeviceBuffer"""

    def __init__(self):
        self.ptrs = []

    def alloc(self, size):
        p = C.c_void_p()
        ok(pb.lib().pire_hip_device_alloc(size, C.byref(p)))
        self.ptrs.append(p)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            pb.lib().pire_hip_device_free(p)
        return False


def device_sequence(c):
    """RunDevice().End().Route() and the fetches of RouteCount() / RouteHits() as batch_runner.hpp makes them, call for call,
    all on the null stream -- on buffers filled with 0xAB first, so that what lies behind a row's hits is seen to stay"""
    L, t, n, r = pb.lib(), c.table, c.n, c.regexps
    exp = c.route()
    fill = np.uint64(0xABABABABABABABAB)
    with DeviceBuffers() as dev:
        d_text, d_offs = dev.alloc(c.text.size + 256), dev.alloc(c.offs.size * 8)
        ok(L.pire_hip_copy_to_device(d_text, c.text.ctypes.data, c.text.size, None))
        ok(L.pire_hip_copy_to_device(d_offs, c.offs.ctypes.data, c.offs.size * 8, None))
        ok(L.pire_hip_stream_synchronize(None))
        d_idx, d_fin, d_cnt = dev.alloc(n * 4), dev.alloc(n), dev.alloc((r + 2) * 8)
        hit_words = r * n + 1
        d_hits, d_counts = dev.alloc(hit_words * 8), dev.alloc((r + 1) * 8)
        ok(L.pire_hip_memset_device(d_hits, 0xAB, hit_words * 8, None))
        ok(L.pire_hip_memset_device(d_counts, 0xAB, (r + 1) * 8, None))
        # Execute()
        ok(L.pire_hip_memset_device(d_cnt, 0, (r + 2) * 8, None))
        ok(L.pire_hip_run(t._h, d_text, d_offs, n, c.flags | pb.FLAG_ON_DEVICE, None, d_idx, d_fin, d_cnt, None))
        # ExecuteRoute()
        ok(L.pire_hip_route(t._h, d_idx, n, pb.FLAG_ON_DEVICE, d_hits, n, d_counts, None))
        # FetchRoute()
        counts = np.zeros(r + 1, dtype=np.uint64)
        ok(L.pire_hip_copy_to_host(counts.ctypes.data, d_counts, r * 8, None))
        ok(L.pire_hip_stream_synchronize(None))
        assert counts[:r].tolist() == exp["counts"].tolist()
        rows = [np.zeros(int(k), dtype=np.uint64) for k in counts[:r]]
        for k in range(r):
            if counts[k]:
                ok(L.pire_hip_copy_to_host(rows[k].ctypes.data, C.c_void_p(d_hits.value + 8 * k * n), int(counts[k]) * 8, None))
        ok(L.pire_hip_stream_synchronize(None))
        for k in range(r):
            assert (rows[k] == exp["hits"][k]).all(), "row %d" % k
        # Fetch(), and the run's own counters
        idx, fin, cnt = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8), np.zeros(r + 2, dtype=np.uint64)
        ok(L.pire_hip_copy_to_host(idx.ctypes.data, d_idx, n * 4, None))
        ok(L.pire_hip_copy_to_host(fin.ctypes.data, d_fin, n, None))
        ok(L.pire_hip_copy_to_host(cnt.ctypes.data, d_cnt, (r + 2) * 8, None))
        # what lies behind the hits of every row, and behind the two arrays
        whole = np.zeros(hit_words, dtype=np.uint64)
        ok(L.pire_hip_copy_to_host(whole.ctypes.data, d_hits, hit_words * 8, None))
        ok(L.pire_hip_copy_to_host(counts.ctypes.data, d_counts, (r + 1) * 8, None))
        ok(L.pire_hip_stream_synchronize(None))
    assert (idx == c.idx).all() and (fin == c.fin).all()
    assert cnt[2:].tolist() == exp["counts"].tolist() and int(cnt[1]) == n
    assert whole[r * n] == fill and counts[r] == fill
    for k in range(r):
        assert (whole[k * n + int(counts[k]):(k + 1) * n] == fill).all(), "row %d written behind its hits" % k


@gpu
@pytest.mark.parametrize("name", PAIRS)
def test_the_shims_device_sequence(torch_cuda, name):
    device_sequence(case(name))


# ---- GPU: which ingredient ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("which", sorted(isolation_cases()))
def test_ingredient_isolation(torch_cuda, which):
    """The four-regexp scanner on sub-lists of route_text, through the scan, the route forms, the lines forms and the shim's
    device sequence: where the whole list fails and one of these passes, the difference between the two lists is the cause"""
    c = Case("aaa_bbb_ccc_abc__route_text", isolation_cases()[which])
    run_both_ways(torch_cuda, c)
    route_every_way(torch_cuda, c)
    lines_every_way(c)
    device_sequence(c)
