"""pire_hip_route / pire_hip_run_route[_strided] / pire_hip_run_lines_route: one ascending hit list per regexp, answered on
the device (route.hip).

Exact equality everywhere.  The expected values come from `expected_route`: end states from the oracle (and the reference
library where oracle/_ref is built, tests/test_select.py::end_states), membership from the host accessor
Table.AcceptedRegexps."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H
from tests import test_select as TS
from tests.conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE = pb.FLAG_BEGIN | pb.FLAG_END
POISON = 0xDEADBEEFCAFEF00D
gpu = pytest.mark.gpu
NEW_SYMBOLS = ["pire_hip_route", "pire_hip_run_route", "pire_hip_run_route_strided", "pire_hip_run_lines_route"]


# ---- the expectation helper ------------------------------------------------------------------------------------------

def membership(t, idx):
    """bool[n, R]: member(i, r) <=> r in AcceptedRegexps(idx[i]) and r < R; a state index beyond the table is nobody's."""
    idx = np.asarray(idx, dtype=np.uint32)
    r = t.RegexpsCount
    uniq = np.unique(idx)
    rows = np.zeros((len(uniq), r), dtype=bool)
    for k, s in enumerate(uniq.tolist()):
        if s < t.Size:
            for a in t.AcceptedRegexps(int(s)):
                if a < r:
                    rows[k, a] = True
    return rows[np.searchsorted(uniq, idx)] if len(idx) else np.zeros((0, r), dtype=bool)


def expected_route(t, idx):
    """What pire_hip_route must answer: {"counts": u64[R], "hits": [R ascending index arrays]}."""
    m = membership(t, idx)
    hits = [np.nonzero(m[:, r])[0].astype(np.uint64) for r in range(t.RegexpsCount)]
    return {"counts": np.array([len(h) for h in hits], dtype=np.uint64), "hits": hits}


def check(got, exp, cap=None):
    assert got["counts"].dtype == np.uint64 and got["counts"].tolist() == exp["counts"].tolist()
    assert len(got["hits"]) == len(exp["hits"])
    for r, (g, e) in enumerate(zip(got["hits"], exp["hits"])):
        k = len(e) if cap is None else min(cap, len(e))
        assert len(g) == k and (g == e[:k]).all(), "row %d" % r


def table_of(name):
    case = [c for c in H.all_cases() + H.big_sets() if c["name"] == name][0]
    blob = H.load_blob(case["blob"])
    return case, pb.Table(blob), ob.OracleScanner(blob)


def state_pool(t, o, case):
    """End states of a golden table's own strings: {frozenset of accepted regexps: a state index}."""
    if "corpus" in case:
        idx = np.unique(np.asarray(case["corpus"]["idx"], dtype=np.uint32))
    else:
        text, offs = H.pack(H.case_strings(case) + [b"", b"zzzz"])
        idx = np.unique(TS.end_states(t, o, text, offs))
    return {frozenset(a for a in t.AcceptedRegexps(int(s)) if a < t.RegexpsCount): int(s) for s in idx.tolist()}


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_route_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    assert set(NEW_SYMBOLS) <= {n for n, _, _ in pb.ABI}
    for name in ("route", "run_route", "run_route_strided", "run_lines_route"):
        assert callable(getattr(pb.Table, name))


@pytest.mark.parametrize("case", [c for c in H.all_cases() if "ref_expect_accepted" in c], ids=lambda c: c["name"])
def test_expectation_helper_against_the_lists_of_the_references_own_tests(case):
    blob = H.load_blob(case["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    text, offs = H.pack(H.case_strings(case))
    exp = expected_route(t, TS.end_states(t, o, text, offs))
    want = case["ref_expect_accepted"]
    assert len(exp["hits"]) == t.RegexpsCount
    for r in range(t.RegexpsCount):
        assert exp["hits"][r].tolist() == [i for i, a in enumerate(want) if r in a]
        assert int(exp["counts"][r]) == sum(1 for a in want if r in a)


def test_validation_refuses_before_any_device_is_touched():
    _, t, _ = table_of("glue_ccc_aaa_bbb")
    L = pb.lib()
    idx = np.zeros(4, dtype=np.uint32)
    hits = np.zeros(3 * 4, dtype=np.uint64)
    spans = np.zeros(3 * 4 * 2, dtype=np.uint64)
    cnt = np.full(3, 77, dtype=np.uint64)
    lines = C.c_uint64(55)
    p, h, s, c, ln = idx.ctypes.data, hits.ctypes.data, spans.ctypes.data, cnt.ctypes.data, C.addressof(lines)
    offs = np.zeros(5, dtype=np.uint64)
    raw = np.frombuffer(b"aaa\nbbb\n", dtype=np.uint8)
    # (table, state_idx, out_hits, hit_cap, out_hit_counts)
    cases = {
        "null table": (None, p, h, 4, c),
        "null state_idx": (t._h, None, h, 4, c),
        "null out_hit_counts": (t._h, p, h, 4, None),
        "hit_cap > 0 with null out_hits": (t._h, p, None, 4, c),
    }
    for flags in (0, pb.FLAG_ON_DEVICE):
        for text, (th, pi, ph, cap, pc) in cases.items():
            assert L.pire_hip_route(th, pi, 4, flags, ph, cap, pc, None) == -1, text
            assert text in L.pire_hip_last_error().decode(), (text, L.pire_hip_last_error())
            if text == "null state_idx":   # the fused and lines forms have state indices of the library's own
                continue
            assert L.pire_hip_run_route(th, None, offs.ctypes.data, 4, BE | flags, None, None, None, None, ph, cap, pc, None) == -1
            assert text in L.pire_hip_last_error().decode()
            assert L.pire_hip_run_route_strided(th, None, 4, 0, 0, BE | flags, None, None, None, None, ph, cap, pc, None) == -1
            assert text in L.pire_hip_last_error().decode()
            assert L.pire_hip_run_lines_route(th, raw.ctypes.data, raw.size, 10, BE | flags, ln, ph, None, cap, pc, None) == -1
            assert text in L.pire_hip_last_error().decode()
        # the lines form's own refusals
        lines_cases = {
            "out_hit_spans without out_hits": (raw.ctypes.data, raw.size, 10, ln, None, s, 0),
            "delim > 255": (raw.ctypes.data, raw.size, 256, ln, h, s, 4),
            "null out_line_count": (raw.ctypes.data, raw.size, 10, None, h, s, 4),
            "size > 0 with null raw": (None, raw.size, 10, ln, h, s, 4),
        }
        for text, (pr, size, delim, pl, ph, ps, cap) in lines_cases.items():
            assert L.pire_hip_run_lines_route(t._h, pr, size, delim, BE | flags, pl, ph, ps, cap, c, None) == -1, text
            assert text in L.pire_hip_last_error().decode(), (text, L.pire_hip_last_error())
    assert cnt.tolist() == [77] * 3 and lines.value == 55 and not hits.any() and not spans.any()


def test_host_mode_edges_need_no_device():
    _, t, _ = table_of("glue_ccc_aaa_bbb")
    L = pb.lib()
    cnt = np.full(3, 77, dtype=np.uint64)
    bad = np.array([0, t.Size], dtype=np.uint32)
    assert L.pire_hip_route(t._h, bad.ctypes.data, 2, 0, None, 0, cnt.ctypes.data, None) == -1
    assert "out of range" in L.pire_hip_last_error().decode() and cnt.tolist() == [77] * 3
    # n == 0: R zero counts
    assert L.pire_hip_route(t._h, None, 0, 0, None, 0, cnt.ctypes.data, None) == 0 and cnt.tolist() == [0] * 3
    got = t.route(np.zeros(0, dtype=np.uint32))
    assert got["counts"].tolist() == [0, 0, 0] and [len(h) for h in got["hits"]] == [0, 0, 0]
    got = t.run_lines_route(b"")
    assert got["lines"] == 0 and got["counts"].tolist() == [0, 0, 0] and [s.shape for s in got["spans"]] == [(0, 2)] * 3
    # R == 0: OK, nothing is written, null counts are fine
    _, e, _ = table_of("empty_scanner")
    assert e.RegexpsCount == 0
    idx = np.zeros(5, dtype=np.uint32)
    poison = np.full(4, POISON, dtype=np.uint64)
    for flags in (0, pb.FLAG_ON_DEVICE):
        assert L.pire_hip_route(e._h, idx.ctypes.data, 5, flags, poison.ctypes.data, 4, poison.ctypes.data, None) == 0
        assert L.pire_hip_route(e._h, idx.ctypes.data, 5, flags, None, 0, None, None) == 0
    assert (poison == np.uint64(POISON)).all()
    got = e.route(idx)
    assert len(got["counts"]) == 0 and got["hits"] == []
    # n >= 2^32
    assert L.pire_hip_route(t._h, idx.ctypes.data, 1 << 32, pb.FLAG_ON_DEVICE, None, 0, cnt.ctypes.data, None) == -5   # PIRE_HIP_EUNSUPPORTED
    assert "2^32" in L.pire_hip_last_error().decode()


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_route_without_gpu_fails_loudly():
    _, t, _ = table_of("glue_ccc_aaa_bbb")
    text, offs = H.pack([b"aaa", b"bbb"])
    for call in (lambda: t.route(np.zeros(3, dtype=np.uint32)), lambda: t.run_route(text, offs),
                 lambda: t.run_route_strided(np.zeros((4, 16), dtype=np.uint8)), lambda: t.run_lines_route(b"aaa\nbbb\n")):
        with pytest.raises(pb.PireHipError) as e:
            call()
        assert e.value.code == -3 and "hip" in str(e.value).lower()


def test_the_route_unit_passes_the_build_audit():
    """route.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "route.hip" in ba.NO_SCRATCH and "route.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert mk.count("route.hip") == 2   # NAMES and AUDIT_UNITS
    names = [ln for ln in mk.splitlines() if ln.startswith("NAMES")][0]
    units = [ln for ln in mk.splitlines() if ln.startswith("AUDIT_UNITS")][0]
    assert names.count("route.hip") == 1 and units.count("route.hip") == 1
    fails, seen = ba.audit("route.hip")
    assert not fails, fails
    # (count and scatter; the scan is select.hip's SelectScanKernel, the lines form's spans split.hip's SplitSpansKernel: each
    # is audited with the unit it lives in)
    assert len(seen) == 2 and all("Route" in k for k in seen), seen


def test_the_route_pass_names_no_kernel_of_its_own():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "route.hip")) as f:
        assert "NoteKernel" not in f.read()


# ---- GPU: wrappers -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def u64(b):
    return b.cpu().numpy().view(np.uint64)


class DevOut:
    """The device-side outputs of one route call: poisoned, hits[R][cap] (+ spans), `guard` words behind each array."""

    def __init__(self, torch, t, cap, spans=False, guard=8):
        self.r, self.cap, self.guard = t.RegexpsCount, cap, guard
        poison = int(np.uint64(POISON).astype(np.int64))
        self.hits = torch.full((self.r * cap + guard,), poison, dtype=torch.int64, device="cuda")
        self.spans = torch.full((self.r * cap * 2 + guard,), poison, dtype=torch.int64, device="cuda") if spans else None
        self.counts = torch.full((self.r + guard,), poison, dtype=torch.int64, device="cuda")
        self.lines = torch.full((1,), poison, dtype=torch.int64, device="cuda")

    def ptrs(self):
        return dict(out_hit_counts_ptr=self.counts.data_ptr(), out_hits_ptr=self.hits.data_ptr() if self.cap else 0, hit_cap=self.cap)

    def fetch(self):
        """After a synchronise: the answer as Table.route returns it; whatever lies behind min(count, cap) of a row, and
        behind the arrays, must still be poison."""
        counts, hits = u64(self.counts), u64(self.hits)
        assert (counts[self.r:] == np.uint64(POISON)).all() and (hits[self.r * self.cap:] == np.uint64(POISON)).all()
        out = {"counts": counts[:self.r].copy(), "hits": []}
        rows = hits[:self.r * self.cap].reshape(self.r, self.cap)
        for r in range(self.r):
            k = min(int(counts[r]), self.cap)
            assert (rows[r, k:] == np.uint64(POISON)).all(), "row %d written behind min(count, hit_cap)" % r
            out["hits"].append(rows[r, :k].copy())
        if self.spans is not None:
            sp = u64(self.spans)
            assert (sp[self.r * self.cap * 2:] == np.uint64(POISON)).all()
            rows = sp[:self.r * self.cap * 2].reshape(self.r, self.cap, 2)
            out["spans"] = []
            for r in range(self.r):
                k = min(int(counts[r]), self.cap)
                assert (rows[r, k:] == np.uint64(POISON)).all(), "spans of row %d written behind its hits" % r
                out["spans"].append(rows[r, :k].copy())
        return out


def dev_idx(torch, idx):
    return torch.as_tensor(np.ascontiguousarray(idx, dtype=np.uint32).view(np.int32), device="cuda")


def dev_route(torch, t, idx, cap=None):
    n = len(idx)
    out = DevOut(torch, t, n if cap is None else cap)
    d = dev_idx(torch, idx) if n else None
    t.route_device(d.data_ptr() if n else 0, n, stream=torch.cuda.current_stream().cuda_stream, **out.ptrs())
    torch.cuda.synchronize()
    return out.fetch()


def host_route_raw(t, idx, cap):
    """pire_hip_route on poisoned host arrays: (counts u64[R], rows u64[R, cap])."""
    r = t.RegexpsCount
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    counts = np.full(r, POISON, dtype=np.uint64)
    hits = np.full(r * cap + 8, POISON, dtype=np.uint64)
    rc = pb.lib().pire_hip_route(t._h, idx.ctypes.data, len(idx), 0, hits.ctypes.data if cap else None, cap, counts.ctypes.data, None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    assert (hits[r * cap:] == np.uint64(POISON)).all()
    return counts, hits[:r * cap].reshape(r, cap)


# ---- GPU: parity ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,case", TS.parity_tables(), ids=lambda v: v if isinstance(v, str) else "")
def test_parity_and_cross_checks(torch_cuda, name, case):
    """Counts and all rows, host pointers and ON_DEVICE, against the helper; row r against Table.select(want=[r]); counts
    against the increments of out_counts[2 + r] of the same run."""
    torch = torch_cuda
    rng = np.random.RandomState(len(name) * 11 + 5)
    flags = BE
    if case is None:
        t, o, alphabet, flags = TS.wide_mask_table()
        assert t.RegexpsCount > 64 and t.mask_words >= 2
        strings = [bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=int(rng.randint(0, 5)))) for _ in range(3000)]
    else:
        blob = H.load_blob(case["blob"])
        t, o = pb.Table(blob), ob.OracleScanner(blob)
        base = H.case_strings(case) if "strings_hex" in case else [bytes.fromhex(h) for h in case["raw"]["strings_hex"]]
        alphabet = b"".join(base) or b"ab"
        strings = base * 4 + H.random_strings(rng, 1500, 24, alphabet) + [b""] * 3
        if "witnesses_hex" in case:
            wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]
            strings += [b"xx " + wit[int(rng.randint(len(wit)))] for _ in range(400)] + wit * 3
    strings = [strings[i] for i in rng.permutation(len(strings))]
    text, offs = H.pack(strings)
    idx = TS.end_states(t, o, text, offs, flags)
    exp = expected_route(t, idx)
    check(t.route(idx), exp)
    check(dev_route(torch, t, idx), exp)
    check(t.route(idx, device=True), exp)
    for r in range(t.RegexpsCount):
        sel = t.select(idx, want=[r], masks=False, hit_masks=False)
        assert sel["count"] == int(exp["counts"][r]) and (sel["hits"] == exp["hits"][r]).all(), r
    if t.RegexpsCount == 0:
        return
    # the fused call on the device, with the run's own counters
    n = len(strings)
    out = DevOut(torch, t, n)
    dt = torch.as_tensor(np.ascontiguousarray(text), device="cuda")
    do = torch.as_tensor(offs.view(np.int64), device="cuda")
    rc = torch.zeros(t.RegexpsCount + 2, dtype=torch.int64, device="cuda")
    di = torch.zeros(n, dtype=torch.int32, device="cuda")
    t.run_route_device(dt.data_ptr(), do.data_ptr(), n, flags, out_idx_ptr=di.data_ptr(), out_counts_ptr=rc.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream, **out.ptrs())
    torch.cuda.synchronize()
    got = out.fetch()
    assert (di.cpu().numpy().view(np.uint32) == idx).all()
    check(got, exp)
    assert u64(rc)[2:].tolist() == got["counts"].tolist() and int(u64(rc)[1]) == n


# ---- GPU: capacity -------------------------------------------------------------------------------------------------------

@gpu
def test_capacity(torch_cuda):
    """hit_cap in {0, 1, c-1, c, c+1} for a row with count c: exactly min(c_r, hit_cap) entries of each row change, the rest
    stay poison, the counts are always full -- device mode and host mode."""
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = state_pool(t, o, case)
    states = np.array(sorted(pool.values()), dtype=np.uint32)
    idx = states[np.random.RandomState(3).randint(len(states), size=2500)]
    exp = expected_route(t, idx)
    c = int(sorted(exp["counts"].tolist())[len(exp["counts"]) // 2])
    assert c > 2 and len(set(exp["counts"].tolist())) > 2
    for cap in (0, 1, c - 1, c, c + 1):
        check(dev_route(torch, t, idx, cap), exp, cap)
        counts, rows = host_route_raw(t, idx, cap)
        assert counts.tolist() == exp["counts"].tolist()
        for r in range(t.RegexpsCount):
            k = min(cap, int(exp["counts"][r]))
            assert (rows[r, :k] == exp["hits"][r][:k]).all() and (rows[r, k:] == np.uint64(POISON)).all(), (cap, r)
    # a capacity beyond the batch: the caller's pitch stays hit_cap where the host call stages min(hit_cap, n)
    counts, rows = host_route_raw(t, idx[:40], 100)
    e40 = expected_route(t, idx[:40])
    for r in range(t.RegexpsCount):
        k = int(e40["counts"][r])
        assert (rows[r, :k] == e40["hits"][r]).all() and (rows[r, k:] == np.uint64(POISON)).all()


# ---- GPU: the scan's carry -------------------------------------------------------------------------------------------------

@gpu
def test_every_rows_scan_carries_over_more_than_1024_tiles(torch_cuda):
    """(1 << 20) + 1025 strings are 1 026 tiles: the scan of every row takes a second step of 1 024 entries and carries the
    total of the first into it.  Synthetic state indices (no scan), three regexps with members behind tile 1 024; hit_cap = n:
    every row complete and ascending, counts exact; hit_cap = 1 000: counts still full, rows cut, the guard words untouched."""
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = state_pool(t, o, case)
    single = {r: s for k, s in pool.items() for r in k if len(k) == 1}
    rs = sorted(single)
    assert t.RegexpsCount >= 2 and len(rs) >= 3
    n = (1 << 20) + 1025
    rng = np.random.RandomState(31)
    choice = np.array([pool[frozenset()], pool[max(pool, key=len)]] + [single[r] for r in rs[:3]], dtype=np.uint32)
    idx = choice[rng.randint(len(choice), size=n)]
    idx[n - 1], idx[n - 2], idx[1024 * 1024 + 3] = single[rs[0]], single[rs[1]], single[rs[2]]
    exp = expected_route(t, idx)
    for r in rs[:3]:
        assert int(exp["hits"][r][-1]) >= 1024 * 1024 and int(exp["counts"][r]) > 1024
    check(dev_route(torch, t, idx), exp)
    check(dev_route(torch, t, idx, 1000), exp, 1000)


# ---- GPU: tile and wave edges ----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 16 * 1024 + 1])
def test_tile_and_wave_edges(torch_cuda, n):
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = state_pool(t, o, case)
    none = pool[frozenset()]
    richest = pool[max(pool, key=len)]
    single = {r: s for k, s in pool.items() for r in k if len(k) == 1}
    assert len(single) >= 3 and len(max(pool, key=len)) >= 1
    rs = sorted(single)
    # matches at the first and last lane of a wave and at the first and last string of a tile, nothing in between
    idx = np.full(n, none, dtype=np.uint32)
    for k, pos in enumerate([0, 63, 64, 127, 1023, 1024, 2047, 2048, n - 1]):
        if pos < n:
            idx[pos] = single[rs[k % len(rs)]]
    check(dev_route(torch, t, idx), expected_route(t, idx))
    check(t.route(idx), expected_route(t, idx))
    # every string matches every regexp it can; none matches
    full = np.full(n, richest, dtype=np.uint32)
    exp = expected_route(t, full)
    assert int(exp["counts"].max()) == n
    check(dev_route(torch, t, full), exp)
    got = dev_route(torch, t, np.full(n, none, dtype=np.uint32))
    assert got["counts"].tolist() == [0] * t.RegexpsCount
    # a random mix
    mix = np.array(sorted(pool.values()), dtype=np.uint32)[np.random.RandomState(n).randint(len(pool), size=n)]
    check(dev_route(torch, t, mix), expected_route(t, mix))


@gpu
def test_a_regexp_present_in_one_wave_of_a_tile_and_one_present_in_none(torch_cuda):
    """The loop over the wave's OR never visits a regexp the wave does not have: its count is a written zero all the same."""
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = state_pool(t, o, case)
    single = {r: s for k, s in pool.items() for r in k if len(k) == 1}
    rs = sorted(single)
    a, b = rs[0], rs[1]
    n = 3 * 1024 + 100
    idx = np.full(n, pool[frozenset()], dtype=np.uint32)
    idx[1024 + 5 * 64 + 7] = single[a]                  # regexp a: one string, wave 5 of tile 1
    idx[2 * 1024 + 64:2 * 1024 + 128] = single[b]       # regexp b: all of wave 1 of tile 2
    got = dev_route(torch, t, idx)
    exp = expected_route(t, idx)
    check(got, exp)
    assert got["counts"].tolist() == [1 if r == a else 64 if r == b else 0 for r in range(t.RegexpsCount)]
    assert got["hits"][a].tolist() == [1024 + 5 * 64 + 7]


@gpu
def test_strings_that_match_several_regexps(torch_cuda):
    """A string that matches k regexps is in k rows: the glued goldens, and the 128-regexp table whose final states accept 64
    regexps at once."""
    torch = torch_cuda
    for name in ("glue_aaa_bbb", "glue_ccc_aaa_bbb", "inline_glue3"):
        case, t, o = table_of(name)
        strings = (H.case_strings(case) + [b"aaabbb", b"bbbaaa", b"aaacccbbb", b"ccc", b"", b"ab"]) * 90
        text, offs = H.pack(strings)
        idx = TS.end_states(t, o, text, offs)
        exp = expected_route(t, idx)
        check(dev_route(torch, t, idx), exp)
        check(t.route(idx), exp)
    m = membership(t, idx)
    assert (m.sum(axis=1) > 1).any()
    t = TS.self_glued()
    assert t.RegexpsCount == 128
    rng = np.random.RandomState(8)
    strings = [bytes(rng.choice(np.frombuffer(b"abc", np.uint8), size=int(rng.randint(0, 9)))) for _ in range(2100)]
    text, offs = H.pack(strings)
    idx = t.run(text, offs)[0]
    exp = expected_route(t, idx)
    assert membership(t, idx).sum(axis=1).max() >= 64
    check(dev_route(torch, t, idx), exp)
    check(t.route(idx), exp)
    check(t.run_route(text, offs, states=False, device=True), exp)


# ---- GPU: the fused forms ----------------------------------------------------------------------------------------------------

@gpu
def test_fused_forms_against_route_after_run(torch_cuda):
    case, t, o = table_of("set_a")
    rng = np.random.RandomState(21)
    wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]
    strings = [b"xx " + wit[int(rng.randint(len(wit)))] if rng.randint(3) == 0 else bytes(rng.randint(32, 127, size=int(rng.randint(0, 60)), dtype=np.uint8))
               for _ in range(2300)]
    text, offs = H.pack(strings)
    idx = TS.end_states(t, o, text, offs)
    after = t.route(t.run(text, offs)[0])
    check(after, expected_route(t, idx))
    for device in (False, True):
        for states in (True, False):
            got = t.run_route(text, offs, states=states, device=device)
            check(got, after)
            if states:
                assert (got["idx"] == idx).all()
            else:
                assert got["idx"] is None
    # fixed-length records
    n, length = 1500, 64
    rec = rng.randint(97, 123, size=(n, length)).astype(np.uint8)
    for i in range(0, n, 3):
        s = np.frombuffer(wit[i % len(wit)][:length], np.uint8)
        rec[i, length - len(s):] = s
        rec[i, length - len(s) - 1] = 32
    ridx = TS.end_states(t, o, rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length)
    after = t.route(t.run_strided_host(rec)[0])
    check(after, expected_route(t, ridx))
    assert int(after["counts"].sum()) > 0
    for device in (False, True):
        for states in (True, False):
            got = t.run_route_strided(rec, states=states, device=device)
            check(got, after)
            if states:
                assert (got["idx"] == ridx).all()


@gpu
def test_host_batch_cut_into_chunks_keeps_indices_relative_to_the_whole_batch(torch_cuda):
    case, _, o = table_of("set_a")
    t = pb.Table(H.load_blob(case["blob"]))
    t.set_config(host_chunk_bytes=4096)   # this table's own configuration: the batch below is many chunks
    rng = np.random.RandomState(4)
    wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]
    strings = [bytes(rng.randint(97, 123, size=40, dtype=np.uint8)) + (b" " + wit[i % len(wit)] if i % 5 == 0 else b"") for i in range(3000)]
    text, offs = H.pack(strings)
    assert int(offs[-1]) > 20 * 4096
    exp = expected_route(t, TS.end_states(t, o, text, offs))
    assert int(exp["counts"].max()) > 0 and max(int(h[-1]) for h in exp["hits"] if len(h)) > 2900
    check(t.run_route(text, offs, states=False), exp)
    check(t.run_route(text, offs, states=True), exp)


# ---- GPU: the lines form -----------------------------------------------------------------------------------------------------

def lines_expectation(t, o, raw):
    """Python's own split of the buffer (getline's semantics), the oracle on the lines: (lines, spans per line, route answer)."""
    parts = raw.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    begin, spans = 0, []
    for p in parts:
        spans.append((begin, begin + len(p)))
        begin += len(p) + 1
    if not parts:
        return parts, spans, {"counts": np.zeros(t.RegexpsCount, dtype=np.uint64), "hits": [np.zeros(0, np.uint64)] * t.RegexpsCount}
    text, offs = H.pack(parts)
    return parts, spans, expected_route(t, TS.end_states(t, o, text, offs))


def lines_buffers():
    rng = np.random.RandomState(17)
    words = [b"aaa", b"bbb", b"ccc", b"aaabbb", b"xaaay", b"", b"nothing", b"cccbbbaaa", b"ab"]
    many = b"\n".join(words[int(rng.randint(len(words)))] + bytes(rng.choice(np.frombuffer(b"abc xyz", np.uint8), size=int(rng.randint(0, 12))))
                      for _ in range(2600))
    return {"many_lines": many + b"\n", "no_trailing_delimiter": many + b"\nbbb", "empty_lines": b"\n\naaa\n\n\nbbb\n\nccc aaa\n\n",
            "only_delimiters": b"\n" * 70, "one_line": b"aaa bbb", "size_0": b""}


@gpu
@pytest.mark.parametrize("which", sorted(lines_buffers()))
def test_lines_form(torch_cuda, which):
    torch = torch_cuda
    raw = lines_buffers()[which]
    case, t, o = table_of("glue_ccc_aaa_bbb")
    parts, spans, exp = lines_expectation(t, o, raw)
    for device in (False, True):
        got = t.run_lines_route(raw, device=device)
        assert got["lines"] == len(parts)
        check(got, exp)
        for r in range(t.RegexpsCount):
            assert got["spans"][r].tolist() == [list(spans[int(i)]) for i in exp["hits"][r]], r
            sel = t.run_lines_select_host(raw, want=[r], hit_masks=False)
            assert (sel["hits"] == got["hits"][r]).all() and (sel["spans"] == got["spans"][r]).all() and sel["count"] == int(got["counts"][r])
    if not raw:
        return
    # a capacity below the longest row, on poisoned arrays
    cap = max(1, int(exp["counts"].max()) // 2)
    out = DevOut(torch, t, cap, spans=True)
    d = torch.as_tensor(np.frombuffer(raw, np.uint8).copy(), device="cuda")
    t.run_lines_route_device(d.data_ptr(), len(raw), BE, out.lines.data_ptr(), out.counts.data_ptr(), out_hits_ptr=out.hits.data_ptr(),
                             out_hit_spans_ptr=out.spans.data_ptr(), hit_cap=cap, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.fetch()
    check(got, exp, cap)
    assert int(u64(out.lines)[0]) == len(parts)
    for r in range(t.RegexpsCount):
        assert got["spans"][r].tolist() == [list(spans[int(i)]) for i in exp["hits"][r][:cap]]


@gpu
def test_rows_chain_into_gathers_without_a_read_back(torch_cuda):
    """Device-mode run_lines_route, then pire_hip_gather_spans per regexp on spans + 2 * r * hit_cap and counts + r as they lie
    on the device; the host looks at nothing in between."""
    torch = torch_cuda
    raw = lines_buffers()["no_trailing_delimiter"]
    case, t, o = table_of("glue_ccc_aaa_bbb")
    parts, _, exp = lines_expectation(t, o, raw)
    r_count, cap = t.RegexpsCount, len(parts)
    stream = torch.cuda.current_stream().cuda_stream
    out = DevOut(torch, t, cap, spans=True)
    d = torch.as_tensor(np.frombuffer(raw, np.uint8).copy(), device="cuda")
    texts = [torch.zeros(len(raw) + cap + 16, dtype=torch.uint8, device="cuda") for _ in range(r_count)]
    offsets = [torch.zeros(cap + 1, dtype=torch.int64, device="cuda") for _ in range(r_count)]
    total = torch.zeros(r_count, dtype=torch.int64, device="cuda")
    t.run_lines_route_device(d.data_ptr(), len(raw), BE, out.lines.data_ptr(), out.counts.data_ptr(), out_hits_ptr=out.hits.data_ptr(),
                             out_hit_spans_ptr=out.spans.data_ptr(), hit_cap=cap, stream=stream)
    for r in range(r_count):
        pb.gather_spans_device(d.data_ptr(), len(raw), out.spans.data_ptr() + 16 * r * cap, total.data_ptr() + 8 * r,
                               span_count_ptr=out.counts.data_ptr() + 8 * r, span_cap=cap, tail=10, out_text_ptr=texts[r].data_ptr(),
                               text_cap=texts[r].numel(), out_offsets_ptr=offsets[r].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    check(out.fetch(), exp)
    for r in range(r_count):
        want = b"".join(parts[int(i)] + b"\n" for i in exp["hits"][r])
        assert int(u64(total)[r]) == len(want)
        assert texts[r].cpu().numpy()[:len(want)].tobytes() == want, r
        assert want[:-1] == b"\n".join(parts[int(i)] for i in exp["hits"][r])


# ---- GPU: determinism, undefined input -------------------------------------------------------------------------------------------

@gpu
def test_two_runs_give_the_same_bytes(torch_cuda):
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = np.array(sorted(state_pool(t, o, case).values()), dtype=np.uint32)
    idx = pool[np.random.RandomState(12).randint(len(pool), size=40000)]
    d = dev_idx(torch, idx)
    runs = []
    for _ in range(2):
        out = DevOut(torch, t, 9000)
        t.route_device(d.data_ptr(), len(idx), stream=torch.cuda.current_stream().cuda_stream, **out.ptrs())
        torch.cuda.synchronize()
        runs.append((u64(out.hits).tobytes(), u64(out.counts).tobytes()))
    assert runs[0] == runs[1]
    raw = lines_buffers()["many_lines"]
    _, g, _ = table_of("glue_ccc_aaa_bbb")
    a, b = g.run_lines_route(raw, device=True), g.run_lines_route(raw, device=True)
    for k in ("device_hits", "device_counts", "device_spans"):
        assert u64(a[k]).tobytes() == u64(b[k]).tobytes(), k


@gpu
def test_a_state_index_beyond_the_table_is_in_no_row(torch_cuda):
    torch = torch_cuda
    case, t, o = table_of("set_a")
    pool = np.array(sorted(state_pool(t, o, case).values()), dtype=np.uint32)
    idx = pool[np.random.RandomState(13).randint(len(pool), size=3000)]
    bad = idx.copy()
    where = [0, 63, 64, 1023, 1024, 2999]
    bad[where] = [t.Size, t.Size + 1, 0xFFFFFFFF, 0x7FFFFFFF, t.Size, 1 << 24]
    exp = expected_route(t, bad)          # (the helper gives such a string no regexp)
    got = dev_route(torch, t, bad)
    check(got, exp)
    ref = expected_route(t, idx)
    for r in range(t.RegexpsCount):
        assert got["hits"][r].tolist() == [i for i in ref["hits"][r].tolist() if i not in where]


# ---- the C++ shim ------------------------------------------------------------------------------------------------------------
# BatchRunner::Route / RouteCount / RouteHits / RouteSpans / DeviceRouteHits (include/pire_hip/batch_runner.hpp) against the C
# calls, compiled against the UNMODIFIED reference headers (tests/cpp/route_shim_test.cpp), the way tests/test_shim_cpp.py
# handles shim_test.cpp

REF_DIR = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(REF_DIR, "bin", "route_shim_test")
REF_PRESENT = os.path.exists(os.path.join(ob.REFERENCE_ROOT, "pire", "run.h"))


@pytest.mark.skipif(not REF_PRESENT, reason="the reference tree is not present (GPU box): the prebuilt binary is used there")
def test_route_shim_compiles_against_reference_headers():
    """tests/cpp/route_shim_test.cpp with the flags oracle/Makefile gives tests/cpp/shim_test.cpp, next to it in oracle/_ref/bin"""
    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = H.make_shim_program("route_shim_test")
    assert r.returncode == 0, r.stdout[-3000:]
    assert os.path.exists(BIN)


@gpu
def test_route_shim_agrees_with_the_c_calls_on_gpu():
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/bin/route_shim_test was not built (needs the reference tree at build time)")
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(route shim" in r.stdout
