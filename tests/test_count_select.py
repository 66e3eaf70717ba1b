"""pire_hip_count_select, the two run forms and the two lines forms: from counted matches to the strings that count, on the
device (count_select.hip).

Exact equality everywhere.  The expected values come from `model_count_select` -- the formulas of include/pire_hip.h written
down with numpy and held against a hand-written truth table --, applied, where a scan is involved, to what the C oracle's
counting and half-final walks say (tests/test_counting.py and tests/test_half_final.py hold them against the unmodified
reference; where that reference is built its numbers are compared here once more), and for lines to Python's own split.
Nothing expected comes from the library.  Every output of a call sits between poisoned guard bytes and is compared bytewise,
what the call had no business writing included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5
GUARD = 64                     # poisoned bytes around every output
EINVAL, EUNSUPPORTED = -1, -5
gpu = pytest.mark.gpu
NAMES = ("pire_hip_count_select", "pire_hip_counting_run_select", "pire_hip_run_half_final_select", "pire_hip_counting_lines_select",
         "pire_hip_half_final_lines_select")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


# ---- the model -----------------------------------------------------------------------------------------------------------

def model_count_select(results, min_count=None, all_=False):
    """include/pire_hip.h: totals[R], hits (every one of them), their rows, the count"""
    results = np.asarray(results, dtype=np.uint32)
    n, R = results.shape
    m = np.ones(R, dtype=np.uint32) if min_count is None else np.asarray(min_count, dtype=np.uint32)
    assert m.shape == (R,)
    wanted = m > 0
    passed = results >= m[None, :]
    if not wanted.any():
        sel = np.zeros(n, dtype=bool)
    elif all_:
        sel = passed[:, wanted].all(axis=1)
    else:
        sel = passed[:, wanted].any(axis=1)
    totals = np.zeros(R, dtype=np.uint64)
    for r in range(R):
        totals[r] = sum(int(x) for x in results[:, r].tolist()) if n < 4096 else int(results[:, r].astype(np.uint64).sum(dtype=np.uint64))
    return {"totals": totals, "hits": np.flatnonzero(sel).astype(np.uint64), "rows": results[sel], "count": int(sel.sum())}


BIG = 0xFFFFFFFF
HAND_ROWS = [[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 1, 1], [BIG, 0, 5], [2, 2, 2]]
# (min_count, ALL) -> the selected rows
HAND = [
    (None, False, [1, 2, 3, 4, 5]),              # NULL: 1 for every regexp
    (None, True, [3, 5]),
    ((1, 1, 1), False, [1, 2, 3, 4, 5]),
    ((3, 0, 2), False, [3, 4, 5]),               # an entry of 0: that regexp is not asked
    ((3, 0, 2), True, [4]),
    ((0, 2, 0), False, [2, 5]),
    ((0, 2, 0), True, [2, 5]),
    ((0, 0, 0), False, []),                      # all entries 0: nothing is wanted, nothing is selected
    ((0, 0, 0), True, []),
    ((BIG, 0, 0), False, [4]),                   # an entry of 0xFFFFFFFF: only that very count reaches it
    ((BIG, 0, 0), True, [4]),
    ((BIG, 1, 0), False, [2, 3, 4, 5]),
    ((BIG, 1, 0), True, []),
    ((BIG, 0, 6), False, [4]),
    ((BIG, 0, 6), True, []),
]


def test_the_model_against_a_hand_written_truth_table():
    res = np.array(HAND_ROWS, dtype=np.uint32)
    for m, all_, want in HAND:
        got = model_count_select(res, m, all_)
        assert got["hits"].tolist() == want and got["count"] == len(want), (m, all_, got["hits"])
        assert got["rows"].tolist() == [HAND_ROWS[i] for i in want]
        assert got["totals"].tolist() == [BIG + 6, 5, 8]                   # over ALL strings, selected or not; beyond 32 bits
    empty = model_count_select(np.zeros((0, 3), dtype=np.uint32), None, False)
    assert empty["totals"].tolist() == [0, 0, 0] and empty["count"] == 0
    none = model_count_select(np.zeros((4, 0), dtype=np.uint32), None, True)
    assert none["count"] == 0 and none["totals"].size == 0


# ---- the fixtures, their batch and what the oracle says (shared; the oracle runs once per table and flag combination) ------------

COUNTING = ("count_glued3_basic", "count_glued3_advanced", "count_glued3_noglue", "count_wide17_noglue")
HALF = ("half_0", "half_5")
GLUED3 = (((8, 0, 0), False), ((0, 1, 1), False), ((1, 0, 1), True), ((12, 1, 1), False))
SELECTIONS = {"count_glued3_basic": GLUED3, "count_glued3_advanced": GLUED3, "count_glued3_noglue": GLUED3,
              "count_wide17_noglue": (((2,) + (0,) * 16, False), ((1,) * 17, False)),
              "half_0": (((2,) * 5, True), ((0, 0, 0, 3, 0), False)), "half_5": (((2,) * 5, True), ((0, 0, 0, 3, 0), False))}
# the shares the issue states, under BEGIN | END
SHARES = {("count_glued3_advanced", 0): 0.479, ("count_glued3_advanced", 1): 0.069, ("count_glued3_advanced", 2): 0.053,
          ("count_glued3_advanced", 3): 0.247, ("count_wide17_noglue", 0): 0.100, ("count_wide17_noglue", 1): 0.984, ("half_0", 0): 0.166,
          ("half_0", 1): 0.068}
_batch, _oracle = [], {}


def batch():
    if not _batch:
        _batch.extend(H.random_strings(np.random.RandomState(7), 3000, 200, b"abc http xyz") + [b""] * 3)
    return _batch


def case_of(name):
    return [c for c in H.golden()["counting" if name in COUNTING else "half_final"] if c["name"] == name][0]


def oracle_results(name, flags, strings=None):
    """results[n, R] of the batch (or of `strings`) from the C oracle; where the reference is built, it agrees"""
    key = (name, flags)
    if strings is None and key in _oracle:
        return _oracle[key]
    many = batch() if strings is None else strings
    blob = H.load_blob(case_of(name)["blob"])
    if name in COUNTING:
        kind = case_of(name)["kind"]
        _, res = ob.OracleCountingScanner(blob, kind).run_strings(many, flags=flags)
        if ob.ref_available() and many:
            assert (ob.RefCountingScanner.load(kind, blob).run_strings(many, flags=flags)[1] == res).all()
    else:
        _, _, res = ob.OracleScanner(blob).run_half_final(*ob.pack_strings(many), flags=flags)
        if ob.ref_available() and many:
            assert (ob.RefHalfFinalScanner.load(blob).run_strings(many, flags=flags)[2] == res).all()
    res = np.ascontiguousarray(res, dtype=np.uint32).reshape(len(many), -1)
    if strings is None:
        res.setflags(write=False)
        _oracle[key] = res
    return res


def table_of(name):
    blob = H.load_blob(case_of(name)["blob"])
    return pb.CountingTable(blob, case_of(name)["kind"]) if name in COUNTING else pb.Table(blob)


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
    assert re.search(r"#define PIRE_HIP_COUNT_ALL 0x1u", src) and pb.COUNT_ALL == 1
    assert src.index("the strings that count, on the device") < src.index("int pire_hip_count_select(")


def _guarded(R=3, cap=4):
    return {"totals": np.full(8 * (R + 2), POISON, dtype=np.uint8), "hits": np.full(8 * (cap + 2), POISON, dtype=np.uint8),
            "rows": np.full(4 * (cap * R + 2), POISON, dtype=np.uint8), "spans": np.full(8 * (2 * cap + 2), POISON, dtype=np.uint8)}


def _untouched(bufs):
    return all((b == POISON).all() for b in bufs.values())


def test_count_select_refuses_before_any_device_is_touched():
    L = pb.lib()
    res = np.array(HAND_ROWS, dtype=np.uint32)
    m = np.array([1, 0, 1], dtype=np.uint32)
    bufs, cnt = _guarded(), C.c_uint64(77)
    r, mp, t, h, w, c = res.ctypes.data, m.ctypes.data, bufs["totals"].ctypes.data, bufs["hits"].ctypes.data, bufs["rows"].ctypes.data, C.addressof(cnt)
    wide = np.zeros(1025, dtype=np.uint32)
    cases = {
        "null out_hit_count": (EINVAL, (r, 6, 3, mp, 0, t, h, w, 4, None)),
        "n > 0 with null results": (EINVAL, (None, 6, 3, mp, 0, t, h, w, 4, c)),
        "unknown bits in mode": (EINVAL, (r, 6, 3, mp, 2, t, h, w, 4, c)),
        "unknown bits in mode ": (EINVAL, (r, 6, 3, mp, 0x80000001, t, h, w, 4, c)),
        "hit_cap > 0 with null out_hits and null out_hit_results": (EINVAL, (r, 6, 3, mp, 1, t, None, None, 4, c)),
        "2^32 strings or more": (EUNSUPPORTED, (r, 1 << 32, 3, mp, 0, t, h, w, 4, c)),
        "more than 1024 regexps": (EUNSUPPORTED, (wide.ctypes.data, 1, 1025, None, 0, None, h, None, 4, c)),
    }
    for what, (code, (a_r, n, R, a_m, mode, a_t, a_h, a_w, cap, a_c)) in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            assert L.pire_hip_count_select(a_r, n, R, a_m, mode, flags, a_t, a_h, a_w, cap, a_c, None) == code, what
            msg = L.pire_hip_last_error().decode()
            assert what.strip() in msg and msg.startswith("pire_hip_count_select: "), (what, msg)
    assert cnt.value == 77 and _untouched(bufs)


def _run_form_cases(t_handle, x, o, bufs, cnt):
    t, h, w, c = bufs["totals"].ctypes.data, bufs["hits"].ctypes.data, bufs["rows"].ctypes.data, C.addressof(cnt)
    return {
        "null out_hit_count": (EINVAL, (t_handle, x, o, 2, None, 0, t, h, w, 4, None)),
        "unknown bits in mode": (EINVAL, (t_handle, x, o, 2, None, 6, t, h, w, 4, c)),
        "hit_cap > 0 with null out_hits and null out_hit_results": (EINVAL, (t_handle, x, o, 2, None, 0, t, None, None, 4, c)),
        "2^32 strings or more": (EUNSUPPORTED, (t_handle, x, o, 1 << 32, None, 0, t, h, w, 4, c)),
        "argument": (EINVAL, (None, x, o, 2, None, 0, t, h, w, 4, c)),                     # what the run call refuses: no table,
        "argument ": (EINVAL, (t_handle, x, None, 2, None, 0, t, h, w, 4, c)),             # ... no offsets
    }


def test_the_run_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    text, offs = H.pack([b"abc http", b"xyz"])
    text, offs = text.copy(), offs.copy()
    for name in ("count_glued3_advanced", "half_0"):
        tab = table_of(name)
        who = "pire_hip_counting_run_select" if name in COUNTING else "pire_hip_run_half_final_select"
        bufs, cnt = _guarded(tab.RegexpsCount), C.c_uint64(77)
        for what, (code, (a_t, a_x, a_o, n, a_m, mode, t, h, w, cap, c)) in _run_form_cases(tab._h, text.ctypes.data, offs.ctypes.data, bufs, cnt).items():
            for flags in (3, 3 | pb.FLAG_ON_DEVICE):
                if name in COUNTING:
                    rc = L.pire_hip_counting_run_select(a_t, tab.kind, a_x, a_o, n, flags, None, None, a_m, mode, t, h, w, cap, c, None)
                else:
                    rc = L.pire_hip_run_half_final_select(a_t, a_x, a_o, n, flags, None, None, None, a_m, mode, t, h, w, cap, c, None)
                msg = L.pire_hip_last_error().decode()
                assert rc == code and what.strip() in msg and msg.startswith(who + ": "), (name, what, rc, msg)
        assert cnt.value == 77 and _untouched(bufs)


def test_the_lines_forms_refuse_before_any_device_is_touched():
    L = pb.lib()
    raw = u8(b"abc http\nxyz\n").copy()
    for name in ("count_glued3_advanced", "half_0"):
        tab = table_of(name)
        who = "pire_hip_counting_lines_select" if name in COUNTING else "pire_hip_half_final_lines_select"
        bufs, cnt, lines = _guarded(tab.RegexpsCount), C.c_uint64(77), C.c_uint64(78)
        r, lp, t, h, s, w, c = (raw.ctypes.data, C.addressof(lines), bufs["totals"].ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data,
                                bufs["rows"].ctypes.data, C.addressof(cnt))
        cases = {
            "null table": (None, r, raw.size, 10, 0, lp, t, h, s, w, 4, c),
            "delim > 255": (tab._h, r, raw.size, 300, 0, lp, t, h, s, w, 4, c),
            "null out_line_count": (tab._h, r, raw.size, 10, 0, None, t, h, s, w, 4, c),
            "size > 0 with null raw": (tab._h, None, raw.size, 10, 0, lp, t, h, s, w, 4, c),
            "null out_hit_count": (tab._h, r, raw.size, 10, 0, lp, t, h, s, w, 4, None),
            "unknown bits in mode": (tab._h, r, raw.size, 10, 4, lp, t, h, s, w, 4, c),
            "hit_cap > 0 with null out_hits and null out_hit_results": (tab._h, r, raw.size, 10, 1, lp, t, None, None, None, 4, c),
            "out_hit_spans without out_hits": (tab._h, r, raw.size, 10, 1, lp, t, None, s, w, 4, c),
        }
        for what, (a_t, a_r, size, delim, mode, a_l, a_tot, a_h, a_s, a_w, cap, a_c) in cases.items():
            for flags in (3, 3 | pb.FLAG_ON_DEVICE):
                if name in COUNTING:
                    rc = L.pire_hip_counting_lines_select(a_t, tab.kind, a_r, size, delim, flags, None, mode, a_l, a_tot, a_h, a_s, a_w, cap, a_c, None)
                else:
                    rc = L.pire_hip_half_final_lines_select(a_t, a_r, size, delim, flags, None, mode, a_l, a_tot, a_h, a_s, a_w, cap, a_c, None)
                msg = L.pire_hip_last_error().decode()
                assert rc == EINVAL and what in msg and msg.startswith(who + ": "), (name, what, rc, msg)
        assert (cnt.value, lines.value) == (77, 78) and _untouched(bufs)


def test_empty_host_calls_answer_zeros_without_a_device():
    L = pb.lib()
    for R in (3, 5, 0):
        bufs, cnt = _guarded(max(R, 1)), C.c_uint64(77)
        t, h, w, c = bufs["totals"].ctypes.data, bufs["hits"].ctypes.data, bufs["rows"].ctypes.data, C.addressof(cnt)
        dummy = np.zeros(16, dtype=np.uint32)
        # no string (R zeros for the totals), or strings of no regexp (a count of 0 and nothing else)
        for res, n in ((None, 0), (dummy.ctypes.data, 0)) if R else ((None, 4), (dummy.ctypes.data, 4)):
            cnt.value = 77
            assert L.pire_hip_count_select(res, n, R, None, 1, 0, t, h, w, 4, c, None) == 0, L.pire_hip_last_error()
            assert cnt.value == 0
            tot = bufs["totals"].view(np.uint64)
            assert tot[:R].tolist() == [0] * R and (bufs["totals"][8 * R:] == POISON).all()
            assert (bufs["hits"] == POISON).all() and (bufs["rows"] == POISON).all()
            bufs["totals"][:] = POISON
    offs0 = np.zeros(1, dtype=np.uint64)
    for name in ("count_glued3_advanced", "count_wide17_noglue", "half_0"):
        tab = table_of(name)
        R = tab.RegexpsCount
        bufs, cnt, lines = _guarded(R), C.c_uint64(77), C.c_uint64(78)
        t, h, s, w, c, lp = (bufs["totals"].ctypes.data, bufs["hits"].ctypes.data, bufs["spans"].ctypes.data, bufs["rows"].ctypes.data,
                             C.addressof(cnt), C.addressof(lines))
        for form in ("run", "lines"):
            cnt.value, lines.value = 77, 78
            bufs["totals"][:] = POISON
            if form == "run" and name in COUNTING:
                rc = L.pire_hip_counting_run_select(tab._h, tab.kind, None, offs0.ctypes.data, 0, 3, None, None, None, 0, t, h, w, 4, c, None)
            elif form == "run":
                rc = L.pire_hip_run_half_final_select(tab._h, None, offs0.ctypes.data, 0, 3, None, None, None, None, 0, t, h, w, 4, c, None)
            elif name in COUNTING:
                rc = L.pire_hip_counting_lines_select(tab._h, tab.kind, None, 0, 10, 3, None, 0, lp, t, h, s, w, 4, c, None)
            else:
                rc = L.pire_hip_half_final_lines_select(tab._h, None, 0, 10, 3, None, 0, lp, t, h, s, w, 4, c, None)
            assert rc == 0, (name, form, L.pire_hip_last_error())
            assert cnt.value == 0 and lines.value == (0 if form == "lines" else 78)
            assert bufs["totals"].view(np.uint64)[:R].tolist() == [0] * R and (bufs["totals"][8 * R:] == POISON).all()
            assert (bufs["hits"] == POISON).all() and (bufs["rows"] == POISON).all() and (bufs["spans"] == POISON).all()
        # the wrappers on nothing
        if name in COUNTING:
            got, gl = tab.run_select(np.zeros(0, np.uint8), offs0), tab.lines_select_host(b"")
        else:
            got, gl = tab.run_half_final_select(np.zeros(0, np.uint8), offs0), tab.half_final_lines_select_host(b"")
        for g in (got, gl):
            assert g["count"] == 0 and g["totals"].tolist() == [0] * R and g["hits"].size == 0 and g["hit_results"].shape == (0, R)
        assert gl["lines"] == 0 and gl["spans"].shape == (0, 2)
    got = pb.count_select_host(np.zeros((0, 3), dtype=np.uint32), min_count=[1, 2, 3], all=True)
    assert got["count"] == 0 and got["totals"].tolist() == [0, 0, 0] and got["hits"].size == 0


@pytest.mark.parametrize("name", COUNTING + HALF)
def test_every_selection_of_the_gpu_part_selects_some_strings_and_not_all(name):
    """... between 1 % and 99 % of them on the oracle's own numbers, and some total exceeds the hit count: neither list, count
    nor totals of the GPU part can be right by being empty, full or equal"""
    assert len(batch()) == 3003 and batch()[-3:] == [b"", b"", b""]
    for flags in (3, 0):
        res = oracle_results(name, flags)
        assert res.shape == (3003, case_of(name)["regexps"])
        for k, (m, all_) in enumerate(SELECTIONS[name]):
            exp = model_count_select(res, m, all_)
            share = exp["count"] / len(res)
            assert 0.01 <= share <= 0.99, (name, flags, m, all_, share)
            assert int(exp["totals"].max()) > exp["count"], (name, flags, m, exp["totals"], exp["count"])
            if flags == 3 and (name, k) in SHARES:
                assert round(share, 3) == SHARES[(name, k)], (name, k, share)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """count_select.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "count_select.hip" in ba.NO_SCRATCH and "count_select.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"^CNTSEL\s*:= count_select\$\(suffix \.hip\)$", mk, re.M)) == 1 and mk.count("$(CNTSEL)") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("count_select.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Count" in k for k in seen), seen               # classify with and without sums, totals, scatter


def test_the_pass_names_no_kernel_and_reads_no_environment():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "count_select.hip")) as f:
        src = f.read()
    assert "NoteKernel" not in src and "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")


# ---- GPU: the harness ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


class Outs:
    """The outputs of one call, host or device, each `bytes` long between GUARD poisoned bytes; check() compares every one of
    them bytewise with what the model says the call writes -- and leaves alone."""

    def __init__(self, torch, device, R, cap, totals=True, hits=True, rows=True, spans=False, lines=False):
        self.torch, self.device, self.R, self.cap = torch, device, R, cap
        sizes = {"count": 8, "totals": 8 * R if totals else None, "hits": 8 * cap if hits else None, "rows": 4 * cap * R if rows else None,
                 "spans": 16 * cap if spans else None, "lines": 8 if lines else None}
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

    def check(self, exp, what="", spans=None, lines=None):
        """exp: the model's answer with every hit; the first min(count, cap) entries of the lists, and nothing else, were written"""
        now = self.read()
        k = min(exp["count"], self.cap)
        want = {"count": np.array([exp["count"]], dtype=np.uint64), "totals": exp["totals"].astype(np.uint64), "hits": exp["hits"][:k].astype(np.uint64),
                "rows": np.ascontiguousarray(exp["rows"][:k], dtype=np.uint32), "spans": None if spans is None else np.ascontiguousarray(spans[:k], dtype=np.uint64),
                "lines": None if lines is None else np.array([lines], dtype=np.uint64)}
        for name, got in now.items():
            payload = want[name].tobytes()
            full = np.full(len(got), POISON, dtype=np.uint8)
            full[GUARD:GUARD + len(payload)] = u8(payload)
            bad = np.flatnonzero(got != full)
            assert bad.size == 0, (what, name, "first differing byte %d of %d (payload %d bytes)" % (bad[0] - GUARD, len(got) - 2 * GUARD, len(payload)))
        return now


def call_pass(torch, device, res, ptr, m, all_, cap, totals=True, hits=True, rows=True, dev_min=None):
    n, R = res.shape
    out = Outs(torch, device, R, cap, totals, hits, rows)
    mp = None if m is None else (dev_min.data_ptr() if device else m.ctypes.data)
    rc = pb.lib().pire_hip_count_select(ptr, n, R, mp, pb.COUNT_ALL if all_ else 0, pb.FLAG_ON_DEVICE if device else 0, out.ptr("totals"),
                                        out.ptr("hits"), out.ptr("rows"), cap, out.ptr("count"), None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out


# ---- GPU: the pass alone -----------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5127)
WIDTHS = (1, 3, 5, 16, 17, 40)
SHAPES = sorted({(n, WIDTHS[(k + j) % len(WIDTHS)]) for k, n in enumerate(SIZES) for j in (0, 1)})


def test_the_synthetic_shapes_cover_every_size_and_width_twice():
    assert all(sum(1 for s in SHAPES if s[0] == n) == 2 for n in SIZES) and all(sum(1 for s in SHAPES if s[1] == R) >= 2 for R in WIDTHS)


@gpu
@pytest.mark.parametrize("n,R", SHAPES)
def test_the_pass_alone_on_synthetic_results(torch_cuda, n, R):
    torch = torch_cuda
    rng = np.random.RandomState(n * 41 + R)
    # the rows 4 bytes behind a 16-byte boundary, on the host and on the device
    room = np.zeros(n * R + 8, dtype=np.uint32)
    lead = 1 + (-(room.ctypes.data // 4) % 4)
    res = room[lead:lead + n * R].reshape(n, R)
    res[:] = rng.randint(0, 5, size=(n, R))
    assert res.ctypes.data % 16 == 4
    dev_room = torch.as_tensor(i64(np.concatenate([np.zeros(1, np.uint32), res.reshape(-1), np.zeros(1 + (n * R) % 2, np.uint32)])), device="cuda")
    dev_ptr = dev_room.data_ptr() + 4
    assert dev_ptr % 16 == 4
    mins = [None, rng.randint(0, 4, size=R).astype(np.uint32), np.zeros(R, dtype=np.uint32)]
    if R > 1:
        mins[1][0], mins[1][1] = 0, 2                         # an entry that is not asked, one that is
    else:
        mins[1][0] = 2
    calls = 0
    for m in mins:
        dev_min = None if m is None else torch.as_tensor(m.astype(np.int32), device="cuda")
        for all_ in (False, True):
            exp = model_count_select(res, m, all_)
            count = exp["count"]
            if m is not None and not m.any():
                assert count == 0
            for cap in sorted({c for c in (0, 1, count - 1, count, count + 5) if c >= 0}):
                for device in (True, False):
                    ptr = dev_ptr if device else res.ctypes.data
                    what = (n, R, None if m is None else m.tolist(), all_, cap, "device" if device else "host")
                    first = call_pass(torch, device, res, ptr, m, all_, cap, dev_min=dev_min).check(exp, what)
                    calls += 1
                    if device and cap == count:
                        again = call_pass(torch, device, res, ptr, m, all_, cap, dev_min=dev_min).check(exp, what)      # the same input: the same bits
                        assert all(first[k].tobytes() == again[k].tobytes() for k in first)
                        # one list without the other, no totals (the classify kernel without its sums), no list at all
                        call_pass(torch, True, res, ptr, m, all_, cap, totals=False, rows=False, dev_min=dev_min).check(exp, what)
                        call_pass(torch, True, res, ptr, m, all_, cap, hits=False, dev_min=dev_min).check(exp, what)
                        call_pass(torch, True, res, ptr, m, all_, 0, totals=False, hits=False, rows=False, dev_min=dev_min).check(exp, what)
    assert calls >= 24
    got = dev_room.cpu().numpy().view(np.uint32)
    assert (got[1:1 + n * R] == res.reshape(-1)).all() and got[0] == 0, "the input was written to"
    # the wrappers
    w = pb.count_select_host(res, min_count=mins[1], all=True)
    exp = model_count_select(res, mins[1], True)
    assert w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all() and (w["hit_results"] == exp["rows"]).all() and (w["totals"] == exp["totals"]).all()


@gpu
@pytest.mark.parametrize("R", (1, 3))
def test_no_strings_from_host_pointers_and_on_the_device(torch_cuda, R):
    """n == 0: a count of 0 and R totals of 0, whatever the capacity; no list is touched, on either side"""
    torch = torch_cuda
    res = np.zeros((0, R), dtype=np.uint32)
    room = np.zeros(4, dtype=np.uint32)                       # (somewhere to point: nothing of it is read)
    dev_room = torch.zeros(4, dtype=torch.int32, device="cuda")
    m = np.full(R, 2, dtype=np.uint32)
    dev_min = torch.as_tensor(m.astype(np.int32), device="cuda")
    for mins in (None, m):
        for all_ in (False, True):
            exp = model_count_select(res, mins, all_)
            assert exp["count"] == 0 and exp["totals"].tolist() == [0] * R
            for cap in (0, 5):
                for device in (True, False):
                    ptr = dev_room.data_ptr() if device else room.ctypes.data
                    what = (R, None if mins is None else mins.tolist(), all_, cap, "device" if device else "host")
                    call_pass(torch, device, res, ptr, mins, all_, cap, dev_min=dev_min).check(exp, what)
                    call_pass(torch, device, res, ptr, mins, all_, cap, totals=False, dev_min=dev_min).check(exp, what)
    assert not dev_room.cpu().numpy().any()


@gpu
def test_totals_beyond_32_bits(torch_cuda):
    torch = torch_cuda
    n = 2049
    res = np.empty((n, 2), dtype=np.uint32)
    res[:, 0] = BIG
    res[:, 1] = np.arange(n)
    totals = [n * BIG, n * (n - 1) // 2]
    assert totals[0] > 1 << 42 and 1024 * BIG > 1 << 32                    # one tile's sum alone does not fit 32 bits
    dev = torch.as_tensor(res.view(np.int32), device="cuda")
    for m, want in (((BIG, 0), list(range(n))), ((0, 2048), [n - 1]), ((BIG, 2048), [n - 1])):
        m = np.array(m, dtype=np.uint32)
        dev_min = torch.as_tensor(m.view(np.int32), device="cuda")
        for all_ in (False, True):
            exp = model_count_select(res, m, all_)
            if not (all_ is False and tuple(m) == (BIG, 2048)):
                assert exp["hits"].tolist() == want
            assert exp["totals"].tolist() == totals
            for device in (True, False):
                call_pass(torch, device, res, dev.data_ptr() if device else res.ctypes.data, m, all_, n, dev_min=dev_min).check(exp, (tuple(m), all_, device))


@gpu
def test_more_tiles_than_the_grid_has_blocks(torch_cuda):
    """8 192 blocks at the most walk the tiles (compact.h kTileMaxBlocks behind tile_pass.h TilePass::Grid(), the grid of the unit's
    classify kernels and of the shared scatter, as the siblings'): 8 194 tiles, and a tile scan of nine steps"""
    torch = torch_cuda
    csrc = os.path.join(ROOT, "pire_amd", "csrc")
    with open(os.path.join(csrc, "compact.h")) as f:
        assert re.search(r"kTileMaxBlocks = 8192;", f.read())
    with open(os.path.join(csrc, "tile_pass.h")) as f:
        assert "dim3 Grid() const { return dim3(std::min(s.tiles, kTileMaxBlocks)); }" in f.read()
    with open(os.path.join(csrc, "count_select.hip")) as f:
        src = f.read()
    assert src.count("hipLaunchKernelGGL(CountClassifyKernel<") == src.count(">, t.Grid(), dim3(kBlockThreads)") == 2
    n = (1 << 23) + 1025
    assert (n + 1023) // 1024 > 8192
    res = (np.arange(n) % 7 == 0).astype(np.uint32).reshape(n, 1)
    dev = torch.as_tensor(res.view(np.int32), device="cuda")
    exp = model_count_select(res, None, False)
    assert exp["count"] == (n + 6) // 7 == int(exp["totals"][0]) and (exp["hits"] == np.arange(0, n, 7)).all()
    call_pass(torch, True, res, dev.data_ptr(), None, False, exp["count"] + 5).check(exp, "2^23 + 1025")
    dev_min = torch.as_tensor(np.array([1], dtype=np.int32), device="cuda")
    call_pass(torch, True, res, dev.data_ptr(), np.array([1], dtype=np.uint32), True, 1000, rows=False, dev_min=dev_min).check(exp, "2^23 + 1025, cap 1000")


# ---- GPU: behind the counting and the half-final kernels -----------------------------------------------------------------------

def run_form(torch, tab, name, device, text, offs, flags, m, all_, cap, keep_results, dev_batch=None):
    """the run + pass call; keep_results: the caller has out_state_idx / out_final / out_results (poisoned first)"""
    n, R = len(offs) - 1, tab.RegexpsCount
    out = Outs(torch, device, R, cap)
    own = None
    if keep_results:
        own = {"idx": np.full(n, 0xA5A5A5A5, dtype=np.uint32), "final": np.full(n, POISON, dtype=np.uint8), "results": np.full((n, R), 0xA5A5A5A5, dtype=np.uint32)}
        if device:
            own = {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v, device="cuda") for k, v in own.items()}
    p = (lambda k: None) if own is None else (lambda k: own[k].data_ptr() if device else own[k].ctypes.data)
    mp = None
    if m is not None:
        m = np.asarray(m, dtype=np.uint32)
        keep = torch.as_tensor(m.view(np.int32), device="cuda") if device else m
        mp = keep.data_ptr() if device else keep.ctypes.data
    if device:
        tp, op = dev_batch[0].data_ptr(), dev_batch[1].data_ptr()
    else:
        tp, op = text.ctypes.data, offs.ctypes.data
    f = flags | (pb.FLAG_ON_DEVICE if device else 0)
    mode = pb.COUNT_ALL if all_ else 0
    if name in COUNTING:
        rc = pb.lib().pire_hip_counting_run_select(tab._h, tab.kind, tp, op, n, f, p("idx"), p("results"), mp, mode, out.ptr("totals"), out.ptr("hits"),
                                                   out.ptr("rows"), cap, out.ptr("count"), None)
    else:
        rc = pb.lib().pire_hip_run_half_final_select(tab._h, tp, op, n, f, p("idx"), p("final"), p("results"), mp, mode, out.ptr("totals"),
                                                     out.ptr("hits"), out.ptr("rows"), cap, out.ptr("count"), None)
    assert rc == 0, pb.lib().pire_hip_last_error()
    if own is not None and device:
        torch.cuda.synchronize()
        own = {k: v.cpu().numpy() for k, v in own.items()}
    return out, own


@gpu
@pytest.mark.parametrize("name", COUNTING + HALF)
def test_behind_the_counting_kernels(torch_cuda, name):
    torch = torch_cuda
    tab = table_of(name)
    text, offs = H.pack(batch())
    text, offs = text.copy(), offs.copy()
    n = len(offs) - 1
    dev_batch = (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))
    for flags in (3, 0):
        res = oracle_results(name, flags)
        for k, (m, all_) in enumerate(SELECTIONS[name]):
            exp = model_count_select(res, m, all_)
            for device in (True, False):
                for keep in (True, False):
                    cap = n if keep else max(exp["count"] - 1, 0)
                    what = (name, flags, m, all_, "device" if device else "host", keep, cap)
                    out, own = run_form(torch, tab, name, device, text, offs, flags, m, all_, cap, keep, dev_batch)
                    out.check(exp, what)
                    if keep:
                        assert (own["results"].view(np.uint32).reshape(n, -1) == res).all(), what
        # min_count NULL: the strings in which anything occurred
        run_form(torch, tab, name, True, text, offs, flags, None, False, n, False, dev_batch)[0].check(model_count_select(res, None, False), (name, flags, "NULL"))
    assert (dev_batch[0].cpu().numpy() == text).all() and (dev_batch[1].cpu().numpy().view(np.uint64) == offs).all()
    # the wrapper
    m, all_ = SELECTIONS[name][0]
    exp = model_count_select(oracle_results(name, 3), m, all_)
    w = tab.run_select(text, offs, min_count=m, all=all_) if name in COUNTING else tab.run_half_final_select(text, offs, min_count=m, all=all_)
    assert w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all() and (w["hit_results"] == exp["rows"]).all() and (w["totals"] == exp["totals"]).all()
    assert (w["results"] == oracle_results(name, 3)).all()


@gpu
@pytest.mark.parametrize("variant", (1, 2))
def test_right_behind_a_row_kernels_own_stream_scratch(torch_cuda, variant):
    """pire_hip_config.counting_variant 1 (never the row kernels) and 2 (always, where the table has the image): the pass's
    scratch is taken right behind whatever scratch the scan took on the same stream, the rows in scratch of the library's own"""
    torch = torch_cuda
    text, offs = H.pack(batch())
    text, offs = text.copy(), offs.copy()
    dev_batch = (torch.as_tensor(text, device="cuda"), torch.as_tensor(i64(offs), device="cuda"))
    kernels = set()
    with pb.config(counting_variant=variant):
        for name in ("count_glued3_advanced", "half_5"):
            tab = table_of(name)
            res = oracle_results(name, 3)
            for m, all_ in SELECTIONS[name]:
                exp = model_count_select(res, m, all_)
                for device in (True, False):
                    run_form(torch, tab, name, device, text, offs, 3, m, all_, exp["count"], False, dev_batch)[0].check(exp, (variant, name, m, all_, device))
                    kernels.add(pb.last_kernel())
    print("counting_variant %d: %s" % (variant, sorted(kernels)))
    assert ("counting_rows" in kernels) == (variant == 2), kernels


# ---- GPU: lines ---------------------------------------------------------------------------------------------------------------

def py_lines(raw):
    """getline: the runs between newlines; no extra empty line behind a trailing newline.  (lines, [begin, end) of every line)"""
    parts = bytes(raw).split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    spans, pos = [], 0
    for s in parts:
        spans.append((pos, pos + len(s)))
        pos += len(s) + 1
    return parts, np.array(spans, dtype=np.uint64).reshape(-1, 2)


def lines_form(torch, tab, name, device, raw, flags, m, all_, cap):
    R = tab.RegexpsCount
    out = Outs(torch, device, R, cap, spans=True, lines=True)
    keep = [torch.as_tensor(raw, device="cuda") if device and len(raw) else raw]
    rp = (keep[0].data_ptr() if device else keep[0].ctypes.data) if len(raw) else None
    mp = None
    if m is not None:
        m = np.asarray(m, dtype=np.uint32)
        keep.append(torch.as_tensor(m.view(np.int32), device="cuda") if device else m)
        mp = keep[1].data_ptr() if device else keep[1].ctypes.data
    f = flags | (pb.FLAG_ON_DEVICE if device else 0)
    mode = pb.COUNT_ALL if all_ else 0
    args = (rp, len(raw), 10, f, mp, mode, out.ptr("lines"), out.ptr("totals"), out.ptr("hits"), out.ptr("spans"), out.ptr("rows"), cap, out.ptr("count"),
            torch.cuda.current_stream().cuda_stream or None)
    if name in COUNTING:
        rc = pb.lib().pire_hip_counting_lines_select(tab._h, tab.kind, *args)
    else:
        rc = pb.lib().pire_hip_half_final_lines_select(tab._h, *args)
    assert rc == 0, pb.lib().pire_hip_last_error()
    return out, keep


@gpu
@pytest.mark.parametrize("name", ("count_glued3_advanced", "count_wide17_noglue", "half_0"))
def test_lines_in_counted_lines_out(torch_cuda, name):
    torch = torch_cuda
    tab = table_of(name)
    R = tab.RegexpsCount
    strings = [s for s in batch()[:3000] if s][:2990]
    strings = strings[:100] + [b""] * 3 + strings[100:]                        # consecutive newlines, a last line that is not empty
    assert not any(b"\n" in s for s in strings) and strings[-1]
    joined = b"\n".join(strings)
    for raw in (u8(joined).copy(), u8(joined + b"\n").copy(), u8(b"\n" * 70).copy()):
        parts, spans = py_lines(raw)
        assert len(parts) == (70 if raw[0] == 10 else len(strings))
        for flags in (3, 0):
            res = oracle_results(name, flags, strings=parts)
            for m, all_ in SELECTIONS[name][:2]:
                exp = model_count_select(res, m, all_)
                hit_spans = spans[exp["hits"].astype(np.int64)]
                for device in (True, False):
                    for cap in (len(parts), max(exp["count"] - 1, 0)) if device else (len(parts),):
                        what = (name, len(raw), flags, m, all_, device, cap)
                        out, keep = lines_form(torch, tab, name, device, raw, flags, m, all_, cap)
                        now = out.check(exp, what, spans=hit_spans, lines=len(parts))
                        if not (device and cap == len(parts)):
                            continue
                        # pire_hip_gather_spans chains on out_hit_spans with the device count: the bytes of the counted lines
                        k = exp["count"]
                        want = b"".join(parts[i] + b"\n" for i in exp["hits"].tolist())
                        got_text = torch.full((len(raw) + cap + 64,), POISON, dtype=torch.uint8, device="cuda")
                        got_bytes = torch.zeros(1, dtype=torch.int64, device="cuda")
                        got_offs = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
                        pb.gather_spans_device(keep[0].data_ptr(), len(raw), out.ptr("spans"), got_bytes.data_ptr(), span_count_ptr=out.ptr("count"),
                                               span_cap=cap, tail=10, out_text_ptr=got_text.data_ptr(), text_cap=len(raw) + cap,
                                               out_offsets_ptr=got_offs.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                        assert int(got_bytes.cpu()[0]) == len(want), what
                        assert got_text.cpu().numpy()[:len(want)].tobytes() == want and k == want.count(b"\n"), what
                        ends = np.cumsum([0] + [len(parts[i]) + 1 for i in exp["hits"].tolist()])
                        assert (got_offs.cpu().numpy()[:k + 1] == ends).all(), what
                        assert (keep[0].cpu().numpy() == raw).all(), "the input was written to"
    # the wrapper
    m, all_ = SELECTIONS[name][0]
    raw = u8(joined)
    parts, spans = py_lines(raw)
    exp = model_count_select(oracle_results(name, 3, strings=parts), m, all_)
    w = tab.lines_select_host(raw, min_count=m, all=all_) if name in COUNTING else tab.half_final_lines_select_host(raw, min_count=m, all=all_)
    assert w["lines"] == len(parts) and w["count"] == exp["count"] and (w["hits"] == exp["hits"]).all() and (w["totals"] == exp["totals"]).all()
    assert (w["spans"] == spans[exp["hits"].astype(np.int64)]).all() and (w["hit_results"] == exp["rows"]).all()
