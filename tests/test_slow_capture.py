"""Pire::SlowCapturingScanner on the device: pire_hip_slow_capture_table_*, pire_hip_slow_capture_run, _run_select and
_lines_gather (slow_capture.hip).

Exact equality everywhere.  What is expected comes from tests/golden/slow_capture: the answers of the UNMODIFIED reference
(tests/cpp/slow_capture_golden.cpp, tests/golden/make_slow_capture_inputs.py, which also makes the strings) on every string of every case -- GetCapture()'s
return, final.GetBegin() / GetEnd(), whether `final` was assigned, and the longest state list of the walk.  `Model.walk` restates
the flat walk of DESIGN.md 4.23 over pire_hip_slow_capture_table_image in Python; the CPU part holds it against the reference on
every fixture string (so a wrong table is caught without a GPU), and the GPU part uses it for the one input the fixtures do not
hold (a string of 65 536 bytes).  Lists, spans and gathered bytes are derived from the fixture's numbers with NumPy by the formulas
of include/pire_hip.h.  Every device output sits between poisoned guard bytes and is compared bytewise."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import pire_amd
from pire_amd import binding as pb
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(H.GOLDEN, "slow_capture")
POISON = 0xA5
GUARD = 64
EINVAL, EFORMAT = -1, -2
gpu = pytest.mark.gpu
NAMES = ("pire_hip_slow_capture_table_create", "pire_hip_slow_capture_table_destroy", "pire_hip_slow_capture_table_get_info",
         "pire_hip_slow_capture_table_image", "pire_hip_slow_capture_run", "pire_hip_slow_capture_run_select",
         "pire_hip_slow_capture_lines_gather")


def _driver():
    """tests/golden/make_slow_capture_inputs.py: the strings are made by its case_strings(), here as where the fixtures were written"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_slow_capture_inputs", os.path.join(H.GOLDEN, "make_slow_capture_inputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def cases():
    with open(os.path.join(DIR, "cases.json")) as f:
        doc = json.load(f)
    assert doc["row"] == ["captured", "begin", "end", "matched", "live"]
    return {c["name"]: c for c in doc["cases"]}


CASE_NAMES = ("lazy_pref", "greedy_pref", "or_first", "or_second", "vk", "google_id", "utf8", "lazy_ab_1", "lazy_ab_2", "alt_cd",
              "greedy_alt", "rep_group", "lazy_class", "id", "star", "anchored_lazy", "wide", "wide64", "wide65")


@functools.lru_cache(maxsize=None)
def blob_of(name):
    with open(os.path.join(DIR, cases()[name]["blob"]), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def strings_of(name):
    """The case's strings, made again by the generator's own function and held against the SHA-1 it recorded"""
    c, drv = cases()[name], _driver()
    strings = drv.case_strings(name, c["gap"])
    assert len(strings) == c["strings"] and drv.digest(strings) == c["sha1"], name
    return strings


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """int64[strings][5] of the reference: captured, begin, end, matched, live"""
    c = cases()[name]
    every = np.fromfile(os.path.join(DIR, "expected.i16"), dtype="<i2").reshape(-1, 5)
    return every[c["first"]:c["first"] + c["strings"]].astype(np.int64)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(captured u8, begin i64, end i64, matched u8, live) of the reference, per string"""
    r = rows_of(name)
    return r[:, 0].astype(np.uint8), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].astype(np.uint8), r[:, 4].copy()


@functools.lru_cache(maxsize=None)
def table(name):
    return pire_amd.SlowCaptureTable(blob_of(name))


# ---- the walk of DESIGN.md 4.23, restated over the exported image --------------------------------------------------------------

class Model:
    def __init__(self, t):
        img = t.image()
        self.letters_count = t.info.letters
        self.pos = img["list_pos"].tolist()
        self.entries = img["entries"].tolist()
        self.flags = img["state_flags"].tolist()
        self.letters = img["letters"].tolist()
        self.init = [tuple(int(v) for v in row) for row in img["init"]]
        self.init_match = None if img["init_match"] is None else tuple(int(v) for v in img["init_match"])

    def walk(self, s):
        """(captured, begin, end, matched, live) of one string"""
        pos, entries, flags, L = self.pos, self.entries, self.flags, self.letters_count
        clist, match = list(self.init), self.init_match
        live = len(clist)
        for p, c in enumerate(s, 1):
            letter = self.letters[c]
            used, nlist = set(), []
            for st, b, e in clist:
                stopped = False
                row = st * L + letter
                for k in range(pos[row], pos[row + 1]):
                    en = entries[k]
                    t = en & 0xFFFF
                    if t in used:
                        continue
                    used.add(t)
                    if stopped:
                        continue
                    f = (t, b if b != -1 else (p if en & 0x10000 else -1), e if e != -1 else (p if en & 0x20000 else -1))
                    nlist.append(f)
                    if flags[t] & 1:
                        match, stopped = f, True
            clist = nlist
            live = max(live, len(clist))
        for st, b, e in clist:
            if flags[st] & 1:
                return (1 if b != -1 else (flags[st] >> 1) & 1, b, e, 1, live)
        if match is not None:
            return (1, match[1], match[2], 1, live)
        return (0, -1, -1, 0, live)


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(table(name))


def model_select(offsets, captured, begin, end):
    """include/pire_hip.h, pire_hip_capture_select with no BeginMark, final = captured, need_final = 1: (hits, spans)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    length = offsets[1:] - offsets[:-1]
    sel = (begin >= 0) & (end >= 0) & (captured != 0)
    b = np.clip(begin, 0, length)
    e = np.clip(end, b, length)
    hits = np.flatnonzero(sel)
    return hits.astype(np.uint64), np.stack([offsets[:-1][hits] + b[hits], offsets[:-1][hits] + e[hits]], axis=1).astype(np.uint64)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_and_binding():
    L = pb.lib()
    declared = {a[0] for a in pb.ABI}
    for name in NAMES:
        assert name in declared and hasattr(L, name), name
    assert pire_amd.SlowCaptureTable is pb.SlowCaptureTable and C.sizeof(pb.SlowCaptureInfo) == 48
    with open(os.path.join(ROOT, "include", "pire_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
    assert "#define PIRE_HIP_ABI_VERSION 6" in header.replace("  ", " ") or re.search(r"PIRE_HIP_ABI_VERSION\s+6\b", header)


def test_the_fixtures_hold_every_case_of_the_issue_with_both_kinds_of_strings():
    assert tuple(cases()) == CASE_NAMES
    total = captured = 0
    for name, c in cases().items():
        cap, b, e, m, live = expected(name)
        assert len(strings_of(name)) == cap.size >= 43
        total, captured = total + cap.size, captured + int(cap.sum())
        if c["always"] == "never":      # A|(A): matches, never captures -- the point of the pair
            assert name == "or_second" and not cap.any() and m.any()
        else:
            assert cap.any() and (c["always"] or not cap.all()), name
        assert ((cap == 0) | (m == 1)).all() and ((m == 1) | ((b == -1) & (e == -1))).all(), name
    assert 0.3 < captured / total < 0.7
    wide = strings_of("wide")
    assert wide[0] == b"a" * 150 + b"b" and [len(s) for s in wide[1:202]] == list(range(201))
    assert tuple(int(x[0]) for x in expected("wide")) == (1, 79, 151, 1, 79)
    assert cases()["wide"]["states"] == 368
    assert int(expected("wide64")[4].max()) == 64 == int(expected("wide64")[4][0])
    assert int(expected("wide65")[4].max()) == 65 == int(expected("wide65")[4][0])
    # the pair that motivates the feature
    text = b"pref ala bla pref cla suff dla"
    assert strings_of("lazy_pref")[0] == text == strings_of("greedy_pref")[0]
    assert [int(x[0]) for x in expected("lazy_pref")[:3]] == [1, 0, 26] and [int(x[0]) for x in expected("greedy_pref")[:3]] == [1, 13, 26]
    assert strings_of("or_first")[0] == b"A" == strings_of("or_second")[0]
    assert [int(x[0]) for x in expected("or_first")[:4]] == [1, 0, 1, 1] and [int(x[0]) for x in expected("or_second")[:4]] == [0, -1, -1, 1]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_blob_creates_and_get_info_agrees_with_the_fixture(name):
    t, c = table(name), cases()[name]
    i = t.info
    assert (i.states, i.letters, i.start, i.empty) == (c["states"], c["letters"], c["start"], 0)
    img = t.image()
    assert img["list_pos"][0] == 0 and img["list_pos"][-1] == i.entries == img["entries"].size
    assert (np.diff(img["list_pos"].astype(np.int64)) >= 0).all() and int(np.diff(img["list_pos"].astype(np.int64)).max()) == i.longest_list
    assert ((img["entries"] & 0xFFFF) < i.states).all() and (img["entries"] >> 18 == 0).all()
    assert img["init"].shape == (i.init_len, 3) and (img["state_flags"] < 4).all()
    for k in range(i.states * i.letters):                      # the targets of one list are distinct
        lst = img["entries"][img["list_pos"][k]:img["list_pos"][k + 1]] & 0xFFFF
        assert len(set(lst.tolist())) == lst.size
    assert (img["letters"] < i.letters).all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_walk_over_the_exported_image_equals_the_reference_on_every_fixture_string(name):
    """The four outputs and the longest state list, exactly.  (No symbol on the parent commit; a wrong host DFS fails here.)"""
    m = model(name)
    want = rows_of(name).tolist()
    for k, s in enumerate(strings_of(name)):
        assert list(m.walk(s)) == want[k], (name, k, s)


def test_a_plain_slow_scanner_blob_is_eformat():
    L = pb.lib()
    for case in H.golden()["slow"][:3]:
        blob = H.load_blob(case["blob"])
        pire_amd.SlowTable(blob)                                # (it is a SlowScanner ...)
        h = C.c_void_p()
        assert L.pire_hip_slow_capture_table_create(blob, len(blob), C.byref(h)) == EFORMAT and not h.value
        assert b"plain SlowScanner" in L.pire_hip_last_error()


@pytest.mark.parametrize("name", ["or_first", "id", "wide64"])
def test_truncated_and_damaged_blobs_are_rejected(name):
    L = pb.lib()
    blob = blob_of(name)
    h = C.c_void_p()
    cuts = sorted(set(list(range(0, 80)) + list(range(80, len(blob), max(1, len(blob) // 97))) + [len(blob) - 8, len(blob) - 1]))
    for cut in cuts:
        assert L.pire_hip_slow_capture_table_create(blob[:cut], cut, C.byref(h)) == EFORMAT and not h.value, cut
    assert L.pire_hip_slow_capture_table_create(None, 100, C.byref(h)) == EFORMAT
    assert L.pire_hip_slow_capture_table_create(blob, len(blob), None) == EINVAL
    bad = bytearray(blob)
    bad[16] = 2                                                 # the header's type: a SimpleScanner
    assert L.pire_hip_slow_capture_table_create(bytes(bad), len(bad), C.byref(h)) == EFORMAT
    bad = bytearray(blob)
    bad[40:48] = (1 << 40).to_bytes(8, "little")                # start >= states
    assert L.pire_hip_slow_capture_table_create(bytes(bad), len(bad), C.byref(h)) == EFORMAT
    # a jump target out of range
    i = table(name).info
    at = 56 + 264 * 8 + ((i.states + 7) & ~7) + (i.states * i.letters + 1) * 8
    bad = bytearray(blob)
    bad[at:at + 4] = (i.states).to_bytes(4, "little")
    assert L.pire_hip_slow_capture_table_create(bytes(bad), len(bad), C.byref(h)) == EFORMAT


def test_an_empty_scanner_loads_as_the_slow_scanner_does():
    """SlowScanner::Save() of an empty scanner: header, m, empty = 1.  One state with nowhere to go: no string matches."""
    blob = bytearray(blob_of("or_first")[:56])
    blob[48] = 1
    t = pire_amd.SlowCaptureTable(bytes(blob))
    assert (t.info.states, t.info.letters, t.info.entries, t.info.init_len, t.info.init_matched, t.info.empty) == (1, 1, 0, 0, 0, 1)
    assert Model(t).walk(b"abc") == (0, -1, -1, 0, 0)
    assert pire_amd.SlowTable(bytes(blob)).Empty


def test_every_refusal_happens_before_a_device_is_touched():
    """(on a machine without a device a call that touched one would answer PIRE_HIP_ENODEVICE)"""
    L = pb.lib()
    t = table("id")
    text, offs = H.pack([b"id=1&", b"x"])
    n = 2
    cap, mat = np.full(n, POISON, np.uint8), np.full(n, POISON, np.uint8)
    b, e = np.full(n, -7, np.int64), np.full(n, -7, np.int64)
    hits, spans = np.full(n, 77, np.uint64), np.full(2 * n, 77, np.uint64)
    cnt, lines, total = C.c_uint64(77), C.c_uint64(78), C.c_uint64(79)
    run = lambda tab, o, flags, c=cap, bb=b, ee=e: L.pire_hip_slow_capture_run(tab, text.ctypes.data, o, n, flags, pb._np_ptr(c), pb._np_ptr(bb),
                                                                               pb._np_ptr(ee), mat.ctypes.data, None)
    assert run(None, offs.ctypes.data, 0) == EINVAL and b"pire_hip_slow_capture_run: null table" in L.pire_hip_last_error()
    for flags in (pb.FLAG_BEGIN, pb.FLAG_END, pb.FLAG_BEGIN | pb.FLAG_END, pb.FLAG_BEGIN | pb.FLAG_ON_DEVICE):
        assert run(t._h, offs.ctypes.data, flags) == EINVAL and b"takes both marks itself" in L.pire_hip_last_error()
    assert run(t._h, None, 0) == EINVAL and b"null offsets" in L.pire_hip_last_error()
    assert run(t._h, None, pb.FLAG_ON_DEVICE) == EINVAL
    for missing in ("c", "bb", "ee"):
        assert run(t._h, offs.ctypes.data, 0, **{missing: None}) == EINVAL
        assert run(t._h, offs.ctypes.data, pb.FLAG_ON_DEVICE, **{missing: None}) == EINVAL
    down = np.array([0, 5, 3], dtype=np.uint64)
    assert run(t._h, down.ctypes.data, 0) == EINVAL and b"non-decreasing" in L.pire_hip_last_error()
    far = np.array([0, 1, (1 << 32)], dtype=np.uint64)          # a string of 2^32 - 1 bytes: the lengths are the host's to see
    assert run(t._h, far.ctypes.data, 0) == EINVAL and b"2^32 - 1 bytes" in L.pire_hip_last_error()
    sel = lambda tab, flags, h=hits, s=spans, cap_=n, c=cnt: L.pire_hip_slow_capture_run_select(
        tab, text.ctypes.data, offs.ctypes.data, n, flags, None, None, None, None, pb._np_ptr(h), pb._np_ptr(s), cap_,
        C.byref(c) if c is not None else None, None)
    assert sel(None, 0) == EINVAL and b"pire_hip_slow_capture_run_select: null table" in L.pire_hip_last_error()
    assert sel(t._h, pb.FLAG_BEGIN) == EINVAL
    assert sel(t._h, 0, c=None) == EINVAL and b"pire_hip_slow_capture_run_select" in L.pire_hip_last_error()
    assert sel(t._h, 0, h=None, s=None) == EINVAL
    raw = np.frombuffer(b"id=1&\nx\n", dtype=np.uint8)
    gather = lambda tab, flags, r=raw.ctypes.data, size=raw.size, delim=10, lp=lines, c=cnt: L.pire_hip_slow_capture_lines_gather(
        tab, r, size, delim, flags, 10, C.byref(lp) if lp is not None else None, hits.ctypes.data, spans.ctypes.data, n,
        C.byref(c) if c is not None else None, None, 0, None, None, None)
    assert gather(None, 0) == EINVAL and b"pire_hip_slow_capture_lines_gather: null table" in L.pire_hip_last_error()
    assert gather(t._h, pb.FLAG_END) == EINVAL and b"takes both marks itself" in L.pire_hip_last_error()
    assert gather(t._h, 0, delim=256) == EINVAL
    assert gather(t._h, 0, lp=None) == EINVAL
    assert gather(t._h, 0, c=None) == EINVAL
    assert gather(t._h, 0, r=None) == EINVAL and b"size > 0 with null raw" in L.pire_hip_last_error()
    # a gather output alone is what pire_hip_gather refuses
    assert L.pire_hip_slow_capture_lines_gather(t._h, raw.ctypes.data, raw.size, 10, 0, 10, C.byref(lines), None, None, 0, C.byref(cnt), None, 0,
                                                hits.ctypes.data, None, None) == EINVAL and b"null out_bytes" in L.pire_hip_last_error()
    assert (cap == POISON).all() and (mat == POISON).all() and (b == -7).all() and (e == -7).all()
    assert (hits == 77).all() and (spans == 77).all() and (cnt.value, lines.value, total.value) == (77, 78, 79)
    info = pb.SlowCaptureInfo()
    assert L.pire_hip_slow_capture_table_get_info(None, C.byref(info)) == EINVAL and L.pire_hip_slow_capture_table_get_info(t._h, None) == EINVAL
    small = np.zeros(1, np.uint32)
    img = t.image()
    assert L.pire_hip_slow_capture_table_image(t._h, img["list_pos"].ctypes.data, small.ctypes.data, 1, img["state_flags"].ctypes.data,
                                               img["init"].ctypes.data, np.zeros(3, np.int64).ctypes.data, img["letters"].ctypes.data) == EINVAL
    L.pire_hip_slow_capture_table_destroy(None)


def test_empty_host_calls_answer_zeros_without_a_device():
    t = table("id")
    offs0 = np.zeros(1, dtype=np.uint64)
    cap, b, e, m = t.run(np.zeros(0, np.uint8), offs0)
    assert cap.size == b.size == e.size == m.size == 0
    assert all(a.size == 0 for a in t.run_strings([]))
    got = t.run_select(np.zeros(0, np.uint8), offs0)
    assert got["count"] == 0 and got["hits"].size == 0 and got["spans"].shape == (0, 2)
    cnt = C.c_uint64(77)
    assert pb.lib().pire_hip_slow_capture_run_select(t._h, None, None, 0, 0, None, None, None, None, None, None, 0, C.byref(cnt), None) == 0
    assert cnt.value == 0
    g = t.lines_gather_host(b"")
    assert (g["lines"], g["count"], g["bytes"]) == (0, 0, 0) and g["hits"].size == 0 and g["text"].size == 0 and g["offsets"].tolist() == [0]
    g = t.lines_gather_host(b"", gather=False)
    assert (g["lines"], g["count"]) == (0, 0)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not installed")
def test_the_unit_passes_the_build_audit():
    """slow_capture.hip is a NO_SCRATCH unit of the build's ISA audit, and the Makefile builds and audits it."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "slow_capture.hip" in ba.NO_SCRATCH and "slow_capture.hip" in ba.UNITS and "slow_capture" in ba.__doc__
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert len(re.findall(r"\bslow_capture\.hip\b", mk)) == 2                       # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("slow_capture.hip")
    assert not fails, fails
    assert len(seen) == 1 and "SlowCaptureKernel" in seen[0], seen


def test_the_unit_is_plain_hip_and_the_product_has_no_host_walk():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "slow_capture.hip")) as f:
        src = f.read()
    assert "asm" not in src.replace("__launch_bounds__", "") and "s_waitcnt" not in src and "getenv" not in src
    assert 'kSlowCaptureKernel[] = "slow_capture"' in src and "NoteKernel(kSlowCaptureKernel" in src and "SelfTest" not in src
    assert "slow_capture" not in [k for k in pb.selftested_kernels()]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

class Out:
    """out_captured, out_begin, out_end, out_matched of n strings on the device, each between GUARD poisoned bytes"""

    def __init__(self, torch, n):
        self.n = n
        self.bufs = {k: torch.full((2 * GUARD + max(n, 1) * w,), POISON, dtype=torch.uint8, device="cuda")
                     for k, w in (("captured", 1), ("begin", 8), ("end", 8), ("matched", 1))}
        self.width = {"captured": 1, "begin": 8, "end": 8, "matched": 1}

    def ptr(self, k):
        return self.bufs[k].data_ptr() + GUARD

    def get(self, k):
        a = self.bufs[k].cpu().numpy()
        w = self.width[k]
        assert (a[:GUARD] == POISON).all() and (a[GUARD + self.n * w:] == POISON).all(), "guard bytes of %s" % k
        body = a[GUARD:GUARD + self.n * w]
        return body.copy() if w == 1 else body.copy().view(np.int64)

    def check(self, want, what):
        for k, w in zip(("captured", "begin", "end", "matched"), want):
            got = self.get(k)
            assert got.shape == w.shape and (got == w).all(), (what, k, np.flatnonzero(got != w)[:8].tolist())


def on_device(torch, strings, lead=0):
    """(text tensor, pointer of the first string, offsets tensor): the strings back to back, `lead` poisoned bytes in front"""
    text, offs = H.pack(strings)
    buf = torch.full((lead + text.size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    if text.size:
        buf[lead:lead + text.size] = torch.as_tensor(text.copy(), device="cuda")
    return buf, buf.data_ptr() + lead, torch.as_tensor(offs.astype(np.int64), device="cuda")


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def run_device(torch, t, strings, lead=0):
    buf, ptr, doffs = on_device(torch, strings, lead)
    out = Out(torch, len(strings))
    t.run_device(ptr, doffs.data_ptr(), len(strings), out.ptr("captured"), out.ptr("begin"), out.ptr("end"), out.ptr("matched"), 0,
                 stream_of(torch))
    torch.cuda.synchronize()
    assert pb.last_kernel() == "slow_capture"
    return out


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_case_with_device_pointers_and_with_host_pointers(name):
    import torch

    t, strings, want = table(name), strings_of(name), expected(name)[:4]
    starts = np.cumsum([0] + [len(s) for s in strings[:-1]])
    assert len(set((starts % 16).tolist())) == 16 or name.startswith("wide6")       # strings start at every address mod 16
    for lead in (0, 3):
        run_device(torch, t, strings, lead).check(want, (name, lead))
    got = t.run_strings(strings)
    for g, w, k in zip(got, want, ("captured", "begin", "end", "matched")):
        assert (g == w).all(), (name, "host", k)
    # out_matched is optional
    buf, ptr, doffs = on_device(torch, strings)
    out = Out(torch, len(strings))
    t.run_device(ptr, doffs.data_ptr(), len(strings), out.ptr("captured"), out.ptr("begin"), out.ptr("end"), 0, 0, stream_of(torch))
    torch.cuda.synchronize()
    assert (out.get("captured") == want[0]).all() and (out.get("matched") == POISON).all() or len(strings) == 0


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_batch_sizes_around_the_block_and_more_strings_than_waves(n):
    """The wide case tiled: 24 * 384 bytes a wave leave 8 waves a block and two blocks a CU, so 4 097 strings are more than the
    grid's waves on a device of 256 CUs and the last block is partial."""
    import torch

    strings, want = strings_of("wide"), expected("wide")[:4]
    idx = [(7 * k) % len(strings) for k in range(n)]
    tiled = [strings[i] for i in idx]
    run_device(torch, table("wide"), tiled).check([w[idx] for w in want], n)


@gpu
@pytest.mark.parametrize("name", ["star", "lazy_ab_1"])
def test_zero_length_strings_first_last_and_in_runs(name):
    import torch

    strings, want = strings_of(name), expected(name)[:4]
    empty = strings.index(b"")
    some = [i for i, s in enumerate(strings) if s][:40]
    idx = [empty] + some[:5] + [empty] * 70 + some[5:] + [empty, empty]
    out = run_device(torch, table(name), [strings[i] for i in idx])
    out.check([w[idx] for w in want], name)
    only = run_device(torch, table(name), [b""] * 130)
    only.check([w[[empty] * 130] for w in want], name)


@gpu
@pytest.mark.parametrize("name,longest", [("wide", 79), ("wide64", 64), ("wide65", 65)])
def test_the_state_list_across_the_64_candidate_boundary(name, longest):
    import torch

    strings, want = strings_of(name), expected(name)
    assert int(want[4][0]) == longest == int(want[4].max()) and want[0][0] == 1
    out = run_device(torch, table(name), strings[:1])
    out.check([w[:1] for w in want[:4]], name)
    if name == "wide":
        assert (int(out.get("begin")[0]), int(out.get("end")[0])) == (79, 151)
    full = np.flatnonzero(want[4] == longest)
    run_device(torch, table(name), [strings[i] for i in full] * 3).check([np.tile(w[full], 3) for w in want[:4]], name)


@functools.lru_cache(maxsize=None)
def long_string():
    """65 536 bytes of the `id` case's alphabet without `&`, the one capture at the end"""
    rng = np.random.RandomState(5)
    body = bytes(rng.choice(np.frombuffer(b"id=12", dtype=np.uint8), size=65536 - 8))
    s = body + b"id=1212&"
    assert len(s) == 65536
    return s, model("id").walk(s)


@gpu
def test_one_long_string_among_short_ones():
    import torch

    s, (c, b, e, m, _) = long_string()
    assert (c, m) == (1, 1) and 65500 < b < e < 65536
    strings, want = strings_of("id"), expected("id")[:4]
    batch = strings[:20] + [s] + strings[20:40]
    exp = [np.concatenate([w[:20], np.array([v], dtype=w.dtype), w[20:40]]) for w, v in zip(want, (c, b, e, m))]
    run_device(torch, table("id"), batch).check(exp, "long")
    run_device(torch, table("id"), [s]).check([x[20:21] for x in exp], "alone")


@gpu
def test_a_small_batch_laid_across_byte_2_to_the_32_of_one_buffer():
    """Offsets from the buffer's start: 2^32 lies between two strings, and inside one."""
    import torch

    total = (1 << 32) + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < total + (1 << 28):
        pytest.skip("%.1f GiB of device memory free, the test needs %.1f" % (free / 2 ** 30, total / 2 ** 30 + 0.25))
    big = torch.empty(total, dtype=torch.uint8, device="cuda")
    try:
        for name in ("id", "wide"):
            strings, want = strings_of(name)[:64], [w[:64] for w in expected(name)[:4]]
            text, offs = H.pack(strings)
            for inside in (0, 5):
                k = next(i for i in range(24, 60) if len(strings[i]) > 8 and len(strings[i - 1]) > 0)
                lead = (1 << 32) - int(offs[k]) - inside
                big[lead - GUARD:lead + text.size + GUARD] = POISON
                big[lead:lead + text.size] = torch.as_tensor(text.copy(), device="cuda")
                doffs = torch.as_tensor((offs + np.uint64(lead)).astype(np.int64), device="cuda")
                assert int(offs[k]) + lead == (1 << 32) - inside and int(offs[-1]) + lead > (1 << 32)
                out = Out(torch, len(strings))
                table(name).run_device(big.data_ptr(), doffs.data_ptr(), len(strings), out.ptr("captured"), out.ptr("begin"), out.ptr("end"),
                                       out.ptr("matched"), 0, stream_of(torch))
                torch.cuda.synchronize()
                out.check(want, (name, inside))
    finally:
        del big
        torch.cuda.empty_cache()


def u64_between_guards(torch, count):
    return torch.full((2 * GUARD + max(count, 1) * 8,), POISON, dtype=torch.uint8, device="cuda")


def read_u64(t, count):
    a = t.cpu().numpy()
    assert (a[:GUARD] == POISON).all() and (a[GUARD + count * 8:] == POISON).all()
    return a[GUARD:GUARD + count * 8].copy().view(np.uint64)


@gpu
@pytest.mark.parametrize("name", ["lazy_ab_2", "id", "star", "wide"])
def test_run_select_lists_the_captures_and_their_spans(name):
    import torch

    t, strings = table(name), strings_of(name)
    cap, b, e, m, _ = expected(name)
    text, offs = H.pack(strings)
    hits, spans = model_select(offs, cap, b, e)
    assert hits.size == int(cap.sum())                           # (every capture of the fixtures has both positions)
    n = len(strings)
    # host pointers
    got = t.run_select(text, offs)
    assert got["count"] == hits.size and (got["hits"] == hits).all() and (got["spans"] == spans).all()
    assert (got["captured"] == cap).all() and (got["begin"] == b).all() and (got["end"] == e).all() and (got["matched"] == m).all()
    got = t.run_select(text, offs, positions=False, hit_cap=3)
    assert got["count"] == hits.size and (got["hits"] == hits[:3]).all() and (got["spans"] == spans[:3]).all()
    assert t.run_select(text, offs, positions=False, lists=False)["count"] == hits.size
    # device pointers: the full lists, a cap smaller than the count, and every optional output null
    buf, ptr, doffs = on_device(torch, strings, 5)
    base = buf.data_ptr()
    shifted = torch.as_tensor((offs + np.uint64(5)).astype(np.int64), device="cuda")
    for cap_ in (n, 3, 0):
        out = Out(torch, n)
        dh, ds, dc = u64_between_guards(torch, cap_), u64_between_guards(torch, 2 * cap_), u64_between_guards(torch, 1)
        t.run_select_device(base, shifted.data_ptr(), n, dc.data_ptr() + GUARD,
                            out.ptr("captured") if cap_ == n else 0, out.ptr("begin") if cap_ == n else 0, out.ptr("end") if cap_ == n else 0,
                            out.ptr("matched") if cap_ == n else 0, dh.data_ptr() + GUARD if cap_ else 0, ds.data_ptr() + GUARD if cap_ else 0,
                            cap_, 0, stream_of(torch))
        torch.cuda.synchronize()
        assert int(read_u64(dc, 1)[0]) == hits.size
        k = min(cap_, hits.size)
        gh, gs = read_u64(dh, cap_), read_u64(ds, 2 * cap_)
        assert (gh[:k] == hits[:k]).all() and (gs[:2 * k].reshape(-1, 2) == spans[:k] + np.uint64(5)).all()
        assert (gh[k:].view(np.uint8) == POISON).all() and (gs[2 * k:].view(np.uint8) == POISON).all()   # nothing behind the cap
        if cap_ == n:
            out.check((cap, b, e, m), name)
        else:
            assert all((out.bufs[key].cpu().numpy() == POISON).all() for key in out.bufs)


@gpu
@pytest.mark.parametrize("trailing", [True, False], ids=["trailing delimiter", "no trailing delimiter"])
@pytest.mark.parametrize("name", ["lazy_ab_1", "star", "id"])
def test_lines_gather_is_grep_o_with_lazy_quantifiers(name, trailing):
    import torch

    t = table(name)
    strings = list(strings_of(name))
    cap, b, e, m, _ = expected(name)
    empty = strings.index(b"")
    order = [i for i in range(len(strings)) if strings[i]][:150]
    order = order[:50] + [empty] * 3 + order[50:]               # empty lines in a run; the last line is not empty
    lines = [strings[i] for i in order]
    raw = b"\n".join(lines) + (b"\n" if trailing else b"")
    starts = np.cumsum([0] + [len(s) + 1 for s in lines])
    line_offs = np.stack([starts[:-1], starts[:-1] + [len(s) for s in lines]], axis=1)
    sel = np.flatnonzero((cap[order] != 0) & (b[order] >= 0) & (e[order] >= 0))
    spans = np.stack([line_offs[sel, 0] + b[order][sel], line_offs[sel, 0] + e[order][sel]], axis=1).astype(np.uint64)
    pieces = [raw[int(x):int(y)] for x, y in spans]
    g = t.lines_gather_host(raw)
    assert g["lines"] == len(lines) and g["count"] == sel.size and (g["hits"] == sel.astype(np.uint64)).all() and (g["spans"] == spans).all()
    assert bytes(g["text"]) == b"".join(p + b"\n" for p in pieces) and g["bytes"] == sum(len(p) + 1 for p in pieces)
    assert g["offsets"].tolist() == np.cumsum([0] + [len(p) + 1 for p in pieces]).tolist()
    g = t.lines_gather_host(raw, gather=False, hit_cap=2)
    assert g["count"] == sel.size and (g["hits"] == sel[:2].astype(np.uint64)).all() and (g["spans"] == spans[:2]).all()
    # device pointers, no tail
    draw = torch.as_tensor(np.frombuffer(raw, dtype=np.uint8).copy(), device="cuda")
    cap_ = len(lines)
    dh, ds, dc, dl, db = (u64_between_guards(torch, k) for k in (cap_, 2 * cap_, 1, 1, 1))
    do = u64_between_guards(torch, cap_ + 1)
    dt = torch.full((2 * GUARD + len(raw),), POISON, dtype=torch.uint8, device="cuda")
    t.lines_gather_device(draw.data_ptr(), len(raw), dl.data_ptr() + GUARD, dc.data_ptr() + GUARD, db.data_ptr() + GUARD, 10, None,
                          dh.data_ptr() + GUARD, ds.data_ptr() + GUARD, cap_, dt.data_ptr() + GUARD, len(raw), do.data_ptr() + GUARD, 0,
                          stream_of(torch))
    torch.cuda.synchronize()
    k = sel.size
    assert int(read_u64(dl, 1)[0]) == len(lines) and int(read_u64(dc, 1)[0]) == k and int(read_u64(db, 1)[0]) == sum(len(p) for p in pieces)
    assert (read_u64(dh, cap_)[:k] == sel.astype(np.uint64)).all() and (read_u64(ds, 2 * cap_)[:2 * k].reshape(-1, 2) == spans).all()
    body = dt.cpu().numpy()
    joined = b"".join(pieces)
    assert bytes(body[GUARD:GUARD + len(joined)]) == joined and (body[:GUARD] == POISON).all() and (body[GUARD + len(joined):] == POISON).all()
    assert read_u64(do, cap_ + 1)[:k + 1].tolist() == np.cumsum([0] + [len(p) for p in pieces]).tolist()


@gpu
def test_the_pair_that_motivates_the_feature():
    """.*?(pref.*suff) against .*(pref.*suff), and (A)|A against A|(A) (capture_ut.cpp:274-295): only this scanner tells them apart"""
    import torch

    text = b"pref ala bla pref cla suff dla"
    for name, span in (("lazy_pref", (0, 26)), ("greedy_pref", (13, 26))):
        out = run_device(torch, table(name), [text])
        assert (int(out.get("captured")[0]), int(out.get("begin")[0]), int(out.get("end")[0]), int(out.get("matched")[0])) == (1,) + span + (1,)
        assert text[span[0]:span[1]] == (b"pref ala bla pref cla suff" if name == "lazy_pref" else b"pref cla suff")
    first, second = run_device(torch, table("or_first"), [b"A"]), run_device(torch, table("or_second"), [b"A"])
    assert (int(first.get("captured")[0]), int(first.get("begin")[0]), int(first.get("end")[0]), int(first.get("matched")[0])) == (1, 0, 1, 1)
    assert (int(second.get("captured")[0]), int(second.get("begin")[0]), int(second.get("end")[0]), int(second.get("matched")[0])) == (0, -1, -1, 1)
