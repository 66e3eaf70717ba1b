"""pire_hip_select / pire_hip_run_select: which strings matched which regexps, answered on the device (select.hip).

Exact equality everywhere.  The expected values come from `expected_select`: end states from the oracle (and the reference
library where oracle/_ref is built), masks and Final from the host accessors Table.AcceptedRegexps / Table.Final."""
import ctypes as C
import importlib.util
import os
import time

import numpy as np
import pytest

import pire_amd
from oracle import binding as ob
from pire_amd import binding as pb
from pire_amd import workloads as W
from tests import helpers as H
from tests.conftest import has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE = pb.FLAG_BEGIN | pb.FLAG_END
POISON = 0xDEADBEEFCAFEF00D
gpu = pytest.mark.gpu


# ---- the expectation helper ------------------------------------------------------------------------------------------

def state_records(t, states):
    """{state index: (mask words as a tuple of ints, Final)} from the host accessors."""
    w = max(1, (t.RegexpsCount + 63) // 64)
    out = {}
    for s in states:
        words = [0] * w
        for r in t.AcceptedRegexps(int(s)):
            if r < t.RegexpsCount:
                words[r // 64] |= 1 << (r % 64)
        out[int(s)] = (tuple(words), bool(t.Final(int(s))) and t.RegexpsCount > 0)
    return out


def expected_select(t, idx, want=None):
    """What pire_hip_select must answer for the end states `idx`: masks u64[n, W], hits (ascending indices), the masks of
    the hits, the count.  `want`: None, or an iterable of regexp numbers (numbers >= RegexpsCount are ignored)."""
    idx = np.asarray(idx, dtype=np.uint32)
    w = max(1, (t.RegexpsCount + 63) // 64)
    uniq = np.unique(idx)
    rec = state_records(t, uniq.tolist())
    table = np.zeros((len(uniq), w), dtype=np.uint64)
    fin = np.zeros(len(uniq), dtype=bool)
    for k, s in enumerate(uniq.tolist()):
        table[k] = np.array(rec[s][0], dtype=np.uint64)
        fin[k] = rec[s][1]
    pos = np.searchsorted(uniq, idx)
    masks = table[pos] if len(idx) else np.zeros((0, w), dtype=np.uint64)
    if want is None:
        sel = fin[pos] if len(idx) else np.zeros(0, dtype=bool)
    else:
        wm = np.zeros(w, dtype=np.uint64)
        for r in want:
            if r < t.RegexpsCount:
                wm[r // 64] |= np.uint64(1 << (r % 64))
        sel = ((masks & wm) != 0).any(axis=1)
    hits = np.nonzero(sel)[0].astype(np.uint64)
    return {"masks": masks, "hits": hits, "hit_masks": masks[sel], "count": int(sel.sum())}


def masks_to_lists(masks):
    return [[64 * w + b for w in range(masks.shape[1]) for b in range(64) if (int(row[w]) >> b) & 1] for row in masks]


def check(got, exp, cap=None):
    """A select answer against the helper's, with room for `cap` hits (None: all of them)."""
    assert got["count"] == exp["count"]
    k = exp["count"] if cap is None else min(cap, exp["count"])
    if got.get("masks") is not None:
        assert (got["masks"] == exp["masks"]).all()
    assert len(got["hits"]) == k and (got["hits"] == exp["hits"][:k]).all()
    if got.get("hit_masks") is not None:
        assert (got["hit_masks"] == exp["hit_masks"][:k]).all()


# ---- tables ------------------------------------------------------------------------------------------------------------

def many_patterns():
    """70 short patterns whose glued scanner stays small (whole-string matches: a trie with a few wildcards)."""
    letters = "abcdefghi"
    pats = [a + b for a in letters for b in letters][:45] + [c + "." for c in letters] + ["." + c for c in letters]
    pats += ["..", "...", "a*", "b+", ".?a", "(ab|cd)", "a.?b"]
    assert len(pats) == 70
    return pats


def self_glued(min_regexps=65):
    """A golden table glued with itself until it has more than 64 regexps (no blob: no oracle for it)."""
    case = [c for c in H.all_cases() if c["name"] == "glue_aaa_bbb"][0]
    t = pb.Table(H.load_blob(case["blob"]))
    while t.RegexpsCount < min_regexps:
        t = pb.Table.glue(t, t)
    return t


def wide_mask_table():
    """(table with W >= 2, oracle or None, alphabet, run flags).  The 70 patterns are compiled as they stand (option n: not
    Surround()ed -- the product of 70 surrounded patterns does not fit the reference's glue limit), so their strings are
    walked without the begin and end marks."""
    if ob.ref_available():
        blob = ob.RefScanner.compile(many_patterns(), ["n"] * 70).save()
        return pb.Table(blob), ob.OracleScanner(blob), b"abcdefghij", 0
    return self_glued(), None, b"abc", BE


def end_states(t, o, text, offs, flags=BE):
    """The oracle's end states -- the reference library's too where it is built --, or, for a table that has no blob, those of
    the already pinned Table.run."""
    if o is None:
        return t.run(text, offs, flags=flags)[0]
    idx, fin = o.run(text, offs, flags=flags, threads=4)
    if ob.ref_available():
        ri, rf = ob.RefScanner.load(o.blob).run(text, offs, flags=flags, threads=4)
        assert (ri == idx).all() and (rf == fin).all()
    return idx


def parity_tables():
    out = [(c["name"], c) for c in H.all_cases() + H.big_sets()]
    return out + [("more_than_64_regexps", None)]


def want_values(t):
    r = t.RegexpsCount
    never = 64 * max(1, (r + 63) // 64) - 1 if r % 64 else None   # a bit at or above RegexpsCount: ignored, selects nothing
    vals = [None, [0], list(range(0, r, 3)) + [r - 1] if r else [], list(range(r))]
    if never is not None:
        vals.append([never])
    if r > 64:
        vals.append([r - 1])                                       # a bit of the second word alone
    return vals


# ---- CPU -----------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["pire_hip_table_mask_words", "pire_hip_select", "pire_hip_run_select", "pire_hip_run_select_strided"]


def test_the_library_exports_the_select_entry_points_and_keeps_its_abi_version():
    L = C.CDLL(pire_amd.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert pb.lib().pire_hip_abi_version() == 6 == pb.ABI_VERSION
    assert set(NEW_SYMBOLS) <= {n for n, _, _ in pb.ABI}


def test_mask_words():
    for case in H.all_cases() + H.big_sets():
        t = pb.Table(H.load_blob(case["blob"]))
        assert t.mask_words == max(1, (t.RegexpsCount + 63) // 64) == 1
    assert pb.lib().pire_hip_table_mask_words(None) == 0


def test_a_table_glued_with_itself_stays_on_the_diagonal():
    """The fallback table with more than 64 regexps: every glue doubles the regexps, none adds a state, and state s accepts
    regexp r + k * (regexps of the golden) for every copy k."""
    case = [c for c in H.all_cases() if c["name"] == "glue_aaa_bbb"][0]
    base = pb.Table(H.load_blob(case["blob"]))
    t = self_glued()
    assert t.RegexpsCount == 128 and t.mask_words == 2 and t.Size == base.Size
    strings = H.case_strings(case)
    o = ob.OracleScanner(H.load_blob(case["blob"]))
    for s in o.run_strings(strings)[0].tolist():
        assert sorted(t.AcceptedRegexps(s)) == sorted(r + 2 * k for r in base.AcceptedRegexps(s) for k in range(64))
        assert t.Final(s) == base.Final(s)


def _select_raw(t, idx, n, want, flags, masks, hits, hit_masks, cap, count):
    return pb.lib().pire_hip_select(t, idx, n, want, flags, masks, hits, hit_masks, cap, count, None)


def test_validation_refuses_before_any_device_is_touched():
    t = pb.Table(H.load_blob("c2_single.blob"))
    L = pb.lib()
    idx = np.zeros(4, dtype=np.uint32)
    hits = np.zeros(4, dtype=np.uint64)
    hm = np.zeros(4, dtype=np.uint64)
    cnt = C.c_uint64(77)
    p, c = idx.ctypes.data, C.addressof(cnt)
    cases = {
        "null table": (None, p, 4, None, 0, None, hits.ctypes.data, None, 4, c),
        "null state_idx": (t._h, None, 4, None, 0, None, hits.ctypes.data, None, 4, c),
        "null out_hit_count": (t._h, p, 4, None, 0, None, hits.ctypes.data, None, 4, None),
        "hit_cap > 0 with null out_hits": (t._h, p, 4, None, 0, None, None, None, 4, c),
        "out_hit_masks without out_hits": (t._h, p, 4, None, 0, None, None, hm.ctypes.data, 0, c),
    }
    for text, args in cases.items():
        for flags in (0, pb.FLAG_ON_DEVICE):
            a = list(args)
            a[4] = flags
            assert _select_raw(*a) == -1, text
            assert text in L.pire_hip_last_error().decode(), (text, L.pire_hip_last_error())
    assert cnt.value == 77
    # the same through the fused calls (their state indices are the library's own: no state_idx case)
    for text in ("null table", "null out_hit_count", "hit_cap > 0 with null out_hits", "out_hit_masks without out_hits"):
        th, _, n, want, flags, om, oh, ohm, cap, oc = cases[text]
        offs = np.zeros(5, dtype=np.uint64)
        assert L.pire_hip_run_select(th, None, offs.ctypes.data, n, BE, None, None, None, None, want, om, oh, ohm, cap, oc, None) == -1
        assert text in L.pire_hip_last_error().decode()
        assert L.pire_hip_run_select_strided(th, None, n, 0, 0, BE, None, None, None, None, want, om, oh, ohm, cap, oc, None) == -1
        assert text in L.pire_hip_last_error().decode()
    # host mode: a state index beyond the table, and n == 0 (a count of 0, no device needed)
    bad = np.array([0, t.Size], dtype=np.uint32)
    assert _select_raw(t._h, bad.ctypes.data, 2, None, 0, None, None, None, 0, c) == -1
    assert "out of range" in L.pire_hip_last_error().decode()
    assert _select_raw(t._h, None, 0, None, 0, None, None, None, 0, c) == 0 and cnt.value == 0
    assert t.select(np.zeros(0, dtype=np.uint32))["count"] == 0


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_run_select_without_gpu_fails_loudly():
    t = pb.Table(H.load_blob(H.all_cases()[0]["blob"]))
    text, offs = H.pack([b"abc", b"de"])
    with pytest.raises(pb.PireHipError) as e:
        t.run_select(text, offs)
    assert e.value.code == -3 and "hip" in str(e.value).lower()
    with pytest.raises(pb.PireHipError) as e:
        t.select(np.zeros(3, dtype=np.uint32))
    assert e.value.code == -3


@pytest.mark.parametrize("case", [c for c in H.all_cases() if "ref_expect_accepted" in c], ids=lambda c: c["name"])
def test_expectation_helper_against_the_lists_of_the_references_own_tests(case):
    blob = H.load_blob(case["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    text, offs = H.pack(H.case_strings(case))
    idx = end_states(t, o, text, offs)
    exp = expected_select(t, idx)
    want = [sorted(a) for a in case["ref_expect_accepted"]]
    assert masks_to_lists(exp["masks"]) == want
    assert exp["hits"].tolist() == [i for i, a in enumerate(want) if a] and exp["count"] == sum(1 for a in want if a)
    assert masks_to_lists(exp["hit_masks"]) == [a for a in want if a]
    for r in range(t.RegexpsCount):
        assert expected_select(t, idx, [r])["hits"].tolist() == [i for i, a in enumerate(want) if r in a]
    assert expected_select(t, idx, [t.RegexpsCount + 3])["count"] == 0


def test_the_select_unit_passes_the_build_audit():
    """select.hip is a NO_SCRATCH unit of the build's ISA audit: the classify, scan and scatter kernels compile without scratch."""
    spec = importlib.util.spec_from_file_location("build_audit", os.path.join(ROOT, "tools", "audit", "build_audit.py"))
    ba = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ba)
    assert "select.hip" in ba.NO_SCRATCH and "select.hip" in ba.UNITS
    with open(os.path.join(ROOT, "pire_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert mk.count("select.hip") == 2   # NAMES and AUDIT_UNITS
    fails, seen = ba.audit("select.hip")
    assert not fails, fails
    assert len(seen) == 4 and all("Select" in k for k in seen), seen


def test_the_select_pass_names_no_kernel_of_its_own():
    with open(os.path.join(ROOT, "pire_amd", "csrc", "select.hip")) as f:
        assert "NoteKernel" not in f.read()


# ---- GPU: wrappers -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available() and pire_amd.device_count() > 0, "GPU tests need a HIP device"
    return torch


class DevOut:
    """The device-side outputs of one select call: poisoned, with `guard` words behind out_hits / out_hit_masks."""

    def __init__(self, torch, t, n, cap, masks=True, hits=True, hit_masks=True, guard=8):
        self.torch, self.w, self.n, self.cap, self.guard = torch, t.mask_words, n, cap, guard
        poison = np.uint64(POISON).astype(np.int64)

        def buf(count):
            return torch.full((max(count, 1),), int(poison), dtype=torch.int64, device="cuda")

        self.masks = buf(n * self.w) if masks else None
        self.hits = buf(cap + guard) if hits else None
        self.hit_masks = buf((cap + guard) * self.w) if hit_masks and hits else None
        self.count = buf(1)

    def ptrs(self):
        p = lambda b: 0 if b is None else b.data_ptr()   # noqa: E731
        return dict(out_hit_count_ptr=self.count.data_ptr(), out_masks_ptr=p(self.masks), out_hits_ptr=p(self.hits),
                    out_hit_masks_ptr=p(self.hit_masks), hit_cap=self.cap if self.hits is not None else 0)

    def fetch(self):
        """After a synchronise: the answer as Table.select returns it; the guard words must still be poison."""
        u = lambda b: b.cpu().numpy().view(np.uint64)   # noqa: E731
        count = int(u(self.count)[0])
        k = min(count, self.cap)
        out = {"count": count, "masks": None, "hits": np.zeros(0, np.uint64), "hit_masks": None}
        if self.masks is not None:
            out["masks"] = u(self.masks)[:self.n * self.w].reshape(self.n, self.w)
        if self.hits is not None:
            h = u(self.hits)
            assert (h[k:self.cap + self.guard] == np.uint64(POISON)).all(), "out_hits written behind min(count, hit_cap)"
            out["hits"] = h[:k]
        if self.hit_masks is not None:
            m = u(self.hit_masks)
            assert (m[k * self.w:(self.cap + self.guard) * self.w] == np.uint64(POISON)).all(), "out_hit_masks written behind the hits"
            out["hit_masks"] = m[:k * self.w].reshape(k, self.w)
        return out


def dev_want(torch, t, want):
    m = t.want_mask(want)
    return None if m is None else torch.as_tensor(m.view(np.int64), device="cuda")


def dev_select(torch, t, idx, want=None, cap=None, **kw):
    n = len(idx)
    out = DevOut(torch, t, n, n if cap is None else cap, **kw)
    d = torch.as_tensor(np.asarray(idx, dtype=np.uint32).view(np.int32), device="cuda")
    wm = dev_want(torch, t, want)
    t.select_device(d.data_ptr() if n else 0, n, want_ptr=0 if wm is None else wm.data_ptr(),
                    stream=torch.cuda.current_stream().cuda_stream, **out.ptrs())
    torch.cuda.synchronize()
    return out.fetch()


def dev_run_select(torch, t, text, offs, want=None, cap=None, flags=BE, strided=None, states=True, stream=None, sync=True, **kw):
    """run_select on the device: an offsets batch (text u8, offs u64), or `strided` = a torch [n, len] tensor."""
    n = strided.shape[0] if strided is not None else len(offs) - 1
    out = DevOut(torch, t, n, n if cap is None else cap, **kw)
    idx = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda") if states else None
    fin = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda") if states else None
    wm = dev_want(torch, t, want)
    args = dict(want_ptr=0 if wm is None else wm.data_ptr(), out_idx_ptr=0 if idx is None else idx.data_ptr(),
                out_final_ptr=0 if fin is None else fin.data_ptr(), stream=(stream or torch.cuda.current_stream()).cuda_stream,
                **out.ptrs())
    if strided is not None:
        t.run_select_strided_device(strided.data_ptr(), n, strided.shape[1], strided.stride(0), flags, **args)
    else:
        dt = torch.as_tensor(np.ascontiguousarray(text), device="cuda") if len(text) else torch.zeros(256, dtype=torch.uint8, device="cuda")
        do = torch.as_tensor(np.asarray(offs, dtype=np.uint64).view(np.int64), device="cuda")
        t.run_select_device(dt.data_ptr(), do.data_ptr(), n, flags, **args)
    if not sync:
        return out, idx, fin, wm
    torch.cuda.synchronize()
    got = out.fetch()
    if states:
        got["idx"] = idx.cpu().numpy().view(np.uint32)[:n]
        got["final"] = fin.cpu().numpy()[:n]
    return got


# ---- GPU: parity ---------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,case", parity_tables(), ids=lambda v: v if isinstance(v, str) else "")
def test_parity_on_offset_and_strided_batches(torch_cuda, name, case):
    torch = torch_cuda
    rng = np.random.RandomState(len(name) * 7 + 1)
    flags = BE
    if case is None:
        t, o, alphabet, flags = wide_mask_table()
        assert t.RegexpsCount > 64 and t.mask_words >= 2
        strings = [bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=int(rng.randint(0, 5)))) for _ in range(3000)]
    else:
        blob = H.load_blob(case["blob"])
        t, o = pb.Table(blob), ob.OracleScanner(blob)
        base = H.case_strings(case) if "strings_hex" in case else [bytes.fromhex(h) for h in case["raw"]["strings_hex"]]
        alphabet = b"".join(base) or b"ab"
        strings = base * 8 + H.random_strings(rng, 600, 40, alphabet) + [b""] * 3
        if "witnesses_hex" in case:
            wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]
            strings += [b"xx " + wit[int(rng.randint(len(wit)))] for _ in range(400)] + wit * 3
    order = rng.permutation(len(strings))
    strings = [strings[i] for i in order]
    text, offs = H.pack(strings)
    idx = end_states(t, o, text, offs, flags)
    # fixed-length records of the same alphabet: the tiled path for tables that have dense rows
    n, length = 1024, 256
    a = np.frombuffer(alphabet, np.uint8)
    rec = a[rng.randint(len(a), size=(n, length))].astype(np.uint8)
    for i in range(0, n, 3):                                  # a third of the records end in one of the strings
        s = np.frombuffer(strings[i % len(strings)][:length], np.uint8)
        if len(s):
            rec[i, length - len(s):] = s
    ridx = end_states(t, o, rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, flags)
    drec = torch.as_tensor(rec, device="cuda")
    for want in want_values(t):
        got = dev_run_select(torch, t, text, offs, want, flags=flags)
        assert (got["idx"] == idx).all()
        check(got, expected_select(t, idx, want))
        got = dev_run_select(torch, t, None, None, want, flags=flags, strided=drec)
        if case is not None and "corpus" in case:
            assert pb.last_kernel() == "tiled"
        assert (got["idx"] == ridx).all()
        check(got, expected_select(t, ridx, want))
        check(dev_select(torch, t, idx, want), expected_select(t, idx, want))


# ---- GPU: edges ------------------------------------------------------------------------------------------------------------

def _state_pool(t, o, big):
    """End states of the golden corpus of a big set: final and non-final ones."""
    c = big["corpus"]
    idx = np.asarray(c["idx"], dtype=np.uint32)
    fin = np.asarray(c["final"], dtype=bool)
    return idx, idx[fin], idx[~fin]


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, (1 << 20) + 37])
@pytest.mark.parametrize("table", ["set_a", "inline_glue3"])
def test_edge_sizes(torch_cuda, table, n):
    """set_a (4 552 states: the masks are gathered from memory) and inline_glue3 (92 states: the large batch takes the
    classify kernel that keeps the masks in LDS)."""
    torch = torch_cuda
    case = [c for c in H.all_cases() + H.big_sets() if c["name"] == table][0]
    t = pb.Table(H.load_blob(case["blob"]))
    rng = np.random.RandomState(n % 1000 + 3)
    pool = np.arange(t.Size, dtype=np.uint32) if table != "set_a" else np.unique(np.asarray(case["corpus"]["idx"], dtype=np.uint32))
    idx = pool[rng.randint(len(pool), size=n)] if n else np.zeros(0, dtype=np.uint32)
    for want in (None, [1], [0, 2]):
        exp = expected_select(t, idx, want)
        check(dev_select(torch, t, idx, want), exp)
    if n in (65, 1025, 2049):
        check(t.select(idx, want=[1]), expected_select(t, idx, [1]))   # host pointers


@gpu
def test_all_selected_none_selected_hit_caps_and_null_outputs(torch_cuda):
    torch = torch_cuda
    big = [b for b in H.big_sets() if b["name"] == "set_a"][0]
    t = pb.Table(H.load_blob(big["blob"]))
    _, finals, plain = _state_pool(t, None, big)
    assert len(finals) and len(plain)
    rng = np.random.RandomState(4)
    n = 5000
    every = finals[rng.randint(len(finals), size=n)]
    none = plain[rng.randint(len(plain), size=n)]
    mixed = np.where(rng.rand(n) < 0.3, every, none)
    check(dev_select(torch, t, every), expected_select(t, every))
    assert dev_select(torch, t, every)["count"] == n
    got = dev_select(torch, t, none)
    assert got["count"] == 0 and len(got["hits"]) == 0
    check(got, expected_select(t, none))
    exp = expected_select(t, mixed)
    count = exp["count"]
    assert 2 < count < n
    for cap in (0, count - 1, count, count + 5, n):
        got = dev_select(torch, t, mixed, cap=cap)          # (DevOut.fetch holds the guard words behind min(count, cap))
        assert got["count"] == count
        check(got, exp, cap=cap)
        check(t.select(mixed, hit_cap=cap), exp, cap=cap)     # host pointers
    # every output pointer NULL except the count
    got = dev_select(torch, t, mixed, cap=0, masks=False, hits=False, hit_masks=False)
    assert got["count"] == count
    # hits without their masks, masks without hits
    check(dev_select(torch, t, mixed, hit_masks=False), exp)
    check(dev_select(torch, t, mixed, cap=0, hits=False, hit_masks=False), exp, cap=0)
    # the fused call with every optional output NULL, the state indices in the library's own scratch
    strings = [b"x"] * 300
    text, offs = H.pack(strings)
    oi = ob.OracleScanner(H.load_blob(big["blob"])).run(text, offs)[0]
    got = dev_run_select(torch, t, text, offs, cap=0, states=False, masks=False, hits=False, hit_masks=False)
    assert got["count"] == expected_select(t, oi)["count"]
    # a scanner without regexps selects nothing
    empty = [c for c in H.all_cases() if c["name"] == "empty_scanner"][0]
    te = pb.Table(H.load_blob(empty["blob"]))
    got = dev_run_select(torch, te, *H.pack([b"a", b"", b"abc"]))
    assert got["count"] == 0 and not got["masks"].any()


@gpu
def test_determinism(torch_cuda):
    torch = torch_cuda
    big = [b for b in H.big_sets() if b["name"] == "set_d"][0]
    t = pb.Table(H.load_blob(big["blob"]))
    pool = np.unique(np.asarray(big["corpus"]["idx"], dtype=np.uint32))
    idx = pool[np.random.RandomState(8).randint(len(pool), size=300000)]
    first = dev_select(torch, t, idx, [0, 3, 5])
    check(first, expected_select(t, idx, [0, 3, 5]))
    for _ in range(9):
        again = dev_select(torch, t, idx, [0, 3, 5])
        assert again["hits"].tobytes() == first["hits"].tobytes() and again["count"] == first["count"]


# ---- GPU: every routing ----------------------------------------------------------------------------------------------------

def _set_a(torch, n, length, seed=1234):
    big = [b for b in H.big_sets() if b["name"] == "set_a"][0]
    blob = H.load_blob(big["blob"])
    host = ob.corpus_fill(seed, 0, n, length, H.plants_for(big), threads=4)
    return big, blob, host


@gpu
def test_run_select_behind_every_scan_kernel(torch_cuda, cfg):
    torch = torch_cuda
    n, length = 2048, 1024
    big, blob, host = _set_a(torch, n, length)
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    d = torch.as_tensor(host, device="cuda")
    oi = o.run(host.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)[0]
    exp = expected_select(t, oi, [1, 4])
    assert exp["count"] > 0
    for flags, kernel in ((BE, "tiled"), (BE | pb.FLAG_GENERIC, "generic")):
        got = dev_run_select(torch, t, None, None, [1, 4], flags=flags, strided=d)
        assert pb.last_kernel() == kernel
        assert (got["idx"] == oi).all()
        check(got, exp)
    # ragged strings out of the same bytes: the ragged and the stream kernel
    lens = np.random.RandomState(7).randint(0, 300, size=4000).astype(np.uint64)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    ri = o.run(host.reshape(-1), offs, threads=4)[0]
    for variant, kernel in ((1, "ragged"), (2, "stream")):
        cfg.set(ragged_variant=variant)
        got = dev_run_select(torch, t, host.reshape(-1), offs, None)
        assert pb.last_kernel() == kernel
        assert (got["idx"] == ri).all()
        check(got, expected_select(t, ri))
    cfg.set(ragged_variant=0)
    # four long strings: the segmented scan
    m, long_len = 4, n * length // 4
    li = o.run(host.reshape(-1), np.arange(m + 1, dtype=np.uint64) * long_len, threads=4)[0]
    got = dev_run_select(torch, t, None, None, None, strided=d.reshape(m, long_len))
    assert pb.last_kernel() == "segmented"
    assert (got["idx"] == li).all()
    check(got, expected_select(t, li))
    # a dictionary scanner on the class-indexed walk
    entry = W.wide_set("dict_1k")
    wblob = W.load_blob(entry["blob"])
    wt, wo = pb.Table(wblob), ob.OracleScanner(wblob)
    wn, wlen = 512, 1024
    rec = W.wide_records(entry, "k512", 77, wn, wlen)
    wi = wo.run(rec.reshape(-1), np.arange(wn + 1, dtype=np.uint64) * wlen, threads=4)[0]
    cfg.set(walk_variant=2)
    got = dev_run_select(torch, wt, None, None, None, strided=torch.as_tensor(rec, device="cuda"))
    assert pb.last_kernel() == "wide"
    assert (got["idx"] == wi).all()
    check(got, expected_select(wt, wi))


@gpu
def test_host_pointer_mode_across_staging_chunks(torch_cuda, cfg):
    """More strings than one staging chunk takes (2^22): hit indices are relative to the whole batch, the answer is the
    ON_DEVICE call's."""
    torch = torch_cuda
    case = [c for c in H.all_cases() if c["name"] == "inline_glue3"][0]
    blob = H.load_blob(case["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    base = H.case_strings(case) + [b"", b"zz", b"q"]
    n = (1 << 22) + 1000
    pick = np.random.RandomState(2).randint(len(base), size=n)
    lens = np.array([len(s) for s in base], dtype=np.uint64)[pick]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    flat = np.frombuffer(b"".join(base), np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in base])])[:-1]
    text = np.empty(int(offs[-1]), dtype=np.uint8)
    for k, s in enumerate(base):                           # all strings of one kind at once
        if len(s):
            where = np.nonzero(pick == k)[0]
            pos = offs[where].astype(np.int64)[:, None] + np.arange(len(s))[None, :]
            text[pos] = flat[starts[k]:starts[k] + len(s)][None, :]
    oi = o.run(text, offs, threads=8)[0]
    exp = expected_select(t, oi, [0, 2])
    assert exp["count"] > 1000 and exp["hits"][-1] > (1 << 22)
    host = t.run_select(text, offs, want=[0, 2])
    assert (host["idx"] == oi).all()
    check(host, exp)
    dev = dev_run_select(torch, t, text, offs, [0, 2])
    for k in ("masks", "hits", "hit_masks"):
        assert host[k].tobytes() == dev[k].tobytes(), k
    assert host["count"] == dev["count"]
    # ... and many small chunks, the state indices kept inside the library
    cfg.set(host_chunk_bytes=1 << 16)
    small = t.run_select(text[:int(offs[300000])], offs[:300001], want=[0, 2], states=False)
    check(small, expected_select(t, oi[:300000], [0, 2]))


# ---- GPU: re-ranking ---------------------------------------------------------------------------------------------------------

@gpu
def test_the_answer_survives_an_explicit_adapt(torch_cuda, cfg):
    torch = torch_cuda
    cfg.set(auto_adapt=1, walk_variant=1, prior_flat=1)
    entry = W.wide_set("dict_1k")
    blob = W.load_blob(entry["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    n, length = 8192, 1024
    rec = W.wide_records(entry, "k128", 5, n, length)
    oi = o.run(rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)[0]
    d = torch.as_tensor(rec, device="cuda")
    exp = expected_select(t, oi)
    before = dev_run_select(torch, t, None, None, None, strided=d)
    check(before, exp)
    perm_before = t.layout()[0].copy()
    assert t.adapt() > 0, "the ranking did not change: the test shows nothing"
    assert (t.layout()[0] != perm_before).any()
    after = dev_run_select(torch, t, None, None, None, strided=d)
    check(after, exp)
    for k in ("masks", "hits", "hit_masks"):
        assert before[k].tobytes() == after[k].tobytes(), k


@gpu
def test_the_answer_survives_a_swap_in_the_background(torch_cuda, cfg):
    """The recipe of tests/test_background_adapt.py: enqueue-only calls on an uploaded table until the library has swapped
    in a table it ranked in the background; every answer the same."""
    torch = torch_cuda
    cfg.set(auto_adapt=0, walk_variant=0, zip_variant=0)
    entry = W.wide_set("dict_1k")
    blob = W.load_blob(entry["blob"])
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    n, length = 32768, 1024
    rec = W.wide_records(entry, "k128", 5, n, length)
    oi = o.run(rec.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)[0]
    d = torch.as_tensor(rec, device="cuda")
    exp = expected_select(t, oi)
    t.upload()
    first, adapts = None, 0
    for i in range(12):
        got = dev_run_select(torch, t, None, None, None, strided=d)
        assert (got["idx"] == oi).all(), i
        check(got, exp)
        first = first or got
        assert got["hits"].tobytes() == first["hits"].tobytes() and got["hit_masks"].tobytes() == first["hit_masks"].tobytes()
        adapts = t.refresh_info().adaptations
        if adapts >= 1 and i >= 3:
            break
        time.sleep(0.05)
    assert adapts >= 1, "the table never adapted: the test shows nothing"


# ---- GPU: enqueue-only -------------------------------------------------------------------------------------------------------

@gpu
def test_an_on_device_call_only_enqueues(torch_cuda, cfg):
    """run_select_strided_device on an uploaded table, on a side stream behind a long-running scan: back on the host before
    that scan has finished, right after the synchronise."""
    torch = torch_cuda
    cfg.set(auto_adapt=1)
    n, length = 4096, 1024
    big, blob, host = _set_a(torch, n, length, seed=99)
    t, o = pb.Table(blob), ob.OracleScanner(blob)
    t.upload()
    d = torch.as_tensor(host, device="cuda")
    oi = o.run(host.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)[0]
    exp = expected_select(t, oi, [0, 1, 2])
    check(dev_run_select(torch, t, None, None, [0, 1, 2], strided=d), exp)   # first use: self-test, images, pool warm-up
    # the long-running scan: one string per lane through the generic kernel, 64 strings of 8 MiB
    ln, llen = 64, 8 << 20
    long_text = torch.empty((ln, llen), dtype=torch.uint8, device="cuda")
    pire_amd.corpus_fill_device(long_text.data_ptr(), 5, 0, ln, llen, llen, H.plants_for(big), torch.cuda.current_stream().cuda_stream)
    lidx = torch.empty(ln, dtype=torch.int32, device="cuda")
    # every buffer of the call under test is there before the long scan starts: a copy from pageable memory or a fill
    # enqueued behind that scan would make the TEST wait, whatever the library does
    out = DevOut(torch, t, n, n)
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    wm = dev_want(torch, t, [0, 1, 2])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = torch.cuda.Event()
    t.run_strided_device(long_text.data_ptr(), ln, llen, llen, BE | pb.FLAG_GENERIC, lidx.data_ptr(), 0, 0, 0, side.cuda_stream)
    done.record(side)
    t0 = time.perf_counter()
    t.run_select_strided_device(d.data_ptr(), n, length, length, BE, want_ptr=wm.data_ptr(), out_idx_ptr=idx.data_ptr(),
                                stream=side.cuda_stream, **out.ptrs())
    returned = time.perf_counter() - t0
    still_running = not done.query()
    side.synchronize()
    assert still_running, "the call came back only after the scan in front of it had finished (%.1f ms)" % (returned * 1e3)
    got = out.fetch()
    assert (idx.cpu().numpy().view(np.uint32) == oi).all()
    check(got, exp)


# ---- the C++ shim ------------------------------------------------------------------------------------------------------------
# BatchRunner::Select / Hits / HitMasks / DeviceHits (include/pire_hip/batch_runner.hpp) against the host loop over
# Scanner::Final / AcceptedRegexps, compiled against the UNMODIFIED reference headers (tests/cpp/select_shim_test.cpp)

import subprocess  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "select_shim_test")
REF_PRESENT = os.path.exists("/root/reference/pire/run.h")


@pytest.mark.skipif(not REF_PRESENT, reason="/root/reference not present (GPU box): the prebuilt binary is used there")
def test_select_shim_compiles_against_reference_headers():
    from oracle import binding as ob

    ob.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    assert os.path.exists(BIN) and os.path.exists(os.path.join(os.path.dirname(BIN), "select_host_loop"))


@pytest.mark.gpu
def test_select_shim_matches_the_host_loop_on_gpu():
    if not os.path.exists(BIN):
        pytest.skip("oracle/_ref/bin/select_shim_test was not built (needs the reference tree at build time)")
    r = subprocess.run([BIN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "OK(select shim" in r.stdout
