"""Tables across re-rankings (table.cpp AdaptTable / BackgroundAdaptStep): what a swap of the host table and its images must leave
as it was.  The suite pins pire_hip_config.auto_adapt = 1 (tests/conftest.py); every test here switches re-ranking back on and
first asserts that the re-ranking it is about really happened (adaptations went up, the image is zipped now, ...), so that none of
them can pass without one.

- the host accessors (final / dead / accepted_regexps / letter_class / next) read the table while it is swapped, and the array
  pire_hip_table_accepted_regexps hands out stays where it was;
- every entry point stays exact before the first swap, right after it and after a swap that zips the image;
- the table's own configuration (pire_hip_table_config_set) rules every ranking path: explicit adapt(), the synchronous automatic
  path, the background worker;
- the entry self-tests follow the table's `selftest` knob, and a re-ranking that zips the image (or gives the plain rows back)
  makes the next call of each kind on the wide walk run its known-answer batch again."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from oracle import binding as ob
from pire_amd import workloads as W
from tests.test_gpu_parity import dev_run_strided, pa, torch_cuda  # noqa: F401  (fixtures)
from tests.test_wide import dev_run_offsets

pytestmark = pytest.mark.gpu

BE = ob.FLAG_BEGIN | ob.FLAG_END
ESELFTEST = -6


class Corpus:
    """A wide scanner, its oracle, fixed-length records (on the device) and the same bytes cut into ragged strings, with every
    expectation the entry points below are compared with."""

    def __init__(self, torch, name, corpus, n=16384, length=1024, seed=5, strings=6000):
        self.entry = W.wide_set(name)
        self.blob = W.load_blob(self.entry["blob"])
        self.o = ob.OracleScanner(self.blob)
        self.data = W.wide_records(self.entry, corpus, seed, n, length)
        self.d = torch.as_tensor(self.data, device="cuda")
        self.oi, self.of = self.o.run(self.data.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)
        rng = np.random.RandomState(seed)
        lens = rng.randint(0, 400, size=strings).astype(np.uint64)
        lens[::53] = 0
        self.offs = np.zeros(strings + 1, dtype=np.uint64)
        self.offs[1:] = np.cumsum(lens)
        self.text = np.ascontiguousarray(self.data.reshape(-1)[:int(self.offs[-1])])
        self.ri, self.rf = self.o.run(self.text, self.offs, threads=4)


def strided(torch, t, c):
    gi, gf, _ = dev_run_strided(torch, t, c.d)
    assert (gi == c.oi).all() and (gf == c.of).all(), "run_strided_device != oracle"


def passes_until(torch, t, c, done, limit, sleep=0.05):
    """Enqueue-only passes (the caller waits for its own stream only) until done(info) or `limit` passes; every answer checked."""
    for _ in range(limit):
        strided(torch, t, c)
        if done(t.refresh_info()):
            return True
        time.sleep(sleep)                 # (the worker re-ranks and uploads on a thread of its own)
    return done(t.refresh_info())


def zipped(info):
    return info.zip_full_states > 0


# ---------------------------------------------------------------------------------------------------------- accessors

def accessor_truth(o, t, states=None):
    """The oracle's final / dead / accepted per state, letter class per byte, Next per state and letter class (one representative
    byte per class: with the classes checked that is Next for every byte); the classes of the marks (chars 256-263, which the
    oracle does not map) as the fresh table reports them.  `states`: the states to know (default: all)."""
    states = range(o.size) if states is None else [int(s) for s in states]
    cls = [o.letter_class(ch) for ch in range(256)] + [t.letter_class(ch) for ch in range(256, 264)]
    reps = {}
    for ch in range(256):
        reps.setdefault(int(cls[ch]), ch)
    reps = sorted(reps.items())
    return {"states": list(states), "final": {s: o.final(s) for s in states}, "dead": {s: o.dead(s) for s in states},
            "accepted": {s: o.accepted(s) for s in states}, "cls": cls, "reps": reps,
            "next": {s: [o.next(s, ch) for _, ch in reps] for s in states}}


def accepted_ptrs(t, states):
    """(address, count) of pire_hip_table_accepted_regexps for every state with a non-empty list -- without dereferencing."""
    from pire_amd import binding as pb

    L = pb.lib()
    out = {}
    for s in states:
        b = C.POINTER(C.c_uint64)()
        n = C.c_size_t()
        assert L.pire_hip_table_accepted_regexps(t._h, s, C.byref(b), C.byref(n)) == 0
        if n.value:
            out[s] = (C.cast(b, C.c_void_p).value, n.value)
    return out


def check_accessors(t, truth, states=None, ptrs=None):
    """Every accessor against the oracle; `ptrs`: the addresses read earlier -- compared BEFORE anything is read through them."""
    states = truth["states"] if states is None else states
    if ptrs is not None:
        now = accepted_ptrs(t, ptrs.keys())
        assert now == ptrs, "pire_hip_table_accepted_regexps moved: the array it handed out earlier was freed"
        for s, (addr, n) in ptrs.items():
            if s in truth["accepted"]:
                assert list(C.cast(addr, C.POINTER(C.c_uint64))[:n]) == truth["accepted"][s], s
    for ch in range(264):
        assert t.letter_class(ch) == truth["cls"][ch], ch
    for s in states:
        assert t.Final(s) == truth["final"][s] and t.Dead(s) == truth["dead"][s], s
        assert t.AcceptedRegexps(s) == truth["accepted"][s], s
        row = truth["next"][s]
        for k, (_, ch) in enumerate(truth["reps"]):
            assert t.Next(s, ch) == row[k], (s, ch)


def test_accessors_survive_background_swaps_and_adapt(pa, torch_cuda, cfg):
    """dict_1k / k128 adapts in the background within a few enqueue-only passes.  The array of accepted regexps of every accepting
    state stays at its address, and every accessor still gives the oracle's answer, after the swap and after an explicit adapt()."""
    torch = torch_cuda
    cfg.set(auto_adapt=0, walk_variant=0, zip_variant=0)
    c = Corpus(torch, "dict_1k", "k128", n=32768)
    t = pa.Table(c.blob)
    truth = accessor_truth(c.o, t)
    ptrs = accepted_ptrs(t, range(c.o.size))
    assert ptrs, "no accepting state: nothing to compare"
    t.upload()
    assert t.refresh_info().adaptations == 0
    assert passes_until(torch, t, c, lambda i: i.adaptations >= 1, 16), "no background swap happened"
    check_accessors(t, truth, ptrs=ptrs)
    other = Corpus(torch, "dict_1k", "k1000", n=8192)   # (text that leaves the new rows: the adapt() below re-ranks)
    before = t.refresh_info().adaptations
    strided(torch, t, other)
    t.adapt()
    assert t.refresh_info().adaptations > before, "adapt() did not re-rank"
    check_accessors(t, truth, ptrs=ptrs)


def test_accessors_race_background_swaps(pa, torch_cuda, cfg):
    """One host thread reads all five accessors in a loop while the main thread's enqueue-only passes make the table swap in
    re-rankings at least twice: every read is the oracle's."""
    torch = torch_cuda
    cfg.set(auto_adapt=0, walk_variant=0, zip_variant=0, auto_adapt_min_traps=8)
    c = Corpus(torch, "dict_10k", "k2048", n=16384)      # (re-ranked again and again: it ends up zipped)
    t = pa.Table(c.blob)
    rng = np.random.RandomState(3)
    known = np.unique(np.concatenate([rng.randint(0, c.o.size, size=3000), np.unique(c.oi)]))
    truth = accessor_truth(c.o, t, known)
    ptrs = accepted_ptrs(t, known)
    t.upload()
    stop, errors, rounds = threading.Event(), [], [0]

    def reader():
        try:
            while not stop.is_set():
                check_accessors(t, truth, states=known[rng.randint(0, len(known), size=400)], ptrs=ptrs)
                rounds[0] += 1
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    th = threading.Thread(target=reader)
    th.start()
    try:
        swapped = passes_until(torch, t, c, lambda i: i.adaptations >= 2, 40)
    finally:
        stop.set()
        th.join()
    assert swapped, ("fewer than two swaps", t.info.adaptations)
    assert not errors, errors
    assert rounds[0] > 0
    check_accessors(t, truth, ptrs=ptrs)


# ------------------------------------------------------------------------------------------------------- entry points

class EntryChecks:
    """Every entry point of one table against its expectation, with device buffers made once."""

    def __init__(self, torch, t, c, other, other_blob):
        from pire_amd import binding as pb

        self.torch, self.t, self.c, self.pb = torch, t, c, pb
        n = len(c.offs) - 1
        self.n = n
        self.dtext = torch.as_tensor(c.text, device="cuda")
        self.doffs = torch.as_tensor(c.offs.astype(np.int64), device="cuda")
        self.want = {}
        for longest in (False, True):
            self.want[("prefix", longest)] = c.o.prefix(c.text, c.offs, longest)
            self.want[("suffix", longest)] = c.o.suffix(c.text, c.offs, longest)
        hi, hf, hr = c.o.run_half_final(c.text, c.offs)
        self.want["half_final"] = (hi, hf, hr.astype(np.uint32))
        self.other, self.other_o = other, ob.OracleScanner(other_blob)
        pi, pf = self.other_o.run(c.text, c.offs, threads=4)
        self.want["pair"] = (c.ri, pi, c.rf | pf)
        m = c.data.shape[0]
        si, sf = self.other_o.run(c.data.reshape(-1), np.arange(m + 1, dtype=np.uint64) * c.data.shape[1], threads=4)
        self.want["pair_strided"] = (c.oi, si, c.of | sf)
        self.states = np.arange(c.o.size, dtype=np.uint32)
        self.want["step"] = np.array([c.o.next(int(s), ord("e")) for s in self.states], dtype=np.uint32)
        self.i64 = torch.empty(n, dtype=torch.int64, device="cuda")

    def sync(self):
        self.torch.cuda.synchronize()

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def all(self, where):
        torch, t, c, pb = self.torch, self.t, self.c, self.pb
        strided(torch, t, c)
        gi, gf, _ = dev_run_offsets(torch, t, c.text, c.offs)
        assert (gi == c.ri).all() and (gf == c.rf).all(), ("run_device", where, pb.last_kernel())
        for longest in (False, True):
            t.prefix_device(self.dtext.data_ptr(), self.doffs.data_ptr(), self.n, longest, self.i64.data_ptr(), stream=self.stream())
            self.sync()
            assert (self.i64.cpu().numpy() == self.want[("prefix", longest)]).all(), ("prefix", longest, where, pb.last_kernel())
            t.suffix_device(self.dtext.data_ptr(), self.doffs.data_ptr(), self.n, longest, self.i64.data_ptr(), stream=self.stream())
            self.sync()
            assert (self.i64.cpu().numpy() == self.want[("suffix", longest)]).all(), ("suffix", longest, where, pb.last_kernel())
        idx = torch.empty(self.n, dtype=torch.int32, device="cuda")
        fin = torch.empty(self.n, dtype=torch.uint8, device="cuda")
        res = torch.zeros((self.n, max(1, t.RegexpsCount)), dtype=torch.int32, device="cuda")
        t.run_half_final_device(self.dtext.data_ptr(), self.doffs.data_ptr(), self.n, BE, idx.data_ptr(), fin.data_ptr(),
                                res.data_ptr(), self.stream())
        self.sync()
        hi, hf, hr = self.want["half_final"]
        assert (idx.cpu().numpy().astype(np.uint32) == hi).all() and (fin.cpu().numpy() == hf).all(), ("half_final", where)
        assert (res.cpu().numpy().astype(np.uint32)[:, :t.RegexpsCount] == hr).all(), ("half_final counts", where)
        i2 = torch.empty(self.n, dtype=torch.int32, device="cuda")
        pb.run_pair_device(t, self.other, self.dtext.data_ptr(), self.doffs.data_ptr(), self.n, BE, idx.data_ptr(), i2.data_ptr(),
                           fin.data_ptr(), self.stream())
        self.sync()
        w1, w2, wf = self.want["pair"]
        assert (idx.cpu().numpy().astype(np.uint32) == w1).all() and (i2.cpu().numpy().astype(np.uint32) == w2).all(), ("pair", where)
        assert (fin.cpu().numpy() == wf).all(), ("pair final", where)
        m, length = c.d.shape
        j1 = torch.empty(m, dtype=torch.int32, device="cuda")
        j2 = torch.empty(m, dtype=torch.int32, device="cuda")
        f2 = torch.empty(m, dtype=torch.uint8, device="cuda")
        pb.run_pair_strided_device(t, self.other, c.d.data_ptr(), m, length, length, BE, j1.data_ptr(), j2.data_ptr(), f2.data_ptr(),
                                   self.stream())
        self.sync()
        w1, w2, wf = self.want["pair_strided"]
        assert (j1.cpu().numpy().astype(np.uint32) == w1).all() and (j2.cpu().numpy().astype(np.uint32) == w2).all(), ("pair_strided", where)
        assert (f2.cpu().numpy() == wf).all(), ("pair_strided final", where)
        st = torch.as_tensor(self.states.astype(np.int32), device="cuda")
        t.step_device(st.data_ptr(), len(self.states), ord("e"), self.stream())
        self.sync()
        assert (st.cpu().numpy().astype(np.uint32) == self.want["step"]).all(), ("step", where)


def test_every_entry_point_stays_exact_across_swaps_that_zip(pa, torch_cuda, cfg):
    """The default policy (auto_adapt = 0): dict_10k / k2048 re-ranks in the background and zips.  Every entry point, interleaved
    (a swap may land at any of their launch boundaries), before the first swap, right after it and after the swap that zips."""
    torch = torch_cuda
    cfg.set(auto_adapt=0, walk_variant=0, zip_variant=0, auto_adapt_min_traps=8)
    c = Corpus(torch, "dict_10k", "k2048", n=16384)
    other_blob = W.load_blob(W.wide_set("dict_1k")["blob"])
    t = pa.Table(c.blob)
    e = EntryChecks(torch, t, c, pa.Table(other_blob), other_blob)
    seen = []
    assert t.refresh_info().adaptations == 0
    e.all("before any swap")
    checked_after_swap = checked_after_zip = False
    for i in range(24):
        info = t.refresh_info()
        adapted, z = info.adaptations >= 1, zipped(info)
        e.all((i, info.adaptations, info.zip_full_states))
        seen.append((info.adaptations, info.zip_full_states))
        checked_after_swap |= adapted
        checked_after_zip |= z
        if checked_after_zip and i >= 2:
            break
        time.sleep(0.05)
    assert checked_after_swap, ("no background swap", seen)
    assert checked_after_zip, ("no swap zipped the table", seen)
    e.all("at the end")


# -------------------------------------------------------------------------------------------- the table's configuration

def rank(torch, t, c, path, rounds):
    """`rounds` re-rankings of the table along `path`; every answer checked on the way."""
    if path == "adapt":
        for _ in range(rounds):
            strided(torch, t, c)
            t.adapt()
    elif path == "sync":                   # auto_adapt = 2, host pointers: the launch boundary drains and re-ranks
        offs = np.arange(c.data.shape[0] + 1, dtype=np.uint64) * c.data.shape[1]
        for _ in range(rounds * 2):
            gi, gf = t.run(c.data.reshape(-1), offs)
            assert (gi == c.oi).all() and (gf == c.of).all()
    else:                                  # auto_adapt = 0, enqueue-only: the background worker
        target = t.refresh_info().adaptations + rounds
        passes_until(torch, t, c, lambda i: i.adaptations >= target, 8 * rounds)


POLICY = {"adapt": 1, "sync": 2, "background": 0}


@pytest.mark.parametrize("path", ["adapt", "sync", "background"])
def test_table_zip_variant_rules_every_ranking_path(pa, torch_cuda, cfg, path):
    """Process zip_variant = 0 (the library zips dict_10k / k2048 after a few measured rankings), table zip_variant = 1: never
    zipped.  Process zip_variant = 1, table zip_variant = 2 and walk_variant = 2: zipped after a measured ranking.  The process
    configuration is what it was."""
    from pire_amd import binding as pb

    torch = torch_cuda
    c = Corpus(torch, "dict_10k", "k2048", n=16384)
    cfg.set(auto_adapt=POLICY[path], walk_variant=0, zip_variant=0, auto_adapt_min_traps=8)
    before = bytes(pb.get_config())
    t = pa.Table(c.blob)
    t.set_config(zip_variant=1)
    rank(torch, t, c, path, 4)
    info = t.refresh_info()
    assert info.adaptations >= 3, (path, info.adaptations)
    assert info.zip_full_states == 0, (path, "zipped against the table's zip_variant = 1", info.zip_full_states)
    strided(torch, t, c)
    assert "zipped" not in pb.last_kernel_symbol(), pb.last_kernel_symbol()
    assert bytes(pb.get_config()) == before

    cfg.set(zip_variant=1)
    before = bytes(pb.get_config())
    t = pa.Table(c.blob)
    t.set_config(zip_variant=2, walk_variant=2)
    assert t.refresh_info().zip_full_states == 0     # the a-priori ranking: the process configuration's (never zip)
    rank(torch, t, c, path, 1)
    info = t.refresh_info()
    assert info.adaptations >= 1, path
    assert info.zip_full_states > 0, (path, "the table's zip_variant = 2 ignored by the ranking")
    strided(torch, t, c)
    assert pb.last_kernel() == "wide" and "zipped" in pb.last_kernel_symbol(), pb.last_kernel_symbol()
    assert bytes(pb.get_config()) == before


def test_table_ragged_variant_survives_a_background_swap(pa, torch_cuda, cfg):
    """Table walk_variant = 2, ragged_variant = 2 under the process defaults: an offsets batch takes stream_wide before and after
    the worker swaps in a new image (the image the worker builds has the stream kernel's tier too)."""
    from pire_amd import binding as pb

    torch = torch_cuda
    cfg.set(auto_adapt=0, auto_adapt_min_traps=8)
    before = bytes(pb.get_config())
    c = Corpus(torch, "dict_10k", "k2048", n=16384)
    t = pa.Table(c.blob)
    t.set_config(walk_variant=2, ragged_variant=2)
    gi, gf, _ = dev_run_offsets(torch, t, c.text, c.offs)
    assert pb.last_kernel() == "stream_wide" and (gi == c.ri).all() and (gf == c.rf).all(), pb.last_kernel()
    assert passes_until(torch, t, c, lambda i: i.adaptations >= 1, 16), "no background swap"
    for _ in range(2):
        gi, gf, _ = dev_run_offsets(torch, t, c.text, c.offs)
        assert (gi == c.ri).all() and (gf == c.rf).all()
        assert pb.last_kernel() == "stream_wide", (pb.last_kernel(), t.refresh_info().adaptations)
    assert bytes(pb.get_config()) == before


# ----------------------------------------------------------------------------------------------------------- self-tests

def entry_calls(pa, torch):
    """(label, call(t) -> None checking its answer) for the entry points with a first-use self-test of their own, and pair."""
    from pire_amd import binding as pb

    blob = W.load_blob(W.wide_set("dict_1k")["blob"])
    o = ob.OracleScanner(blob)
    text = W.wide_records(W.wide_set("dict_1k"), "k128", 9, 512, 256).reshape(-1)
    rng = np.random.RandomState(4)
    lens = rng.randint(0, 200, size=600).astype(np.uint64)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    text = np.ascontiguousarray(text[:int(offs[-1])])
    other = pa.Table(blob)
    oi, of = o.run(text, offs)

    def prefix(t):
        assert (t.prefix(text, offs, True) == o.prefix(text, offs, True)).all()

    def suffix(t):
        assert (t.suffix(text, offs, True) == o.suffix(text, offs, True)).all()

    def half_final(t):
        gi, gf, gr = t.run_half_final(text, offs)
        wi, wf, wr = o.run_half_final(text, offs)
        assert (gi == wi).all() and (gf == wf).all() and (gr == wr).all()

    def pair(t):
        n = len(offs) - 1
        d, doffs = torch.as_tensor(text, device="cuda"), torch.as_tensor(offs.astype(np.int64), device="cuda")
        i1, i2 = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        fin = torch.empty(n, dtype=torch.uint8, device="cuda")
        pb.run_pair_device(t, other, d.data_ptr(), doffs.data_ptr(), n, BE, i1.data_ptr(), i2.data_ptr(), fin.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (i1.cpu().numpy().astype(np.uint32) == oi).all() and (i2.cpu().numpy().astype(np.uint32) == oi).all()
        assert (fin.cpu().numpy() == of).all()

    return blob, [("Prefix", prefix), ("Suffix", suffix), ("HalfFinalScanner", half_final), ("pair", pair)]


def test_entry_self_tests_follow_the_table_selftest_knob(pa, torch_cuda, cfg):
    """Process selftest = 0, table selftest = 2 (one expected answer altered): the first prefix / suffix / half_final / pair call on
    a fresh table is refused with PIRE_HIP_ESELFTEST.  Process selftest = 2, table selftest = 1: they pass and are exact."""
    from pire_amd import binding as pb

    torch = torch_cuda
    blob, calls = entry_calls(pa, torch)
    for label, call in calls:
        cfg.set(selftest=0)
        t = pa.Table(blob)
        t.set_config(selftest=2)
        with pytest.raises(pb.PireHipError) as err:
            call(t)
        assert err.value.code == ESELFTEST and "self-test of " in str(err.value), (label, str(err.value))
        cfg.set(selftest=2)
        t = pa.Table(blob)
        t.set_config(selftest=1)
        call(t)
    cfg.set(selftest=0)


def refused(call, kernel):
    from pire_amd import binding as pb

    with pytest.raises(pb.PireHipError) as err:
        call()
    assert err.value.code == ESELFTEST and kernel in str(err.value), (kernel, str(err.value))


def wide_kinds(torch, t, c, e_prefix, e_half):
    """(kernel name it must report, call checking its answer) for the kinds on the wide walk: wide, the offsets batch on it,
    prefix and HalfFinal with the class-indexed walk's variants."""
    from pire_amd import binding as pb

    def wide():
        strided(torch, t, c)
        assert pb.last_kernel() == "wide"

    def offsets():
        gi, gf, _ = dev_run_offsets(torch, t, c.text, c.offs)
        assert (gi == c.ri).all() and (gf == c.rf).all()
        assert pb.last_kernel() == "ragged_wide", pb.last_kernel()

    def prefix():
        assert (t.prefix(c.text, c.offs, True) == e_prefix).all()

    def half_final():
        gi, gf, gr = t.run_half_final(c.text, c.offs)
        assert (gi == e_half[0]).all() and (gf == e_half[1]).all() and (gr == e_half[2]).all()

    return [("wide kernel", wide, "wide"), ("ragged_wide kernel", offsets, "ragged_wide"), ("Prefix", prefix, "ragged_prefix_wide"),
            ("HalfFinalScanner", half_final, "ragged_half_final_wide")]


def flip_and_retest(torch, t, c, kinds, flip, cfg):
    """Every kind passes on the current layout (its bit set); flip() changes zipped <-> plain; then selftest = 2 refuses the next
    call of each kind, and selftest = 0 lets it pass, exact, with the kernel among the self-tested ones."""
    from pire_amd import binding as pb

    cfg.set(selftest=0)
    for _, call, _ in kinds:
        call()
    was = zipped(t.refresh_info())
    flip()
    assert zipped(t.refresh_info()) != was, ("the layout did not flip", t.info.zip_full_states)
    cfg.set(selftest=2, auto_adapt=1)
    for label, call, _ in kinds:
        refused(call, label)
    cfg.set(selftest=0)
    for _, call, kernel in kinds:
        call()
        assert kernel in pb.selftested_kernels(), (kernel, pb.selftested_kernels())
    strided(torch, t, c)
    assert ("zipped" in pb.last_kernel_symbol()) == (not was), pb.last_kernel_symbol()


@pytest.mark.parametrize("path", ["adapt", "background"])
def test_a_zipping_rerank_runs_the_self_tests_again(pa, torch_cuda, cfg, path):
    """dict_10k / k2048 on the wide walk: wide, ragged_wide / stream_wide, prefix and HalfFinal pass on the plain rows; the table
    is re-ranked until it is zipped (adapt() / a background swap); the next call of each kind runs its known-answer batch again."""
    from pire_amd import binding as pb

    torch = torch_cuda
    cfg.set(walk_variant=2, zip_variant=1, auto_adapt=1, auto_adapt_min_traps=8)   # the plain rows first ...
    c = Corpus(torch, "dict_10k", "k2048", n=16384)
    t = pa.Table(c.blob)
    kinds = wide_kinds(torch, t, c, c.o.prefix(c.text, c.offs, True), c.o.run_half_final(c.text, c.offs))
    assert not zipped(t.refresh_info())

    def flip():
        cfg.set(zip_variant=2)             # ... then the next measured ranking zips
        if path == "adapt":
            for _ in range(6):
                strided(torch, t, c)
                t.adapt()
                if zipped(t.refresh_info()):
                    return
        else:
            # the call at whose launch boundary the zipped table is swapped in is the first wide call on it: refused already
            cfg.set(auto_adapt=0, selftest=2)
            refusals = []
            for _ in range(24):
                try:
                    strided(torch, t, c)
                except pb.PireHipError as err:
                    refusals.append((err.code, str(err)))
                    break
                if zipped(t.refresh_info()):
                    break
                time.sleep(0.05)
            cfg.set(auto_adapt=1, selftest=0)
            assert zipped(t.refresh_info()), "no background swap zipped the table"
            assert refusals and refusals[0][0] == ESELFTEST and "wide kernel" in refusals[0][1], \
                ("the call that swapped the zipped image in ran it without a self-test", refusals)

    flip_and_retest(torch, t, c, kinds, flip, cfg)


def test_going_back_to_the_plain_rows_runs_the_self_tests_again(pa, torch_cuda, cfg):
    """dict_1k: zipped by k1000 (adapt()), the kinds on the wide walk pass on the zipped image; k32 gives the plain rows back
    (adapt()): the next call of each kind runs its known-answer batch again."""
    torch = torch_cuda
    cfg.set(walk_variant=2, zip_variant=0, auto_adapt=1)
    big = Corpus(torch, "dict_1k", "k1000", n=32768)
    small = Corpus(torch, "dict_1k", "k32", n=32768, seed=6)
    t = pa.Table(big.blob)
    for _ in range(6):
        strided(torch, t, big)
        t.adapt()
        if zipped(t.refresh_info()):
            break
    assert zipped(t.info), "k1000 visits 4 000 states: the library zips"
    kinds = wide_kinds(torch, t, small, small.o.prefix(small.text, small.offs, True), small.o.run_half_final(small.text, small.offs))

    def flip():
        for _ in range(10):                 # (the estimates of the old corpus are halved at every adapt())
            strided(torch, t, small)
            t.adapt()
            if not zipped(t.refresh_info()):
                return

    flip_and_retest(torch, t, small, kinds, flip, cfg)
