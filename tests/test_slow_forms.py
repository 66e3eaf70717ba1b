"""Every launch form of the SlowScanner kernels (slow.hip: PlanSlow), each at its boundaries.

The host picks a launch from the automaton's geometry and the batch: tables in LDS or in device memory, blocks of 256,
512 or 1024 threads, 16 waves per block of the wave-per-string kernel or fewer, the 16-slot list kernel in front or
not, one grid-stride pass or several.  pire_hip_slow_table_plan says what a launch will do; the first half of this
file (CPU) recomputes that plan from the constants, written once here, and checks that the fixtures of
tests/golden/slow_forms.json (make_golden_slow_forms.py) between them reach every form.  The second half (gpu) runs the
forms, bit-exact against the oracle: Final, the full state set and the counters."""
import gzip
import hashlib
import json
import os
import re
import struct

import numpy as np
import pytest

from oracle import binding as ob
from tests import helpers as H

B, E = ob.FLAG_BEGIN, ob.FLAG_END
ALL_FLAGS = (B | E, 0, B, E)
CUS = 256                      # an MI355X; the CPU tests plan for it, the GPU tests for the device they run on


def _load():
    with open(os.path.join(H.GOLDEN, "slow_forms.json")) as f:
        return json.load(f)


_J = _load()
FORMS, LANES = _J["slow_forms"], {c["name"]: c for c in _J["slow_lanes"]}
OLD = {c["name"]: c for c in H.golden()["slow"]}
with open(os.path.join(H.GOLDEN, "slow_wide.json")) as _f:
    OLD.update({c["name"]: c for c in json.load(_f)["slow_wide"]})


def case_strings(case):
    if "strings_hex" in case:
        return [bytes.fromhex(h) for h in case["strings_hex"]]
    with open(os.path.join(H.GOLDEN, case["strings_gz"]), "rb") as f:
        text = gzip.decompress(f.read())
    ends = np.cumsum(case["lengths"])
    return [text[int(e) - k:int(e)] for e, k in zip(ends, case["lengths"])]


def sha_rows(bits):
    return [hashlib.sha256(bytes(np.ascontiguousarray(b))).hexdigest() for b in bits]


# ---- SlowScanner::Save() bytes, read here without the library (scanner_io.cpp:71-111) -------------------------------------
class Blob:
    def __init__(self, blob):
        self.states, self.letters, self.start = struct.unpack_from("<QQQ", blob, 24)
        pos = 56
        self.letter_of = np.frombuffer(blob, "<u8", 264, pos).astype(np.int64)
        pos += 264 * 8 + (self.states + 7) // 8 * 8
        npos = self.states * self.letters + 1
        self.jump_pos = np.frombuffer(blob, "<u8", npos, pos).astype(np.int64)
        pos += npos * 8
        self.jumps = np.frombuffer(blob, "<u4", int(self.jump_pos[-1]), pos).astype(np.int64)
        self.words = (self.states + 31) // 32
        self.njumps = len(self.jumps)

    def targets(self, state, letter):
        i = state * self.letters + letter
        out = []
        for t in self.jumps[self.jump_pos[i]:self.jump_pos[i + 1]].tolist():
            if t not in out:
                out.append(t)
        return out

    def list_kernel_gives_up(self, string, flags):
        """SlowListKernel's bookkeeping restated: 16 slots, duplicates kept; a string leaves the list when a step spawns
        twice, meets a row of three targets, or spawns with slot 15 in use."""
        slots = [self.start] + [None] * 15
        chars = ([258] if flags & B else []) + list(string) + ([259] if flags & E else [])
        for ch in chars:
            letter, nxt, spawned = int(self.letter_of[ch]), [], []
            for s in slots:
                t = [] if s is None else self.targets(s, letter)
                if len(t) > 2:
                    return True
                if len(t) == 2:
                    if t[0] == s:          # a self loop is the spawned one
                        t = t[::-1]
                    spawned.append(t[1])
                nxt.append(t[0] if t else None)      # in place; a thread without a target dies where it stands
            if len(spawned) > 1 or (spawned and nxt[15] is not None):
                return True
            slots = spawned + nxt[:15] if spawned else nxt
        return False


# ---- the launch plan, from the constants (slow.hip PlanSlow; internal.h GridBlocks; order.hip OrdersByLength) -------------
LIST_MAX_ROWS = 16383
SINGLE_LDS_MAX, TABLES_LDS_MAX = 64 * 1024, 150 * 1024
SCAN_BIG_BATCH = 128 * 1024
WIDE_LDS_ROOM, WIDE_WAVES = 158 * 1024 - 272, 16
ORDER_FROM = 32768


def grid_blocks(n, cus, threads, lds):
    per_cu = max(1, min(2048 // threads, (160 * 1024) // max(lds, 1)))
    return max(1, min((n + threads - 1) // threads, cus * per_cu))


def passes(n, lanes):
    return (n + lanes - 1) // lanes


def expected_plan(g, njumps, n, ragged, cus, no_list=0, sets_in_memory=0, no_length_order=0):
    states, letters, words = g["states"], g["letters"], g["words"]
    wide = words > 8
    list_table = (states + 1) * letters <= LIST_MAX_ROWS
    walker = "slow_wide" if wide else "slow"
    first = "slow_list" if list_table and n < 2 ** 32 - 1 and not no_list else walker
    p = {"kernel": first, "walker": walker, "k": 0 if wide else 1 if words <= 1 else 2 if words <= 2 else 4 if words <= 4 else 8,
         "list_table": list_table, "single_in_lds": False, "masks_in_lds": False, "waves": 0, "pos_in_lds": False,
         "jumps_in_lds": False, "sets_in_lds": False, "by_length": False, "cus": cus}
    if first == "slow_list":
        p["by_length"] = bool(ragged and ORDER_FROM <= n < 2 ** 32 and not no_length_order)
        lds = 1056 + 16 + (states + 1) * letters * 4
        threads = 1024 if n >= cus * 2048 else 512 if n >= cus * 512 else 256
        blocks = grid_blocks(n, cus, threads, lds)
        lst = {"threads": threads, "blocks": blocks, "lds_bytes": lds, "passes": passes(n, blocks * threads)}
    if not wide:
        mask_bytes, single_bytes = states * letters * p["k"] * 4, (states + 1) * letters * 8
        p["single_in_lds"] = single_bytes <= SINGLE_LDS_MAX
        p["masks_in_lds"] = mask_bytes + (single_bytes if p["single_in_lds"] else 0) <= TABLES_LDS_MAX
        lds = 272 + (single_bytes if p["single_in_lds"] else 0) + (mask_bytes if p["masks_in_lds"] else 0)
        threads = 1024 if n >= SCAN_BIG_BATCH else 256
        blocks = grid_blocks(n, cus, threads, lds)
        walk = {"threads": threads, "blocks": blocks, "lds_bytes": lds, "passes": passes(n, blocks * threads)}
    else:
        set_bytes = words * 8
        waves = min(WIDE_WAVES, WIDE_LDS_ROOM // set_bytes)
        in_lds = waves >= 1 and not sets_in_memory
        if not in_lds:
            waves = WIDE_WAVES
        room = WIDE_LDS_ROOM - (waves * set_bytes if in_lds else 0)
        pos_bytes, jump_bytes = (states * letters + 1) * 4, njumps * 4
        p["pos_in_lds"] = pos_bytes <= room
        if p["pos_in_lds"]:
            room -= pos_bytes
        p["jumps_in_lds"] = p["pos_in_lds"] and jump_bytes <= room
        p["sets_in_lds"], p["waves"] = in_lds, waves
        blocks = max(1, min((n + waves - 1) // waves, cus))
        lds = 272 + (waves * set_bytes if in_lds else 0) + (pos_bytes if p["pos_in_lds"] else 0) + (jump_bytes if p["jumps_in_lds"] else 0)
        walk = {"threads": waves * 64, "blocks": blocks, "lds_bytes": lds, "passes": passes(n, blocks * waves)}
    p["walk"] = walk
    p.update(lst if first == "slow_list" else walk)
    return p


def blob_of(case):
    return H.load_blob(case["blob"])


PLAN_NS = (1, 20000, 131071, 131072, 524288)


@pytest.mark.parametrize("case", list(OLD.values()) + FORMS + list(LANES.values()), ids=lambda c: c["name"])
def test_plan_is_what_the_constants_say(case, cfg):
    """The launches are what they were when the thresholds stood inline in the four launchers: the plan of every golden
    slow case, old and new, recomputed here from geometry and constants, for 256 CUs, offsets and strided batches and
    every knob that the plan reads."""
    import pire_amd

    blob = blob_of(case)
    t, b = pire_amd.SlowTable(blob), Blob(blob)
    g = case["geometry"]
    assert (b.states, b.letters, b.words) == (g["states"], g["letters"], g["words"])
    for knobs in ({}, {"slow_no_list": 1}, {"slow_sets_in_memory": 1}, {"no_length_order": 1}):
        cfg.set(slow_no_list=0, slow_sets_in_memory=0, no_length_order=0)
        cfg.set(**knobs)
        kw = {k[5:] if k.startswith("slow_") else k: v for k, v in knobs.items()}
        for n in PLAN_NS + (0, 32767, 32768, 524289, 2 ** 20, 2 ** 32 - 2, 2 ** 32 - 1):
            for ragged in (True, False):
                want = expected_plan(g, b.njumps, n, ragged, CUS, **kw)
                want["passes"], want["walk"]["passes"] = min(want["passes"], 2 ** 32 - 1), min(want["walk"]["passes"], 2 ** 32 - 1)
                assert t.plan(n, ragged, CUS) == want, (case["name"], knobs, n, ragged)
    assert t.plan(1000, True, 7)["cus"] == 7


def form_of(plan, words):
    """What the issue's table tells apart: the kernel, where its tables live, how many waves, how many rounds of 64 set words."""
    if plan["walker"] == "slow":
        return ("slow", plan["k"], plan["list_table"], plan["single_in_lds"], plan["masks_in_lds"])
    return ("slow_wide", plan["list_table"], plan["sets_in_lds"], plan["pos_in_lds"], plan["jumps_in_lds"], plan["waves"],
            (words + 63) // 64)


# name of the fixture -> the form it is there for
WANT_FORMS = {
    "forms_masks_in_memory": ("slow", 8, True, True, False),
    "forms_tables_in_memory": ("slow", 8, True, False, False),
    "forms_tables_in_memory_no_list": ("slow", 8, False, False, False),
    "forms_x124": ("slow", 8, True, True, True),                     # the last automaton of the bitset kernel
    "forms_x125": ("slow_wide", True, True, True, True, 16, 1),      # the first of the wave-per-string kernel
    "forms_x1020": ("slow_wide", True, True, True, True, 16, 1),     # 64 set words: one round, full
    "forms_x1021": ("slow_wide", True, True, True, True, 16, 2),     # 65: a second round of one word
    "forms_x3000": ("slow_wide", False, True, True, False, 16, 1 + 187 // 64),
    "forms_x21000": ("slow_wide", False, True, False, False, 15, 1 + 1312 // 64),
}


def test_fixtures_reach_every_form(cfg):
    """Should a constant of slow.hip move, a form may lose the fixture that reaches it: then this fails.  Plans at the n
    the GPU test uses (the fixture's own strings, offsets form)."""
    import pire_amd

    cfg.set(slow_no_list=0, slow_sets_in_memory=0, no_length_order=0)
    got, words = {}, {}
    for case in FORMS:
        t = pire_amd.SlowTable(blob_of(case))
        n = len(case.get("lengths") or case["strings_hex"])
        plan = t.plan(n, True, CUS)
        got[case["name"]] = form_of(plan, t.words)
        words[case["name"]] = t.words
        assert plan["kernel"] == ("slow_list" if plan["list_table"] else plan["walker"])
        cfg.set(slow_no_list=1)
        assert t.plan(n, True, CUS)["kernel"] == plan["walker"]
        cfg.set(slow_no_list=0)
    assert got == WANT_FORMS
    assert (words["forms_x124"], words["forms_x125"], words["forms_x1020"], words["forms_x1021"]) == (8, 9, 64, 65)
    # ... and none of them is a form the older golden cases reached already, but the pair that frames a boundary
    old = set()
    for case in OLD.values():
        t = pire_amd.SlowTable(H.load_blob(case["blob"]))
        old.add(form_of(t.plan(len(case["strings_hex"]), True, CUS), t.words))
    new = {v for k, v in got.items() if k not in ("forms_x124", "forms_x125", "forms_x1020")}
    assert not (new & old), new & old
    assert {c["geometry"]["words"] for c in LANES.values()} == {1, 2, 4, 8}


@pytest.mark.parametrize("case", FORMS, ids=lambda c: c["name"])
def test_oracle_reproduces_the_form_fixtures(case):
    blob = blob_of(case)
    assert hashlib.sha256(blob).hexdigest() == case["blob_sha256"]
    o = ob.OracleSlowScanner(blob)
    g = case["geometry"]
    assert (o.size, o.letters, o.words) == (g["states"], g["letters"], g["words"])
    strings = case_strings(case)
    assert strings[:2] == [b"", case["head"][:1].encode()] and len(strings[3]) == 1 + len(case["head"]) + case["gap"]
    fin, bits = o.run_strings(strings)
    assert fin.tolist() == case["final"] and fin[:5].tolist() == [0, 0, 0, 1, 0]
    assert sha_rows(bits) == case["bits_sha256"]


# ---- on the device ------------------------------------------------------------------------------------------------------
PAD = 64          # elements of canary on either side of every output


class Out:
    """Final, state bits and counters of n strings on the device, each between two runs of PAD poisoned elements."""

    def __init__(self, n, words):
        import torch

        self.n, self.words = n, words
        self.fin = torch.full((2 * PAD + n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.bits = torch.full((2 * PAD + n * words,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((2 * PAD + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        self.cnt[PAD:PAD + 2] = 0

    def ptrs(self):
        return self.fin.data_ptr() + PAD, self.bits.data_ptr() + 4 * PAD, self.cnt.data_ptr() + 8 * PAD

    def check(self, want_fin, want_bits, what):
        """Bit-exact results, every string counted once, nothing written outside [0, n)."""
        import torch

        torch.cuda.synchronize()
        fin, bits, cnt = self.fin.cpu().numpy(), self.bits.cpu().numpy().view(np.uint32), self.cnt.cpu().numpy()
        for a, fill in ((fin, 0xA5), (bits, 0xA5A5A5A5), (cnt, 0x5A5A5A5A5A5A5A5A)):
            assert (a[:PAD] == fill).all() and (a[len(a) - PAD:] == fill).all(), ("canary", what)
        got_fin, got_bits = fin[PAD:PAD + self.n], bits[PAD:len(bits) - PAD].reshape(self.n, self.words)
        bad = np.nonzero(got_fin != want_fin)[0]
        assert bad.size == 0, ("final", what, bad[:8])
        bad = np.nonzero((got_bits != want_bits).any(axis=1))[0]
        assert bad.size == 0, ("state bits", what, bad[:8])
        assert cnt[PAD:PAD + 2].tolist() == [int(want_fin.sum()), self.n], ("counts", what)
        return got_fin, got_bits


def run_offsets_device(t, text, offs, flags, ptr_shift=0):
    """The ON_DEVICE offsets form on a fresh poisoned Out; `text` a device tensor, `offs` numpy uint64."""
    import torch

    n = len(offs) - 1
    doffs = torch.as_tensor(np.asarray(offs, dtype=np.uint64).astype(np.int64), device="cuda")
    out = Out(n, t.words)
    t.run_device(text.data_ptr() + ptr_shift, doffs.data_ptr(), n, flags, *out.ptrs(), torch.cuda.current_stream().cuda_stream)
    return out


def run_strings_device(t, strings, flags):
    import torch

    text, offs = H.pack(strings)
    d = torch.as_tensor(np.concatenate([np.asarray(text, dtype=np.uint8), np.zeros(16, np.uint8)]), device="cuda")
    return run_offsets_device(t, d, offs, flags)


def run_strided_device(t, records, length, stride, flags):
    """records: numpy uint8 [n, stride]."""
    import torch

    d = torch.as_tensor(np.ascontiguousarray(records), device="cuda")
    out = Out(records.shape[0], t.words)
    t.run_strided_device(d.data_ptr(), records.shape[0], length, stride, flags, *out.ptrs(), torch.cuda.current_stream().cuda_stream)
    return out


_oracle_cache = {}


def oracle_of(key, blob, strings, flags):
    """The oracle's answer, computed once per (fixture, flags) and shared by the tests that need it."""
    k = (key, flags)
    if k not in _oracle_cache:
        _oracle_cache[k] = ob.OracleSlowScanner(blob).run_strings(strings, flags=flags)
    return _oracle_cache[k]


@pytest.mark.gpu
@pytest.mark.parametrize("no_list", [0, 1], ids=["default", "no_list"])
@pytest.mark.parametrize("case", FORMS, ids=lambda c: c["name"])
def test_form_matrix(case, no_list, cfg):
    """Every fixture through the default path and with pire_hip_config.slow_no_list, from host pointers and in the
    ON_DEVICE offsets form; the kernel that ran is the one the plan names."""
    import pire_amd
    from pire_amd import binding as pb

    blob = blob_of(case)
    t, strings = pire_amd.SlowTable(blob), case_strings(case)
    cfg.set(slow_no_list=no_list)
    plan = t.plan(len(strings), True, 0)
    assert form_of(plan, t.words) == WANT_FORMS[case["name"]]
    assert plan["kernel"] == (plan["walker"] if no_list or not plan["list_table"] else "slow_list")
    for flags in ALL_FLAGS:
        of, obits = oracle_of(case["name"], blob, strings, flags)
        if flags == B | E:
            assert of.tolist() == case["final"] and sha_rows(obits) == case["bits_sha256"]
        gf, gb, cnt = t.run_strings(strings, flags=flags, counts=True)
        assert pb.last_kernel() == plan["kernel"]
        assert (gf == of).all() and (gb == obits).all(), (case["name"], flags, "host")
        assert cnt.tolist() == [int(of.sum()), len(strings)]
        out = run_strings_device(t, strings, flags)
        assert pb.last_kernel() == plan["kernel"]
        out.check(of, obits, (case["name"], flags, "device"))


def popcount_rows(bits):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1).sum(axis=1)


LEFT = re.compile(r"pire_hip slow: (\d+) of (\d+) strings left the list kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("name,gap", [("slow_x300", 300), ("slow_x40_utf8", 40)])
def test_sixteen_slots(name, gap, cfg, capfd):
    """SlowListKernel keeps 16 slots.  A record  y * a + x * k + y * rest  of x.{n}$ has 1 + k states alive at the end of
    its run of x (the start state and one thread per x; checked on the oracle): k <= 15 fits the list, k >= 16 pushes a
    live thread out of slot 15 and the string is handed to the kernel behind (a thread lost there would be missing from
    the state bits of the run without END; END leaves only what it leads on from).  No two threads of x.{n}$ ever merge, so
    the count the list kernel reports (pire_hip_config.slow_stats) is exact: the records whose set outgrew 16 states."""
    import pire_amd
    from pire_amd import binding as pb

    blob = H.load_blob(OLD[name]["blob"])
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    length = min(72, gap)                                # short enough for the first thread to be alive at the end
    stride = length + 3
    shape = [(a, k) for a in (0, 1, 2, 3, 5, 8, 13, 15, 16, 17, 21) for k in range(13, 19)]
    rec = np.full((len(shape), stride), ord("y"), dtype=np.uint8)
    for i, (a, k) in enumerate(shape):
        rec[i, a:a + k] = ord("x")
    rec[:, length:] = ord("x")                           # between the records: must not be read
    sizes = popcount_rows(o.run_strings([b"y" * a + b"x" * k for a, k in shape], flags=0)[1])
    assert sizes.tolist() == [1 + k for _, k in shape]
    left = int((sizes > 16).sum())
    assert left == sum(k >= 16 for _, k in shape) and 0 < left < len(shape)
    strings = [rec[i, :length].tobytes() for i in range(len(shape))]
    cfg.set(slow_stats=1, slow_no_list=0)
    assert t.plan(len(shape), False, 0)["kernel"] == "slow_list"
    for flags in (E, 0):
        of, obits = o.run_strings(strings, flags=flags)
        capfd.readouterr()
        out = run_strided_device(t, rec, length, stride, flags)
        assert pb.last_kernel() == "slow_list"
        out.check(of, obits, (name, flags))
        said = LEFT.findall(capfd.readouterr().err)
        assert said == [(str(left), str(len(shape)))], said


def wave_records(gap, n, rng, length=1024):
    """One record per lane for test_top_inside_one_wave: (records [n, length], lengths for the offsets form)."""
    ks = (list(range(18)) * (n // 18 + 1))[:n]
    rng.shuffle(ks)
    kinds = ([0, 1, 2] * (n // 3 + 1))[:n]
    rng.shuffle(kinds)
    rec = np.full((n, length), ord("y"), dtype=np.uint8)
    lens = np.full(n, length, dtype=np.int64)
    for j in range(n):
        k, a = ks[j], int(rng.randint(1, 48))
        a += 1 if a % 16 == 0 else 0
        if kinds[j] == 1:                      # crowded to the record's end: about k threads alive all the way
            if k:
                rec[j, a::max(1, (gap + 1) // k)] = ord("x")
            continue
        at = a
        while at + 18 < length:                # a run, more than gap + 1 bytes in which every thread dies, the next run
            rec[j, at:at + k] = ord("x")
            at += k + gap + 2 + int(rng.randint(0, 40))
            k = int(rng.randint(1, 18))
        if kinds[j] == 2:                      # a length of its own (offsets form): leaves the 16-byte window loop early
            lens[j] = length - int(rng.randint(17, 300))
    return rec, lens


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 128])
@pytest.mark.parametrize("name,gap", [("slow_x300", 300), ("slow_x40_utf8", 40)])
def test_top_inside_one_wave(name, gap, n, cfg):
    """`top`, the number of groups of four slots a step of the list kernel touches, is one value for the wave.  One
    wave, one wave and a lane, two waves; every lane its own run length (0 .. 17 x) and start (never a multiple of 16).
    In some lanes more than gap + 1 other bytes follow the run: every thread dies inside the window loop, `top` has to
    come down, and a second run has to bring it up again; others stay crowded to the end; a third has a length of its
    own (offsets form, caller's order), so that lanes leave the window loop while others walk on."""
    import pire_amd
    from pire_amd import binding as pb

    blob = H.load_blob(OLD[name]["blob"])
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    rec, lens = wave_records(gap, n, np.random.RandomState(1000 + n))
    whole = [rec[j].tobytes() for j in range(n)]
    cut = [rec[j, :lens[j]].tobytes() for j in range(n)]
    assert len({len(s) % 16 for s in cut}) > 8
    cfg.set(slow_no_list=0, no_length_order=1)
    for flags in ALL_FLAGS:
        of, obits = o.run_strings(whole, flags=flags)
        out = run_strided_device(t, rec, rec.shape[1], rec.shape[1], flags)
        assert pb.last_kernel() == "slow_list"
        out.check(of, obits, (name, n, flags, "strided"))
        of, obits = o.run_strings(cut, flags=flags)
        out = run_strings_device(t, cut, flags)
        assert pb.last_kernel() == "slow_list"
        out.check(of, obits, (name, n, flags, "offsets"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [("forms_x10", 1), ("forms_x20", 2), ("forms_x50", 4), ("forms_x120", 8)])
def test_four_slots(name, k, cfg):
    """A lane of SlowScanKernel keeps four states as a list and more as a bitset of K words.  Runs of 3, 4, 5 and 6 x
    (with the start state: 4 states -- the list holds them -- and 5, 6, 7), more than gap + 1 other bytes in which they
    die, a second run: list -> bitset -> list -> bitset, at every start 0 .. 17, for every K."""
    import pire_amd
    from pire_amd import binding as pb

    case = LANES[name]
    blob, gap = H.load_blob(case["blob"]), case["gap"]
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    cfg.set(slow_no_list=1)
    strings = []
    for a in range(18):
        for r1 in (3, 4, 5, 6):
            for r2 in (3, 4, 5, 6):
                tail = gap - (a + r1 + r2) % (r2 + 2)        # the end falls gap bytes behind one of the second run's x, or does not
                strings.append(b"y" * a + b"x" * r1 + b"y" * (gap + 2) + b"x" * r2 + b"y" * tail)
    plan = t.plan(len(strings), True, 0)
    assert (plan["kernel"], plan["k"]) == ("slow", k)
    sizes = popcount_rows(o.run_strings([b"y" * a + b"x" * r for a in (0, 7) for r in (3, 4, 5, 6)], flags=0)[1])
    assert sizes.tolist() == [4, 5, 6, 7] * 2
    finals = set()
    for flags in ALL_FLAGS:
        of, obits = o.run_strings(strings, flags=flags)
        finals.add(int(of.sum()))
        gf, gb, cnt = t.run_strings(strings, flags=flags, counts=True)
        assert pb.last_kernel() == "slow"
        assert (gf == of).all() and (gb == obits).all(), (name, flags)
        assert cnt.tolist() == [int(of.sum()), len(strings)]
        run_strings_device(t, strings, flags).check(of, obits, (name, flags))
    assert any(0 < f < len(strings) for f in finals)


def every_alignment_and_length(top=48):
    """An order of the 16 * (top + 1) pairs (start mod 16, length) in which every string starts where the one before
    ended: an Euler circuit of the graph  m -> (m + length) mod 16."""
    left = {m: list(range(top, -1, -1)) for m in range(16)}
    stack, walk = [(0, None)], []
    while stack:
        m, via = stack[-1]
        if left[m]:
            k = left[m].pop()
            stack.append(((m + k) % 16, k))
        else:
            stack.pop()
            if via is not None:
                walk.append(via)
    walk.reverse()
    return walk


@pytest.mark.gpu
@pytest.mark.parametrize("no_list", [0, 1], ids=["default", "no_list"])
@pytest.mark.parametrize("name", ["slow_x40_utf8", "slow_x300"])
def test_every_start_alignment_and_length(name, no_list, cfg):
    """The head and tail loops of all three kernels depend on the string's address modulo 16: one string for every
    (address mod 16, length 0 .. 48), 784 in all, inside a device buffer of random bytes (as
    test_poisoned_surroundings.py embeds them).  The oracle's results, the same again when the bytes around the strings
    are redrawn, and not one byte written outside the outputs."""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    blob = H.load_blob(OLD[name]["blob"])
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    lengths = every_alignment_and_length()
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert sorted(zip((starts[:-1] % 16).tolist(), lengths)) == [(m, k) for m in range(16) for k in range(49)]
    rng = np.random.RandomState(77)
    alphabet = np.frombuffer(b"xxxy z\xd0\xb6", dtype=np.uint8)
    text = alphabet[rng.randint(0, len(alphabet), size=int(starts[-1]))]
    strings = [text[starts[i]:starts[i + 1]].tobytes() for i in range(len(lengths))]
    lead, tail = 64, 300
    cfg.set(slow_no_list=no_list)
    kernel = t.plan(len(strings), True, 0)["kernel"]
    assert kernel == ("slow_list" if not no_list else "slow" if t.words <= 8 else "slow_wide")
    crowded = sum(Blob(blob).list_kernel_gives_up(s, 0) for s in strings)
    assert 0 < crowded < len(strings) // 2           # the kernel behind the list kernel gets its share of the alignments
    for flags in ALL_FLAGS:
        of, obits = o.run_strings(strings, flags=flags)
        seen = []
        for redraw in range(2):
            buf = rng.randint(0, 256, size=lead + text.size + tail).astype(np.uint8)
            buf[lead:lead + text.size] = text
            d = torch.as_tensor(buf, device="cuda")
            assert d.data_ptr() % 16 == 0
            out = run_offsets_device(t, d, starts.astype(np.uint64) + np.uint64(lead if redraw else 0), flags,
                                     ptr_shift=0 if redraw else lead)
            assert pb.last_kernel() == kernel
            seen.append(out.check(of, obits, (name, no_list, flags, redraw)))
        assert (seen[0][0] == seen[1][0]).all() and (seen[0][1] == seen[1][1]).all()


BASE = 4099          # distinct strings of a large batch: string i of the batch is base[i % BASE]


def smallest(pred, hi=1 << 22):
    lo = 1
    assert pred(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
    return lo


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["forms_x10", "slow_alt"])
def test_block_sizes_and_passes(name, cfg):
    """Blocks of 256, 512 and 1024 threads and a second, backwards pass: batches at the sizes where the plan (for the
    device's own CUs) changes -- the first n with 512-thread and with 1024-thread blocks of the list kernel, one lane
    and 65 lanes more than one pass holds, three passes where 2^20 strings reach them (on 256 CUs they do not: a pass
    holds 524 288 lanes), the first n with 1024-thread blocks of the bitset kernel -- as offsets in length order,
    offsets in the caller's order, and records of 16 bytes every 19.  String i is base[i % 4099], strings of 0 .. 24
    bytes: the oracle walks the 4 099 base strings once per flag combination (8 ms for all four, measured on the CPU)
    and its answer is tiled.  Every string must be counted exactly once.  One string in a hundred of abc|ad*e holds
    an `a`, whose row of three targets the list cannot take, the base strings that open a second or third pass among
    them: the kernel behind the list kernel has work in every pass.  (x.{10}$ cannot crowd 16 slots: its window of
    11 bytes holds 11 threads.)"""
    import torch
    import pire_amd
    from pire_amd import binding as pb

    blob = H.load_blob((LANES.get(name) or OLD[name])["blob"])
    t, o, model = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob), Blob(blob)
    cfg.set(slow_no_list=0, no_length_order=0)
    assert t.plan(1, True, 0)["kernel"] == "slow_list"
    n512 = smallest(lambda n: t.plan(n, True, 0)["threads"] >= 512)
    n1024 = smallest(lambda n: t.plan(n, True, 0)["threads"] >= 1024)
    top = t.plan(n1024, True, 0)
    lanes = top["blocks"] * top["threads"]
    assert t.plan(lanes, True, 0)["passes"] == 1 and t.plan(lanes + 1, True, 0)["passes"] == 2
    sizes = [n512, n1024, lanes + 1, lanes + 65] + ([2 * lanes + 1] if 2 * lanes + 1 <= 1 << 20 else [])
    cfg.set(slow_no_list=1)
    n_scan = smallest(lambda n: t.plan(n, True, 0)["threads"] >= 1024)
    cfg.set(slow_no_list=0)
    print("CUs", top["cus"], "lanes of a pass", lanes, "list kernel n", sizes, "bitset kernel n", n_scan)
    assert max(sizes + [n_scan]) <= 1 << 21
    assert t.plan(n512 - 1, True, 0)["threads"] == 256 and t.plan(n1024 - 1, True, 0)["threads"] == 512

    rng = np.random.RandomState(4099)
    crowd = {i for i in range(BASE) if i % 97 == 0} | {(p * lanes + d) % BASE for p in (1, 2) for d in (0, 1, 64)}
    quiet = np.frombuffer(b"bcde x" if name == "slow_alt" else b"xxy z", dtype=np.uint8)
    base, have = [], set()
    while len(base) < BASE:
        s = bytearray(quiet[rng.randint(0, len(quiet), size=int(rng.randint(0, 25)))].tobytes())
        if name == "slow_alt" and len(base) in crowd:
            s = bytearray(b"abcde"[i] for i in rng.randint(0, 5, size=int(rng.randint(3, 25))))
            s[int(rng.randint(0, len(s)))] = ord("a")
        if bytes(s) not in have:
            have.add(bytes(s))
            base.append(bytes(s))
    gives_up = [model.list_kernel_gives_up(s, 0) for s in base]
    assert [i for i in range(BASE) if gives_up[i]] == (sorted(crowd) if name == "slow_alt" else [])
    base_text, base_offs = H.pack(base)
    base_lens = np.diff(base_offs.astype(np.int64))
    base_rec = quiet[rng.randint(0, len(quiet), size=(BASE, 19))]
    for i in sorted(crowd):
        base_rec[i, int(rng.randint(0, 16))] = ord("a")
    rec_strings = [base_rec[i, :16].tobytes() for i in range(BASE)]
    want = {}
    for flags in ALL_FLAGS:
        want["ragged", flags] = o.run_strings(base, flags=flags)
        want["strided", flags] = o.run_strings(rec_strings, flags=flags)
    stream = torch.cuda.current_stream().cuda_stream

    def batch(n, form, no_list, no_order):
        cfg.set(slow_no_list=no_list, no_length_order=no_order)
        plan = t.plan(n, form == "ragged", 0)
        idx = np.arange(n) % BASE
        if form == "ragged":
            offs = np.concatenate([[0], np.cumsum(base_lens[idx])]).astype(np.uint64)
            text = np.tile(np.asarray(base_text), n // BASE + 1)[:int(offs[-1]) + 16]
            d = torch.as_tensor(text, device="cuda")
            assert plan["by_length"] == (not no_list and not no_order and n >= 32768)
        else:
            d = torch.as_tensor(base_rec[idx], device="cuda")
        for flags in ALL_FLAGS:
            of, obits = want[form, flags]
            if form == "ragged":
                out = run_offsets_device(t, d, offs, flags)
            else:
                out = Out(n, t.words)
                t.run_strided_device(d.data_ptr(), n, 16, 19, flags, *out.ptrs(), stream)
            assert pb.last_kernel() == plan["kernel"] == ("slow" if no_list else "slow_list")
            out.check(of[idx], obits[idx], (name, n, form, no_list, no_order, flags, plan["threads"], plan["passes"]))
        return plan

    seen = set()
    for n in sizes:
        for form, no_order in (("ragged", 0), ("ragged", 1), ("strided", 0)):
            plan = batch(n, form, 0, no_order)
            seen.add((plan["threads"], min(plan["passes"], 3)))
    assert seen >= {(512, 1), (1024, 1), (1024, 2)}
    for form, no_order in (("ragged", 0), ("ragged", 1), ("strided", 0)):
        assert batch(n_scan, form, 1, no_order)["threads"] == 1024
