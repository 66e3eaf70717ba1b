"""The pair kernel (pair.hip, both forms) and the segmented scan's one-mode pass (tiled.hip, ScanTiledSegKernel) where a task
ENDS EARLY: the same ring of two register tiles chained across tasks, the same wave-wide early-out, the same re-prime behind
it and the same hand-counted waits as the kernels of tests/test_kernel_tails.py -- and neither an ISA walk in the build audit
nor a first-use self-test.  No table of tests/test_pair.py is absorbing on BOTH sides and no string of tests/test_segmented.py
ends in an absorbing state, so the early-out of these three kernels was dead code to the suite.  Here: pairs whose two sides
both have an absorbing state with a dense row, records that all reach it in their first tile, absorbed tasks chained to live
ones, tails shorter than a tile, table A's cut row 254, remainders; and segmented scans over text that is absorbed from early
on.  Every expected value is the oracle's (each table alone, Final = either), every string of every launch is compared, and
every test asserts which kernel ran."""
import numpy as np
import pytest

from oracle import binding as ob
from pire_amd import workloads as W
from tests import helpers as H
from tests.test_gpu_parity import pa, torch_cuda  # noqa: F401  (fixtures)
from tests.test_wide import records_of

pytestmark = pytest.mark.gpu
REPS = 300                      # as tests/test_kernel_tails.py: the ragged fault showed once in a few hundred launches
BE = ob.FLAG_BEGIN | ob.FLAG_END
PAIR_HOT_A = 254                # pair.hip kPairHotA: table A keeps device ids 0..253 as dense rows, 254 is its trap id

PAIRS = [("string", "string"), ("string", "dict_1k"), ("dict_1k", "string"), ("dict_1k", "dict_1k"), ("inline_glue3", "string"),
         ("inline_glue3", "dict_1k"), ("string", "same"), ("dict_1k", "same")]   # "same": t1 is t2
PAIR_IDS = ["%s+%s" % p for p in PAIRS]


# ------------------------------------------------------------------------------------------------ host side: tables, witnesses

def _blob(name):
    if name == "dict_1k":
        return W.load_blob(W.wide_set(name)["blob"])
    c = [x for x in H.all_cases() + H.big_sets() if x["name"] == name][0]
    return H.load_blob(c["blob"])


def _begin_state(o):
    """Initialize() + Begin(), as an index."""
    return int(o.run(np.zeros(0, dtype=np.uint8), np.zeros(2, dtype=np.uint64), flags=ob.FLAG_BEGIN)[0][0])


def _is_absorbing(o, s):
    return all(o.next(s, c) == s for c in range(256))


def _path_to(o, start, want):
    """Breadth-first walk over o.next from `start`: the shortest text (one byte per letter class) that ends in a state
    `want` accepts."""
    reps = {}
    for c in list(range(97, 123)) + list(range(32, 97)) + list(range(123, 256)) + list(range(32)):
        reps.setdefault(o.letter_class(c), c)
    prev = {start: None}
    queue = [start]
    for s in queue:
        if want(s):
            out = []
            while prev[s] is not None:
                s, c = prev[s]
                out.append(c)
            return bytes(reversed(out))
        for c in reps.values():
            nx = o.next(s, c)
            if nx not in prev:
                prev[nx] = (s, c)
                queue.append(nx)
    raise AssertionError("no state of the kind wanted is reachable")


_SIDE = {}


def _side(name):
    """(blob, oracle, witness, absorbing state): a text that takes the scanner from Begin() into its Final state all of whose
    transitions are self loops, and that state's index."""
    if name not in _SIDE:
        blob = _blob(name)
        o = ob.OracleScanner(blob)
        if name == "string":
            w = b"abc"
        elif name == "dict_1k":
            w = W.dictionary_words(W.wide_set(name))[11]
        else:
            w = _path_to(o, _begin_state(o), lambda s: o.final(s) and _is_absorbing(o, s))
        s = int(o.run(np.frombuffer(w, dtype=np.uint8), np.array([0, len(w)], dtype=np.uint64), flags=ob.FLAG_BEGIN)[0][0])
        assert o.final(s) and _is_absorbing(o, s), (name, w, s)
        _SIDE[name] = (blob, o, w, s)
    return _SIDE[name]


def _dev_id(t, orig):
    return int(np.nonzero(t.layout()[0] == orig)[0][0])


_FILLER = {}


def _filler(n, length, seed=99):
    """Records without a match of any table here: the dictionary's token stream (a cached base, read-only); a large batch
    repeats 16 384 records, every repeat rotated (workloads.rotated_repeat_order)."""
    key = (n, length, seed)
    if key not in _FILLER:
        if len(_FILLER) > 2:
            _FILLER.clear()
        base = records_of(W.wide_set("dict_1k"), "k128", seed, min(n, 16384), length)
        _FILLER[key] = base if n <= 16384 else base[W.rotated_repeat_order(n, 16384)]
    return _FILLER[key]


def _plant(data, rows, words):
    """The words back to back (a space between) from byte 0 of the rows chosen: inside the first 128-byte tile."""
    w = np.frombuffer(b" ".join(words), dtype=np.uint8)
    assert len(w) <= 128
    data[rows, :len(w)] = w


def _pair_corpus(n1, n2, n, length, in_a, in_b=None, seed=99, late_a=None, late_b=None):
    """data u8[n, length], the oracle's (idx, final) of both sides: side A's witness in the records `in_a`, side B's in `in_b`
    (default: the same records), in their first tile; `late_a` / `late_b`: records with that side's witness at byte 300, behind
    the first pair of tiles -- after the assertions every planted test starts with: exactly the planted records end in the
    absorbing state of the side planted, and are Final."""
    _, o1, w1, s1 = _side(n1)
    _, o2, w2, s2 = _side(n1 if n2 == "same" else n2)
    in_b = in_a if in_b is None else in_b
    if w1 == w2:                                   # one table on both sides: one word, absorbed together
        in_a = in_b = in_a | in_b
    data = _filler(n, length, seed).copy()
    _plant(data, in_a & in_b, [w1] if w1 == w2 else [w1, w2])
    _plant(data, in_a & ~in_b, [w1])
    _plant(data, in_b & ~in_a, [w2])
    for late, w in ((late_a, w1), (late_b, w2)):
        if late is not None:
            assert w1 != w2 and length >= 300 + len(w)
            data[late, 300:300 + len(w)] = np.frombuffer(w, dtype=np.uint8)
    in_a = in_a if late_a is None else in_a | late_a
    in_b = in_b if late_b is None else in_b | late_b
    offs = np.arange(n + 1, dtype=np.uint64) * length
    r1 = o1.run(data.reshape(-1), offs, threads=8)
    r2 = o2.run(data.reshape(-1), offs, threads=8)
    assert (r1[0][in_a] == s1).all() and r1[1][in_a].all() and (r1[0][~in_a] != s1).all(), (n1, n2, "side A")
    assert (r2[0][in_b] == s2).all() and r2[1][in_b].all() and (r2[0][~in_b] != s2).all(), (n1, n2, "side B")
    return data, r1, r2


def _head(r, k):
    return r[0][:k], r[1][:k]


# ------------------------------------------------------------------------------------------------ device side

class _PairRun:
    """pire_hip_run_pair_strided over one resident batch; the outputs are overwritten with junk before every launch."""

    def __init__(self, torch, t1, t2, data, length):
        self.torch, self.t1, self.t2 = torch, t1, t2
        self.n, self.stride = data.shape
        self.length = length
        self.d = torch.as_tensor(data, device="cuda")
        self.i1 = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.i2 = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.fin = torch.empty(self.n, dtype=torch.uint8, device="cuda")

    def __call__(self, flags=BE, n=None, outs=(True, True, True)):
        from pire_amd import binding as pb

        n = self.n if n is None else n
        self.i1.fill_(-2)
        self.i2.fill_(-2)
        self.fin.fill_(9)
        pb.run_pair_strided_device(self.t1, self.t2, self.d.data_ptr(), n, self.length, self.stride, flags,
                                   self.i1.data_ptr() if outs[0] else 0, self.i2.data_ptr() if outs[1] else 0,
                                   self.fin.data_ptr() if outs[2] else 0, self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        return (self.i1[:n].cpu().numpy().astype(np.uint32), self.i2[:n].cpu().numpy().astype(np.uint32),
                self.fin[:n].cpu().numpy())


def _same(got, r1, r2, what=None):
    g1, g2, gf = got
    bad = np.nonzero((g1 != r1[0]) | (g2 != r2[0]) | (gf != (r1[1] | r2[1])))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10].tolist(), (bad[:10] // 64).tolist())


def _pair_tables(pa, n1, n2):
    """The two tables (one, for "same"), each with its absorbing state in a dense row of the pair kernel, side A's below
    kPairHotA: otherwise `done` cannot fire and the early-out is not reached.
    The one exception is pinned as what it is: a table with more states than dense rows on side A.  The ranking puts the Final
    states LAST among the 255 dense rows (table.cpp PermuteByScore: plain, Dead, Final), so dict_1k's only Final state -- the
    absorbing one -- has device id 254 whatever adapt() has measured, which is exactly the row side A gives up.  With dict_1k
    as side A the pair is never absorbed; every record that has matched sits in A's trap id and is walked exactly, chunk by
    chunk, while side B is in its absorbing row: that (and not the early-out) is what those pairs check."""
    def make(name, side_a):
        blob, o, w, s = _side(name)
        t = pa.Table(blob)
        if side_a and t.info.states > t.info.hot_states:
            assert name == "dict_1k" and t.info.hot_states == PAIR_HOT_A + 1 and _dev_id(t, s) == PAIR_HOT_A
        else:
            assert _dev_id(t, s) < min(PAIR_HOT_A if side_a else 256, t.info.hot_states), (name, _dev_id(t, s))
        return t

    if n2 == "same":
        t = make(n1, True)
        return t, t
    return make(n1, True), make(n2, False)


# ------------------------------------------------------------------------------------------------ A. the fused pair

@pytest.mark.parametrize("n1,n2", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("n,length", [(64 * 40, 256), (64 * 40 + 17, 4096), (1 << 15, 512)])
def test_pair_where_every_record_is_absorbed_at_once(pa, torch_cuda, cfg, n1, n2, n, length):
    """Both witnesses in the first tile of EVERY record: every task of the fused kernel ends by the wave-wide early-out with
    its next tile requested (256-byte records: at the last pair of tiles, where there is no early-out)."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    data, r1, r2 = _pair_corpus(n1, n2, n, length, np.ones(n, dtype=bool))
    run = _PairRun(torch_cuda, t1, t2, data, length)
    _same(run(n=n & ~63), _head(r1, n & ~63), _head(r2, n & ~63))   # the whole tasks alone: the fused pass and nothing else
    assert pb.last_kernel() == "pair_tiled" and pb.last_kernel_symbol() == "pirehip::ScanPairTiledKernel"
    for r in range(REPS):
        _same(run(), r1, r2, r)
    # (a remainder: two ordinary passes over the last n % 64 records behind the fused one -- too few for a tiled pass)
    assert pb.last_kernel() == ("pair_tiled" if n % 64 == 0 else "generic")


def _chained_shape(torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # two tasks (of 64 records) for every wave slot of the chip and a few more; a wave's next task is cus * 16 tasks on:
    # not a multiple of 3, or the pattern below would chain absorbed tasks to absorbed ones only
    assert (cus * 16) % 3 != 0
    return 2 * cus * 16 * 64 + 64 * 37, 512


@pytest.mark.parametrize("n1,n2", PAIRS, ids=PAIR_IDS)
def test_pair_early_out_between_chained_tasks(pa, torch_cuda, cfg, n1, n2):
    """Two tasks out of three absorbed in their first tile, several tasks per wave: an absorbed task is followed by a live one
    through the chain tile, a live one by an absorbed one, an absorbed one by an absorbed one whose first tile must be ITS
    OWN (the re-prime behind an early-out)."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    n, length = _chained_shape(torch_cuda)
    planted = ((np.arange(n) // 64) % 3) != 0
    data, r1, r2 = _pair_corpus(n1, n2, n, length, planted, seed=12345)
    run = _PairRun(torch_cuda, t1, t2, data, length)
    for r in range(3):
        _same(run(), r1, r2, r)
        assert pb.last_kernel() == "pair_tiled"


@pytest.mark.parametrize("sides", ["a", "b"], ids=["only side A absorbed", "only side B absorbed"])
@pytest.mark.parametrize("n1,n2", [("string", "dict_1k"), ("dict_1k", "string"), ("inline_glue3", "string")],
                         ids=["string+dict_1k", "dict_1k+string", "inline_glue3+string"])
def test_pair_is_not_absorbed_while_one_side_is_live(pa, torch_cuda, cfg, n1, n2, sides):
    """The same batch with ONE side's witness in the first tile: that side sits in its absorbing row from there on, the pair
    does not.  In every other task the live side's own witness follows at byte 300: a kernel that left on one side's word
    never sees it and returns that side not Final (End() takes every state without a match to the same one, so the state
    of byte 256 for that of byte 512 alone would not show)."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    n, length = _chained_shape(torch_cuda)
    planted = ((np.arange(n) // 64) % 3) != 0
    none = np.zeros(n, dtype=bool)
    late = planted & ((np.arange(n) // 64) % 2 == 0)
    data, r1, r2 = _pair_corpus(n1, n2, n, length, planted if sides == "a" else none, planted if sides == "b" else none, seed=12345,
                                late_a=late if sides == "b" else None, late_b=late if sides == "a" else None)
    run = _PairRun(torch_cuda, t1, t2, data, length)
    for r in range(3):
        _same(run(), r1, r2, r)
        assert pb.last_kernel() == "pair_tiled"


@pytest.mark.parametrize("n1,n2", PAIRS, ids=PAIR_IDS)
def test_pair_with_63_lanes_of_64_in_the_absorbing_rows(pa, torch_cuda, cfg, n1, n2):
    """No wave may leave early: one record of every 64 is live, and it is a different lane from task to task."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    n, length = 64 * 1024, 512
    i = np.arange(n)
    planted = (i % 64) != ((i // 64) * 7) % 64
    data, r1, r2 = _pair_corpus(n1, n2, n, length, planted, seed=5)
    run = _PairRun(torch_cuda, t1, t2, data, length)
    for r in range(20):
        _same(run(), r1, r2, r)
        assert pb.last_kernel() == "pair_tiled"


@pytest.mark.parametrize("n1,n2", [("string", "dict_1k"), ("dict_1k", "string"), ("inline_glue3", "string"), ("dict_1k", "same")],
                         ids=["string+dict_1k", "dict_1k+string", "inline_glue3+string", "dict_1k+same"])
@pytest.mark.parametrize("length", [256 + 1, 300, 256 + 127, 1024 + 100])
def test_pair_tails_shorter_than_a_tile(pa, torch_cuda, cfg, n1, n2, length):
    """PairTiledEligible takes any len >= 256 with an even number of whole 128-byte tiles; what is left of a record behind
    them is walked byte by byte from memory (the kernel's tail loop) -- the header used to say "len a multiple of 256", the
    code is what is meant, and this pins it: such a batch takes the fused kernel, and ends where the record ends.  Behind
    `len`, up to the stride (len rounded up to 16, and 64 more for them): 0xFF and then both witnesses, which no walk may
    reach.  The witnesses also end with the record in every third task (only the byte-wise loop sees their last bytes) and
    sit in the first tile of every other third (the early-out skips the tail)."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    _, o1, w1, s1 = _side(n1)
    _, o2, w2, s2 = _side(n1 if n2 == "same" else n2)
    stride = (length + 15) // 16 * 16 + 64
    n = 64 * 48
    data = np.full((n, stride), 0xFF, dtype=np.uint8)
    data[:, :length] = _filler(n, length, 3)
    both = np.frombuffer(w1 + b" " + w2, dtype=np.uint8)
    data[:, length + 4:length + 4 + len(both)] = both              # poison: beyond the record
    task = np.arange(n) // 64
    head = task % 3 == 1
    data[head, :len(both)] = both
    data[task % 3 == 2, length - len(both):length] = both          # ending with the record: the byte-wise tail loop completes them
    text = np.ascontiguousarray(data[:, :length]).reshape(-1)
    offs = np.arange(n + 1, dtype=np.uint64) * length
    run = _PairRun(torch_cuda, t1, t2, data, length)
    for flags in (BE, ob.FLAG_BEGIN, ob.FLAG_END, 0):
        r1 = o1.run(text, offs, flags=flags, threads=4)
        r2 = o2.run(text, offs, flags=flags, threads=4)
        if flags & ob.FLAG_BEGIN:
            assert (r1[0][head] == s1).all() and (r2[0][head] == s2).all()
            assert (r1[0][task % 3 == 2] == s1).all() and (r2[0][task % 3 == 2] == s2).all()
            assert (r1[0][task % 3 == 0] != s1).all() and (r2[0][task % 3 == 0] != s2).all()
        for r in range(3):
            _same(run(flags=flags), r1, r2, (flags, r))
            assert pb.last_kernel() == "pair_tiled", (length, stride)


def test_pair_with_a_visited_state_in_row_254(pa, torch_cuda, cfg):
    """Table A keeps 254 dense rows of its 255: the state with device id 254 becomes A's trap id and is walked exactly, as
    side B it has its row.  set_d over a text that visits that very state, as side A and as side B of `string`."""
    from pire_amd import binding as pb

    blob = _blob("set_d")
    _, os_, ws, ss = _side("string")
    od = ob.OracleScanner(blob)
    td, ts = pa.Table(blob), pa.Table(_blob("string"))
    assert td.info.hot_states == 255
    s254 = int(td.layout()[0][PAIR_HOT_A])
    path = _path_to(od, _begin_state(od), lambda s: s == s254)
    big = [b for b in H.big_sets() if b["name"] == "set_d"][0]
    n, length = 64 * 64, 1024
    data = ob.corpus_fill(11, 0, n, length, H.plants_for(big), threads=4).copy()
    rows = np.arange(n)
    data[rows % 2 == 0, :len(path)] = np.frombuffer(path, dtype=np.uint8)                  # through the state ...
    data[rows % 4 == 0, length - len(path):] = np.frombuffer(path, dtype=np.uint8)         # ... and, as far as the text before
    data[rows % 8 == 1, 40:43] = np.frombuffer(ws, dtype=np.uint8)                         # allows, ending in it
    offs = np.arange(n + 1, dtype=np.uint64) * length
    visits = od.visit_counts(data.reshape(-1), offs)
    assert visits[s254] >= n // 2, (s254, int(visits[s254]))
    rd = od.run(data.reshape(-1), offs, threads=4)
    rs = os_.run(data.reshape(-1), offs, threads=4)
    assert int(td.layout()[0][PAIR_HOT_A]) == s254                   # still the ranking the text was made for
    for t1, t2, r1, r2 in ((td, ts, rd, rs), (ts, td, rs, rd)):
        run = _PairRun(torch_cuda, t1, t2, data, length)
        for r in range(3):
            _same(run(), r1, r2, r)
            assert pb.last_kernel() == "pair_tiled"


@pytest.mark.parametrize("n1,n2", [("string", "dict_1k"), ("dict_1k", "same")], ids=["string+dict_1k", "dict_1k+same"])
def test_pair_remainder_and_null_outputs(pa, torch_cuda, cfg, n1, n2):
    """n = 64 k + r: the fused pass over the whole tasks, two ordinary passes over the last r records, their Finals or-ed;
    exactly one task; each of the three output pointers null in turn (what is not asked for stays untouched)."""
    from pire_amd import binding as pb

    t1, t2 = _pair_tables(pa, n1, n2)
    length = 512
    for n in (64, 64 * 9 + 1, 64 * 9 + 63):
        i = np.arange(n)
        in_a = ((i // 32) % 3) != 1                            # wholly and half absorbed tasks, a mixed remainder;
        in_b = in_a ^ (i % 5 == 0)                             # every fifth record Final on one side alone
        data, r1, r2 = _pair_corpus(n1, n2, n, length, in_a, in_b, seed=n)
        assert n % 64 == 0 or (r1[1] | r2[1])[n & ~63:].any()
        assert n1 == n2 or n2 == "same" or ((r1[1] != r2[1]).any() and (r1[1] != r2[1])[n & ~63:].any() == (n % 64 > 1))
        run = _PairRun(torch_cuda, t1, t2, data, length)
        _same(run(n=n & ~63), _head(r1, n & ~63), _head(r2, n & ~63))
        assert pb.last_kernel() == "pair_tiled"                # the same text, len and stride: the fused part of the calls below
        for outs in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
            g1, g2, gf = run(outs=outs)
            # two ordinary passes over n >= 64 records would be tiled passes: "generic" is the remainder's alone
            assert pb.last_kernel() == ("pair_tiled" if n % 64 == 0 else "generic")
            assert (g1 == r1[0]).all() if outs[0] else (g1 == np.uint32(-2 & 0xFFFFFFFF)).all(), (n, outs)
            assert (g2 == r2[0]).all() if outs[1] else (g2 == np.uint32(-2 & 0xFFFFFFFF)).all(), (n, outs)
            assert (gf == (r1[1] | r2[1])).all() if outs[2] else (gf == 9).all(), (n, outs)


# ------------------------------------------------------------------------------------------------ B. the segmented scan

SEG_SYMBOL = {"one mode": "pirehip::ScanTiledSegKernel", "two modes": "pirehip::ScanPairTiledKernel"}


SEG_PERIOD = 48 * 1024


def _seg_filler(total):
    """Bytes that cannot match and that take both scanners back to their start state."""
    base = np.frombuffer(b"_ =/\n_", dtype=np.uint8)
    return np.resize(base[np.random.RandomState(7).randint(0, len(base), size=SEG_PERIOD)], total)


def _seg_text(name, total, free=()):
    """`total` bytes that are absorbed from early on: the witness every 48 bytes in the filler; `free`: (begin, end)
    stretches of filler alone."""
    _, o, w, s = _side(name)
    block = _seg_filler(SEG_PERIOD)
    pos = np.arange(5, SEG_PERIOD - len(w), 48)
    block[pos[:, None] + np.arange(len(w))[None, :]] = np.frombuffer(w, dtype=np.uint8)
    text = np.resize(block, total)
    for b, e in free:
        text[b:e] = _seg_filler(e - b)
    return text


def _seg_config(cfg, kernel, seg, warm, budget=32):
    # "one mode": nothing is learned, the grid segments take ScanTiledSegKernel; "two modes": mode 0 and the first mode the
    # table has learned, walked (not derived, no product automaton) in one pass of the pair kernel
    cfg.set(segment_bytes=seg, segment_warmup=warm, segment_budget=budget, segment_modes=1 if kernel == "one mode" else 2,
            segment_no_pair=0, segment_no_derive=1, segment_no_product=1)


def _seg_table(pa, torch, cfg, name, kernel):
    """A table for one of the two passes.  "two modes": taught its absorbing state as a mode by a first scan without warm-up
    and without repair rounds (every absorbed segment is then a surprise, and the surprise becomes a mode at once)."""
    from pire_amd import binding as pb

    blob, o, w, s = _side(name)
    t = pa.Table(blob)
    assert _dev_id(t, s) < t.info.hot_states, (name, _dev_id(t, s))   # a dense row: otherwise there is no early-out
    if kernel == "two modes":
        _seg_config(cfg, kernel, 1024, 0, budget=0)
        text = _seg_text(name, 256 * 1024)
        got = _seg_run(torch, t, text, 1, len(text))
        want = o.run(text, np.array([0, len(text)], dtype=np.uint64))
        assert pb.last_kernel().startswith("segmented") and got[0][0] == want[0][0] == s and got[1][0] == want[1][0]
    return t, o, s


def _seg_run(torch, t, text, n, length, d=None):
    d = torch.as_tensor(text, device="cuda") if d is None else d
    idx = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    fin = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    t.run_strided_device(d.data_ptr(), n, length, length, BE, idx.data_ptr(), fin.data_ptr(), 0, 0,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.uint32), fin.cpu().numpy()


SEG_SHAPES = [(1, (1 << 21) + 777), (3, 1 << 19)]


@pytest.mark.parametrize("kernel", ["one mode", "two modes"])
@pytest.mark.parametrize("name", ["string", "dict_1k"])
@pytest.mark.parametrize("n,length", SEG_SHAPES, ids=["one string", "three strings"])
def test_segment_kernels_on_text_absorbed_from_early_on(pa, torch_cuda, cfg, kernel, name, n, length):
    """All 64 segments of most tasks are in the absorbing state right behind their warm-up: the task ends by the early-out;
    then the same with witness-free stretches of a whole task at a string's start and in its middle -- live tasks between
    absorbed ones, and in the middle stretch a guess that is not absorbing while the true state is, so that the chain's
    repair rounds run (and, without a budget, the plain walk)."""
    from pire_amd import binding as pb

    t, o, s = _seg_table(pa, torch_cuda, cfg, name, kernel)
    offs = np.arange(n + 1, dtype=np.uint64) * length
    for seg in (1024, 2048, 4096):
        stretch = 64 * seg
        starts, middles = [], []       # (string's first byte, hole's end); a string too short for both has one of them
        for i in range(n):
            if length >= 4 * stretch or i % 2 == 0:
                starts.append((i * length, i * length + stretch))
            if length >= 4 * stretch or i % 2 == 1:
                mid = i * length + max(1, (length // 2) // stretch) * stretch
                middles.append((i * length, mid + stretch))
        holes = starts + [(e - stretch, e) for _, e in middles]
        for free, budgets in (((), (32,)), (holes, (32, 0))):
            text = _seg_text(name, n * length, free)
            oi, of = o.run(text, offs, threads=4)
            assert (oi == s).all() and of.all()
            if free:   # live where it is meant to be: not absorbed at the end of a first stretch, absorbed all through a middle one
                cuts = [(x, False) for x in starts] + [(x, True) for x in middles] + [((b, e - stretch), True) for b, e in middles]
                for (b, e), want in cuts:
                    assert (o.run(text, np.array([b, e], dtype=np.uint64))[0][0] == s) == want, (b, e, want)
            d = torch_cuda.as_tensor(text, device="cuda")
            for warm in (0, 256):
                for budget in budgets:
                    _seg_config(cfg, kernel, seg, warm, budget)
                    gi, gf = _seg_run(torch_cuda, t, text, n, length, d)
                    assert pb.last_kernel().startswith("segmented") and pb.last_kernel_symbol() == SEG_SYMBOL[kernel], \
                        (pb.last_kernel(), pb.last_kernel_symbol(), seg, warm, budget)
                    assert (gi == oi).all() and (gf == of).all(), (seg, warm, budget, bool(free))


_TASKS = {}


def _task_strings(torch, name, seg, per_cu):
    """Strings of exactly one task (64 segments) each, `per_cu` of them for every CU and 37 more; two of three absorbed
    from their first bytes on, the third without a witness: its end state is the filler's, and only if every segment of it
    was walked over its OWN bytes.  With more than 16 tasks per CU a wave walks several tasks through the chain tile; its
    next task is blocks * waves tasks on."""
    _, o, w, s = _side(name)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    key = (name, seg, per_cu, cus)
    if _TASKS.get("key") == key:
        return _TASKS["value"]
    _TASKS.clear()
    n, length = per_cu * cus + 37, 64 * seg
    step = cus * 16
    i = np.arange(n)
    live = (i + i // step) % 3 == 0          # whatever the CU count: a wave's tasks are not all of one kind
    text = _seg_text(name, n * length).reshape(n, length)
    text[live] = _seg_filler(length)
    oi, of = o.run(text.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=8)
    assert (oi[~live] == s).all() and of[~live].all() and (oi[live] != s).all() and not of[live].any()
    # the filler takes the scanner back to where a segment's guess without a warm-up is made from: the live strings' chains
    # hold, so their answers are the segment kernel's
    first = np.ascontiguousarray(text[np.nonzero(live)[0][0]])
    prefixes = [first[:k * seg].tobytes() for k in range(1, 65)]     # ... at every one of its segment boundaries
    assert (o.run_strings(prefixes, flags=ob.FLAG_BEGIN)[0] == _begin_state(o)).all()
    _TASKS.update(key=key, value=(text, n, length, oi, of))
    return _TASKS["value"]


@pytest.mark.parametrize("kernel", ["one mode", "two modes"])
@pytest.mark.parametrize("name", ["string", "dict_1k"])
@pytest.mark.parametrize("per_cu,seg", [(3, 1024), (33, 512)], ids=["3 tasks per CU", "33 tasks per CU"])
def test_segment_kernels_few_and_many_tasks_per_cu(pa, torch_cuda, cfg, kernel, name, per_cu, seg):
    """Both branches of waves = max(4, min(16, tasks per CU)) of the two launchers: small blocks with one task per wave, and
    full blocks whose waves chain two and three tasks -- absorbed ones (left early, a tile of their own still on its way)
    in front of live ones.  Without a warm-up the first tile a task walks is its segments' first 128 bytes: a task that
    walked the tile its predecessor left behind returns a live string absorbed."""
    from pire_amd import binding as pb

    t, o, s = _seg_table(pa, torch_cuda, cfg, name, kernel)
    text, n, length, oi, of = _task_strings(torch_cuda, name, seg, per_cu)
    d = torch_cuda.as_tensor(text, device="cuda")
    for warm in (0, 256):
        for r in range(2):
            _seg_config(cfg, kernel, seg, warm)
            gi, gf = _seg_run(torch_cuda, t, text, n, length, d)
            assert pb.last_kernel().startswith("segmented") and pb.last_kernel_symbol() == SEG_SYMBOL[kernel], \
                (pb.last_kernel(), pb.last_kernel_symbol(), warm)
            bad = np.nonzero((gi != oi) | (gf != of))[0]
            assert len(bad) == 0, (warm, r, len(bad), bad[:10].tolist())


@pytest.mark.parametrize("kernel", ["one mode", "two modes"])
@pytest.mark.parametrize("name", ["string", "dict_1k"])
def test_segment_kernels_repeated(pa, torch_cuda, cfg, kernel, name):
    """REPS // 2 launches of each pass over the text that is absorbed from early on."""
    from pire_amd import binding as pb

    t, o, s = _seg_table(pa, torch_cuda, cfg, name, kernel)
    n, length = SEG_SHAPES[0]
    text = _seg_text(name, n * length)
    oi, of = o.run(text, np.arange(n + 1, dtype=np.uint64) * length)
    assert (oi == s).all() and of.all()
    d = torch_cuda.as_tensor(text, device="cuda")
    _seg_config(cfg, kernel, 1024, 256)
    for r in range(REPS // 2):
        gi, gf = _seg_run(torch_cuda, t, text, n, length, d)
        assert (gi == oi).all() and (gf == of).all(), r
        assert pb.last_kernel() == "segmented" and pb.last_kernel_symbol() == SEG_SYMBOL[kernel], (r, pb.last_kernel_symbol())
