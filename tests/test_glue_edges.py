"""Scanner::Glue on the device (pire_hip_table_glue_gpu, pire_amd/csrc/glue.hip) at its level, cap and hash-table edges.

The comparator is a MODEL of the construction in plain Python (glue_model below), over the operands' accessors alone: it
restates glue.h:123-137 (letter classes, Next of a pair), determine.h:100-122 (the breadth-first numbering) and
multi.h:1024-1043 (flags and accepted regexps), needs neither a GPU nor the reference tree, and also yields what no table
shows: the boundaries h_0 = 1 < h_1 < ... < h_K = N of the breadth-first levels and the number of distinct target pairs of
every level.  tests/golden/glue (make_glue_inputs.py) holds the operands' Save() blobs and the same figures read off the
reference's own left-to-right Scanner::Glue, with what that Glue answered for every max_size of the sweeps below.

With two answer-only changes to glue.hip on a scratch copy the GPU group fails where it should."""
import json
import os

import numpy as np
import pytest

from oracle import binding as ob
from tests import helpers as H

with open(os.path.join(H.GOLDEN, "glue", "cases.json")) as _f:
    DOC = json.load(_f)
PAIRS = {p["name"]: p for p in DOC["pairs"]}
CHARS = [c for c in range(264) if c != 257]          # 0 .. MaxChar - 1 without Epsilon (glue.h:125-127)
DEVICE_LIMIT = 1 << 22                               # glue.hip GlueBfsDevice: above it the host version answers


@pytest.fixture(scope="module")
def pa():
    import pire_amd

    return pire_amd


# ------------------------------------------------------------------------------------------------------------ the model

class Dfa:
    """What the model reads of an operand and what it builds: cls[char], next[state][class], final / dead / accepted per state."""

    def __init__(self, cls, nxt, fin, dead, acc, initial, regexps):
        self.cls, self.next, self.final, self.dead, self.accepted = cls, nxt, fin, dead, acc
        self.initial, self.regexps = initial, regexps
        self.size, self.letters = len(nxt), len(nxt[0])

    @classmethod
    def read(cls, o):
        """from accessors (an OracleScanner, or a Table through Accessors): every state, every class by its first char"""
        classes = [o.letter_class(c) for c in CHARS]
        reps = {}
        for c, k in zip(CHARS, classes):
            reps.setdefault(k, c)
        assert sorted(reps) == list(range(o.letters)), "letter classes are not 0 .. LettersCount - 1"
        by_class = [reps[k] for k in range(o.letters)]
        states = range(o.size)
        return cls(classes, [[o.next(s, c) for c in by_class] for s in states], [bool(o.final(s)) for s in states],
                   [bool(o.dead(s)) for s in states], [list(o.accepted(s)) for s in states], o.initial, o.regexps)

    def representatives(self):
        reps = {}
        for c, k in zip(CHARS, self.cls):
            reps.setdefault(k, c)
        return [reps[k] for k in range(self.letters)]


class Accessors:
    """a pire_amd.Table under the accessor names of the oracle's scanners"""

    def __init__(self, t):
        self.size, self.letters, self.regexps, self.initial = t.Size, t.LettersCount, t.RegexpsCount, t.initial
        self.letter_class, self.next, self.final, self.dead, self.accepted = t.letter_class, t.Next, t.Final, t.Dead, t.AcceptedRegexps


def glue_model(a, b):
    """The product of two Dfa as the reference numbers it; .bounds and .distinct are the levels' figures."""
    # glue.h:123-127: the classes are the pairs of the operands' classes, numbered as their first char arrives
    number, cls, la, lb = {}, [], [], []
    for ca, cb in zip(a.cls, b.cls):
        if (ca, cb) not in number:
            number[(ca, cb)] = len(la)
            la.append(ca)
            lb.append(cb)
        cls.append(number[(ca, cb)])
    # determine.h:103-122: states in index order, classes in order, a pair seen for the first time takes the next index
    states, index, nxt = [(a.initial, b.initial)], {(a.initial, b.initial): 0}, []
    bounds, distinct, lo = [1], [], 0
    while lo < len(states):
        hi, targets = len(states), set()
        for sa, sb in states[lo:hi]:
            row = []
            for ka, kb in zip(la, lb):
                t = (a.next[sa][ka], b.next[sb][kb])                    # glue.h:132-137
                if t not in index:
                    index[t] = len(states)
                    states.append(t)
                targets.add(t)
                row.append(index[t])
            nxt.append(row)
        distinct.append(len(targets))
        if len(states) > hi:
            bounds.append(len(states))
        lo = hi
    # multi.h:1024-1043: Final = either, Dead = both, lhs ids and then rhs ids behind them
    m = Dfa(cls, nxt, [a.final[x] or b.final[y] for x, y in states], [a.dead[x] and b.dead[y] for x, y in states],
            [a.accepted[x] + [r + a.regexps for r in b.accepted[y]] for x, y in states], 0, a.regexps + b.regexps)
    m.bounds, m.distinct = bounds, distinct
    return m


def assert_same(got, want):
    """two Dfa, exhaustively; the first difference is named"""
    assert (got.size, got.letters, got.regexps, got.initial) == (want.size, want.letters, want.regexps, want.initial)
    assert got.cls == want.cls, [(c, g, w) for c, g, w in zip(CHARS, got.cls, want.cls) if g != w][:5]
    for s in range(want.size):
        assert got.next[s] == want.next[s], (s, got.next[s], want.next[s])
        assert (got.final[s], got.dead[s], got.accepted[s]) == (want.final[s], want.dead[s], want.accepted[s]), s


# ------------------------------------------------------------------------------------------------------------- fixtures

_memo = {}


def operand_blob(name):
    return H.load_blob(os.path.join("glue", DOC["operands"][name]["blob"]))


def operand(name):
    """the operand as the model reads it, from the reference's Save() blob (read once, left unchanged)"""
    if ("dfa", name) not in _memo:
        _memo["dfa", name] = Dfa.read(ob.OracleScanner(operand_blob(name)))
    return _memo["dfa", name]


def model(pair):
    if ("model", pair) not in _memo:
        _memo["model", pair] = glue_model(operand(PAIRS[pair]["lhs"]), operand(PAIRS[pair]["rhs"]))
    return _memo["model", pair]


def tables(pa, pair):
    """(lhs, rhs) Tables; `self` is one handle twice"""
    p = PAIRS[pair]
    a = pa.Table(operand_blob(p["lhs"]))
    return a, (a if p["rhs"] == p["lhs"] else pa.Table(operand_blob(p["rhs"])))


def sweep(pair):
    """{1, 2} + {h - 2, h - 1, h for every boundary} + {N - 2, N - 1, N}, positive values only"""
    bounds = model(pair).bounds
    n = bounds[-1]
    vals = {1, 2, n - 2, n - 1, n}
    for h in bounds:
        vals |= {h - 2, h - 1, h}
    return sorted(v for v in vals if v > 0)


def ref_pattern(name):
    o = DOC["operands"][name]
    return bytes.fromhex(o["pattern_hex"]), o["options"]


def ref_glues(names, m=0):
    """the live reference's left-to-right Glue: the glued scanner, or None where it failed"""
    try:
        ref = ob.RefScanner.compile([ref_pattern(n)[0] for n in names], [ref_pattern(n)[1] for n in names], glue_max=m)
    except ValueError as e:
        assert "gluing failed" in str(e), e
        return None
    return None if ref.empty else ref


def is_failure(t):
    """task.Failure() = Scanner(): the empty scanner (glue.h:146, multi.h:121)"""
    return bool(t.Empty) and t.RegexpsCount == 0


# ------------------------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("pair", list(PAIRS))
def test_model_figures_are_the_references(pair):
    """N, LC, the level boundaries and distinct_k of the model == what was read off the reference's glued table."""
    m, p = model(pair), PAIRS[pair]
    assert (m.size, m.letters) == (p["N"], p["LC"])
    assert m.bounds == p["boundaries"] and m.distinct == p["distinct"]
    assert m.bounds[0] == 1 and m.bounds[-1] == m.size and len(m.distinct) == len(m.bounds)


def test_fixtures_reach_what_they_are_for():
    """The shapes the cases below rest on, from the model's figures (so a regenerated fixture cannot quietly lose them)."""
    t = model("tiny")
    assert t.bounds == [1, 3, 5, 8, 12, 14, 16, 18, 21, 24, 28, 30, 32, 33] and t.letters == 11
    assert (model("self").size, model("self").letters) == (3, 3)
    c = model("chain")
    assert len(c.bounds) > 300 and c.size == 604                       # hundreds of levels, each with its read-backs
    assert model("classes").letters > 127 and model("classes").size < 3000
    r = model("trie")
    widths = [(h - l) * r.letters for l, h in zip([0] + r.bounds, r.bounds)]
    assert max(widths) == 67991 and r.bounds[:4] == [1, 11, 651, 1534] and r.distinct[:3] == [11, 651, 904]


@pytest.mark.parametrize("pair", list(PAIRS))
def test_host_glue_is_the_model(pa, pair):
    """Table.glue(a, b) on the host == the model in every state, letter and flag; and so is the live reference where built."""
    a, b = tables(pa, pair)
    t = pa.Table.glue(a, b)
    assert not t.Empty
    assert_same(Dfa.read(Accessors(t)), model(pair))
    if ob.ref_available():
        ref = ref_glues([PAIRS[pair]["lhs"], PAIRS[pair]["rhs"]])
        assert_same(Dfa.read(ob.OracleScanner(ref.save())), model(pair))


@pytest.mark.parametrize("pair", ["tiny", "trie"])
def test_host_failure_rule_over_the_sweep(pa, pair):
    """host Empty == recorded reference == (max_size < N - 1) at every level boundary; a glued result is the whole product."""
    a, b = tables(pa, pair)
    n, rec = model(pair).size, PAIRS[pair]["glued_at"]
    for m in sweep(pair):
        t = pa.Table.glue(a, b, m)
        assert is_failure(t) == (not rec[str(m)]) == (m < n - 1), m
        assert t.Empty == is_failure(t)
        if not t.Empty:
            assert_same(Dfa.read(Accessors(t)), model(pair))
    if ob.ref_available():                                              # the live reference against the same rule
        names = [PAIRS[pair]["lhs"], PAIRS[pair]["rhs"]]
        for m in (sweep(pair) if pair == "tiny" else [10, n - 2, n - 1]):
            assert (ref_glues(names, m) is None) == (m < n - 1), m


def abc_models():
    a, b, c = operand("hello"), operand("acd"), operand("xy")
    return glue_model(glue_model(a, b), c), glue_model(a, glue_model(b, c))


def check_products_of_products(pa, gpu):
    a, b, c = (pa.Table(operand_blob(n)) for n in DOC["abc_left"]["operands"])
    left_model, right_model = abc_models()
    left = pa.Table.glue(pa.Table.glue(a, b, gpu=gpu), c, gpu=gpu)
    assert_same(Dfa.read(Accessors(left)), left_model)
    rec = DOC["abc_left"]
    assert_same(Dfa.read(Accessors(left)), Dfa.read(ob.OracleScanner(H.load_blob(os.path.join("glue", rec["blob"])))))
    assert (left.Size, left.LettersCount) == (rec["N"], rec["LC"])
    right = pa.Table.glue(a, pa.Table.glue(b, c, gpu=gpu), gpu=gpu)       # the reference never builds this one: the model alone
    assert_same(Dfa.read(Accessors(right)), right_model)
    assert right.RegexpsCount == 3
    return left, right


def test_host_products_of_products(pa):
    """glue(glue(a, b), c) == the reference's own table and the model; glue(a, glue(b, c)) == the model."""
    assert DOC["abc_left"]["operands"] == ["hello", "acd", "xy"]
    check_products_of_products(pa, gpu=False)
    if ob.ref_available():
        assert_same(Dfa.read(ob.OracleScanner(ref_glues(DOC["abc_left"]["operands"]).save())), abc_models()[0])


@pytest.mark.parametrize("gpu", [False, True])
def test_refusals_and_empty_operands_need_no_device(pa, gpu):
    """What both entry points decide before a device is touched: a SimpleScanner table or a counting table as either operand is
    PireHipError (and not the missing device's: the message names the rule); an empty operand returns the other one."""
    a = pa.Table(operand_blob("hello"))
    simple = pa.Table(H.load_blob([c for c in H.golden()["simple"] if c["name"] == "simple_hello"][0]["blob"]))
    case = H.golden()["counting"][0]
    counting = pa.CountingTable(H.load_blob(case["blob"]), case["kind"])
    for other in (simple, counting):
        for lhs, rhs in ((other, a), (a, other), (other, other)):
            with pytest.raises(pa.PireHipError, match="Pire::Scanner tables"):
                pa.Table.glue(lhs, rhs, gpu=gpu)
    empty = pa.Table(H.load_blob([c for c in H.all_cases() if c["name"] == "empty_scanner"][0]["blob"]))
    assert empty.Empty
    want = Dfa.read(Accessors(a))
    for t in (pa.Table.glue(empty, a, gpu=gpu), pa.Table.glue(a, empty, gpu=gpu), pa.Table.glue(a, empty, 1, gpu=gpu)):
        assert not t.Empty
        assert_same(Dfa.read(Accessors(t)), want)
    both = pa.Table.glue(empty, empty, gpu=gpu)
    assert both.Empty and both.RegexpsCount == 0


# ------------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch_cuda(pa):
    import torch

    assert torch.cuda.is_available() and pa.device_count() > 0
    return torch


def device_next_columns(torch, t, reps):
    """[class][state] -> Next, through the device image of the table: one pire_hip_step over all states per class"""
    out = []
    start = torch.arange(t.Size, dtype=torch.int32, device="cuda")
    for ch in reps:
        st = start.clone()
        t.step_device(st.data_ptr(), t.Size, ch, torch.cuda.current_stream().cuda_stream)
        out.append(st)
    torch.cuda.synchronize()
    return [c.cpu().numpy().tolist() for c in out]


def assert_device_table_is(torch, t, m):
    """the glued table == the model m: the accessors exhaustively, and what the device walks"""
    assert not t.Empty
    assert_same(Dfa.read(Accessors(t)), m)
    for k, col in enumerate(device_next_columns(torch, t, m.representatives())):
        assert col == [row[k] for row in m.next], k


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
def test_gpu_numbering_is_the_model(pa, torch_cuda, pair):
    """(a) Table.glue(a, b, gpu=True) == the model: 303 levels of two states (chain), 134 letter classes (classes), a table
    with itself (self), and first occurrences that compete across the 266 blocks of one level (trie)."""
    m = model(pair)
    if pair == "trie":
        assert max((h - l) * m.letters for l, h in zip([0] + m.bounds, m.bounds)) > 256   # more than one 256-thread block
    if pair == "classes":
        assert m.letters > 127
    a, b = tables(pa, pair)
    assert_device_table_is(torch_cuda, pa.Table.glue(a, b, gpu=True), m)


@pytest.mark.gpu
def test_gpu_glue_is_deterministic(pa, torch_cuda):
    """(a) three device glues of the trie product (atomics across blocks) give one table, bit for bit."""
    a, b = tables(pa, "trie")
    runs = [Dfa.read(Accessors(pa.Table.glue(a, b, gpu=True))) for _ in range(3)]
    for r in runs:
        assert_same(r, model("trie"))
    for r in runs[1:]:
        assert (r.cls, r.next, r.final, r.dead, r.accepted) == (runs[0].cls, runs[0].next, runs[0].final, runs[0].dead, runs[0].accepted)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["tiny", "trie"])
def test_gpu_failure_rule_over_the_sweep(pa, torch_cuda, pair):
    """(b) device Empty == host Empty == recorded reference == (max_size < N - 1) two below, one below and at every level
    boundary: the per-level decision of the device against the per-state decision of determine.h:112-113."""
    a, b = tables(pa, pair)
    n, rec = model(pair).size, PAIRS[pair]["glued_at"]
    for m in sweep(pair):
        dev, host = pa.Table.glue(a, b, m, gpu=True), pa.Table.glue(a, b, m)
        assert is_failure(dev) == is_failure(host) == (not rec[str(m)]) == (m < n - 1), m
        assert dev.Empty == is_failure(dev) and host.Empty == is_failure(host), m
        if not dev.Empty:                                               # every non-empty result is the unbounded product
            assert_same(Dfa.read(Accessors(dev)), model(pair))
            assert_same(Dfa.read(Accessors(host)), model(pair))


@pytest.mark.gpu
@pytest.mark.parametrize("max_size", [10, 11, 12])
def test_gpu_full_pair_table_hands_over(pa, torch_cuda, max_size):
    """(c) cap = max_size + 1 >= 11 lets level 0 through, and level 1 meets more distinct pairs than the pair table has slots:
    SlotOf gives up after maxProbe probes (bounded: it cannot spin) and the sequential version decides.  Which side
    answered cannot be seen from here; the answer must be the reference's: the empty scanner."""
    m = model("trie")
    cap = max_size + 1
    # glue.hip GlueBfsDevice owns this formula: hashSize = the smallest power of two >= 4 * (cap + 64)
    slots = 1
    while slots < 4 * (cap + 64):
        slots *= 2
    assert cap >= m.bounds[1]                                           # level 0 passes the failure rule
    assert m.distinct[1] + m.bounds[1] > slots and m.distinct[1] > slots   # level 1 cannot fit, whatever it shares with level 0
    assert PAIRS["trie"]["glued_at"][str(max_size)] is False            # the reference fails here
    a, b = tables(pa, "trie")
    t = pa.Table.glue(a, b, max_size, gpu=True)
    assert t.Empty and t.RegexpsCount == 0
    assert is_failure(pa.Table.glue(a, b, max_size))


@pytest.mark.gpu
def test_gpu_largest_device_max_size_and_the_host_hand_over(pa, torch_cuda):
    """(d) max_size = 2^22 is the largest the device buffers are sized for (about 0.4 GB at 3 letter classes); 2^22 + 1
    goes to the host version.  Both are the unbounded product."""
    a, b = tables(pa, "self")
    for m in (DEVICE_LIMIT + 1, DEVICE_LIMIT):
        assert_device_table_is(torch_cuda, pa.Table.glue(a, b, m, gpu=True), model("self"))
    a, b = tables(pa, "tiny")
    assert_device_table_is(torch_cuda, pa.Table.glue(a, b, DEVICE_LIMIT + 1, gpu=True), model("tiny"))


@pytest.mark.gpu
def test_gpu_products_of_products(pa, torch_cuda):
    """(e) operands that are device products themselves, in both associations."""
    left, right = check_products_of_products(pa, gpu=True)
    left_model, right_model = abc_models()
    assert_device_table_is(torch_cuda, left, left_model)
    assert_device_table_is(torch_cuda, right, right_model)


def probe_strings(pair):
    """2000 strings over the operands' alphabet: words and cut words of the patterns between noise"""
    rng = np.random.RandomState(5)
    if pair == "tiny":
        pieces = [b"hell", b" ", b"\t", b"w", b"orl", b"a", b"b", b"c", b"x", b"zq", b"o w"]
        whole = [b"hello \t world", b"abcdxyzw", b"ccaadd d d"]
    else:
        words = ref_pattern("trie")[0].decode()[1:-2].split("|")
        assert len(words) == 630
        pieces = [w.encode()[:k] for w in words[::7] for k in (1, 2, 5, 12)] + [b"z", b"ab", b" "]
        whole = [w.encode() + b"z" for w in words] + [b"q"]
    out = []
    for _ in range(2000):                       # noise, then a word of the patterns cut anywhere (seldom whole: behind a match
        w = whole[rng.randint(0, len(whole))]   # a Surround()ed scanner stays where it is)
        out.append(b"".join(pieces[i] for i in rng.randint(0, len(pieces), size=rng.randint(0, 4))) + w[:rng.randint(0, len(w) + 1)])
    return out


REACHED = {"tiny": 12, "trie": 300}     # distinct states the probe strings must end in: a third of tiny's 33, hundreds of trie's


def model_walk(m, strings):
    """(state behind BeginMark and the string's bytes, state behind EndMark as well) per string, by the model's table"""
    begin, end, inside, whole = m.cls[CHARS.index(258)], m.cls[CHARS.index(259)], [], []
    for s in strings:
        st = m.next[m.initial][begin]
        for byte in s:
            st = m.next[st][m.cls[byte]]
        inside.append(st)
        whole.append(m.next[st][end])
    return inside, whole


def test_probe_strings_go_somewhere():
    """The strings of the scan below end in many states of the products, matching and not (by the model: no GPU needed)."""
    for pair in ("tiny", "trie"):
        inside, whole = model_walk(model(pair), probe_strings(pair))
        assert len(set(inside)) > REACHED[pair] and 0 < sum(model(pair).final[s] for s in whole) < 2000, pair


@pytest.mark.gpu
@pytest.mark.parametrize("pair", ["tiny", "trie"])
def test_gpu_glued_table_scans_like_the_host_glued_one(pa, torch_cuda, pair):
    """(f) one scan through the result: the same state indices and Final flags from the device-glued and the host-glued table
    (with and without the EndMark step), which are the model's own walk."""
    a, b = tables(pa, pair)
    strings = probe_strings(pair)
    inside, whole = model_walk(model(pair), strings)
    assert len(set(inside)) > REACHED[pair] and 0 < sum(model(pair).final[s] for s in whole) < len(strings)
    dev, host = pa.Table.glue(a, b, gpu=True), pa.Table.glue(a, b)
    got = [x.tolist() for t in (dev, host) for flags in (ob.FLAG_BEGIN, ob.FLAG_BEGIN | ob.FLAG_END) for x in t.run_strings(strings, flags=flags)]
    assert got[:4] == got[4:] and got[4] == inside and got[6] == whole and got[7] == [int(model(pair).final[s]) for s in whole]
