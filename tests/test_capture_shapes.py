"""pire_hip_capture_run on tables of every shape its routing distinguishes (pire_amd/csrc/counting.hip):

    capture_rows                        states <= 34, dense form, counting_variant = 2 (or a batch that fills the GPU)
    capture_dense, blocks of 256        35..80 states   (states * 512 <= 40 KiB)
    capture_dense, blocks of 1024       81..255 states
    capture, transitions in LDS         more than 255 states or PIRE_HIP_RUN_GENERIC; states * letters * 8 <= 60 KiB
    capture, transitions in memory      the same above 60 KiB
    ragged_capture                      n >= 256, letters <= 127: the expanded table (state x pending action) on the
                                        ragged kernel -- dense rows, compact tier, cold states re-walked exactly
    (ragged_capture declines)           more than 127 letter classes: no expanded table, the per-lane kernel takes the batch

The fixtures (tests/golden/make_golden.py, capture_shapes()) are compiled by the unmodified reference and assert their
shape in the generator; the tests assert it again from pire_hip_counting_table_get_info.  Every answer is compared,
exactly, with the plain-C restatement oracle.binding.OracleCountingScanner.capture, which tests/test_capture.py holds
against the reference itself on every fixture, and which test_random_capture_* hold against it on every drawn scanner.

A capturing scanner with more than 127 letter classes exists: `capture_ascii124` (253 states, 130 letters).
What was tried on the way: the 134-symbol construction with 64 Cyrillic letters gives 74 letters (the capture
compile path takes the pattern byte by byte and ignores the `u` option; bytes >= 0x80 are refused by the lexer as
"Control character in tokens sequence", so are escaped bytes other than the lexer's own controls); 88 printable ASCII
symbols give 92-94 letters; all 120 ASCII bytes 1..127 except `abz[]{}` give 124-126; with `\\[ \\] \\{ \\}` as well
(124 symbols) 128, and 130 with `^` / `$` alternatives, which give BeginMark and EndMark classes of their own.  No
fixture combines more than 255 states with more than 127 letters; the kernels that case takes (capture, transitions in
device memory) are those of capture_words150 and, under PIRE_HIP_RUN_GENERIC, of capture_ascii124 itself.
"""
import numpy as np
import pytest

from oracle import binding as ob
from tests import helpers as H

FLAGS = (3, 0, 1, 2)      # PIRE_HIP_RUN_BEGIN | _END, neither, BEGIN alone, END alone


def fixtures():
    return [c for c in H.golden().get("capturing", []) if "shape" in c]


@pytest.fixture(scope="module")
def pa():
    import pire_amd

    assert pire_amd.device_count() > 0
    return pire_amd


@pytest.fixture(scope="module")
def cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def per_lane(states, generic=False, variant=0, n=0, cus=1 << 30):
    """The one-string-per-lane kernel launchPerLane() takes (counting.hip)."""
    if generic or states > 255:
        return "capture"
    if states <= 34 and variant != 1 and (variant == 2 or n >= cus * 256):
        return "capture_rows"
    return "capture_dense"


def with_ragged(states, letters, n, always, **kw):
    """... behind the ragged kernel with actions: taken from 256 strings on where the expanded table exists (<= 127 letters)
    and either the library's estimate of the share of action states is small or ragged_act_always is set.  Returns the
    set of names the call may report."""
    lane = per_lane(states, n=n, **kw)
    if n < 256 or letters > 127:
        return {lane}
    return {"ragged_capture"} if always else {"ragged_capture", lane}


def shape_of(case, t):
    """The shape the generator asserted, asserted again from the library's own table info."""
    s, l = t.Size, t.LettersCount
    assert (s, l) == (case["states"], case["letters"])
    b = s * l * 8
    want = {"rows": s <= 34, "dense256": 34 < s <= 80, "dense1024": 80 < s <= 255 and l <= 127, "lds": s > 255 and b <= 60 * 1024,
            "global": s > 255 and b > 60 * 1024, "letters128": l > 127 and s <= 255}[case["shape"]]
    assert want, (case["name"], case["shape"], s, l, b)
    if case["name"] in ("capture_sym134", "capture_ascii124"):
        assert b > 60 * 1024        # under PIRE_HIP_RUN_GENERIC: the transitions stay in device memory
    return s, l


def build_batch(case, seed, n_noise=3600):
    """Like the batch of test_gpu_capture_parity: noise of the fixture's alphabet glued with planted witnesses, a witness at
    every offset 0..300 (all positions relative to 16-byte chunks and 128-byte windows), strings that are nothing but
    witnesses, every proper prefix of the witnesses and every 9-byte word over the alphabet's first two letters (end states
    all over the table), strings of several KiB, empty ones."""
    rng = np.random.RandomState(seed)
    a = np.frombuffer(bytes.fromhex(case["alphabet_hex"]), dtype=np.uint8)
    wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]

    def noise(k):
        return bytes(a[rng.randint(0, len(a), size=int(k))])

    many = []
    for _ in range(n_noise):
        many.append(b"".join(wit[rng.randint(0, len(wit))] if rng.randint(0, 4) == 0 else noise(rng.randint(0, 40))
                             for _ in range(rng.randint(0, 6))))
    for k in range(0, 301):
        many.append(noise(k) + wit[k % len(wit)] + noise(300 - k))
    many += wit + [w * 3 for w in wit[:40]] + [wit[0] * 40]
    prefixes = [w[:k] for w in wit for k in range(1, len(w))]
    many += prefixes[:1800]
    many += [bytes(a[(m >> k) & 1] for k in range(9)) for m in range(512)]     # every 9-byte word over two letters
    many += [noise(6000) + wit[1 % len(wit)] + noise(3000), wit[0] + noise(5000), noise(9000), b"", b"", b""]
    while len(many) < 5700:
        many.append(noise(rng.randint(0, 120)))
    order = rng.permutation(len(many))
    return [many[i] for i in order]


# What the library takes when left to itself (5 700 strings): the ragged kernel with actions unless its byte model puts
# more than 0.2 % of the steps on action states (sym134: every symbol re-arms BeginCapture; dotgap: every `a` does), or
# there is no expanded table (ascii124) -- then the per-lane form of the table's size.  A record of the routing at the
# time of writing, pinned so that a change of it is seen; either kernel is exact.
OWN_CHOICE = {"capture_kv": "ragged_capture", "capture_gap": "ragged_capture", "capture_alt40": "ragged_capture",
              "capture_rep": "ragged_capture", "capture_words150": "ragged_capture", "capture_sym134": "capture_dense",
              "capture_dotgap": "capture", "capture_ascii124": "capture_dense"}


def same(a, b):
    return all((x == y).all() for x, y in zip(a, b)) and (a[2] == ((a[3] >= 0) & (a[4] >= 0))).all()


def test_batches_are_not_vacuous():
    """On the CPU: under BEGIN|END every fixture's batch has captured and uncaptured strings, and the batches of the tables
    without a dense form end (before the EndMark step) in more distinct states than the ragged kernel has dense rows (255) -- so the expanded
    table's walk (state x pending action: at least as many distinct states) must leave the rows."""
    assert len(fixtures()) >= 8
    for case in fixtures():
        o = ob.OracleCountingScanner(H.load_blob(case["blob"]), 0)
        many = build_batch(case, 5)
        assert len(many) >= 5000
        idx, fin, cap, b, e = o.capture(*ob.pack_strings(many))
        assert 0 < cap.sum() < len(many), (case["name"], int(cap.sum()))
        assert 0 < fin.sum() < len(many), (case["name"], int(fin.sum()))
        if case["states"] > 255:
            idx = o.capture(*ob.pack_strings(many), flags=1)[0]       # (the EndMark step folds the end states together)
            assert len(set(idx.tolist())) > 255, (case["name"], len(set(idx.tolist())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", fixtures(), ids=lambda c: c["name"])
def test_every_form_on_every_shape(case, pa, cfg, cus):
    from pire_amd import binding as pb

    blob = H.load_blob(case["blob"])
    t, o = pa.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s, l = shape_of(case, t)
    many = build_batch(case, 5)
    n = len(many)
    text, offs = H.pack(many)
    reached = set()

    def run(want, flags, names, **config):
        cfg.set(ragged_act_always=0, no_ragged_act=0, counting_variant=0, capture_by_length=0, no_length_order=0)
        cfg.set(**config)
        got = t.capture(text, offs, flags=flags)
        k = pb.last_kernel()
        assert k in names, (case["name"], flags, config, k, names)
        assert same(got, want), (case["name"], flags, config, k)
        reached.add(k)
        return k

    for flags in FLAGS:
        want = o.capture(*ob.pack_strings(many), flags=flags)
        if flags == 3:
            assert 0 < want[2].sum() < n
        if flags == 1 and s > 255:
            assert len(set(want[0].tolist())) > 255      # more distinct (expanded) states than dense rows
        own = run(want, flags, with_ragged(s, l, n, False, cus=cus))             # the library's own choice
        print("%s flags=%d: the library's own choice is %s" % (case["name"], flags, own))
        assert own == OWN_CHOICE[case["name"]], (case["name"], flags, own)
        run(want, flags, with_ragged(s, l, n, True, cus=cus), ragged_act_always=1)
        for variant in (0, 1, 2):
            run(want, flags, {per_lane(s, variant=variant, n=n, cus=cus)}, no_ragged_act=1, counting_variant=variant)
        run(want, flags | pb.FLAG_GENERIC, {"capture"})
        run(want, flags | pb.FLAG_GENERIC, {"capture"}, no_ragged_act=1, counting_variant=2)
        # (below 32 768 strings the length order is not built: these two settings must change nothing)
        run(want, flags, {per_lane(s, n=n, cus=cus)}, no_ragged_act=1, capture_by_length=1)
        run(want, flags, {per_lane(s, variant=2, n=n, cus=cus)}, no_ragged_act=1, counting_variant=2, no_length_order=1)
    expect = {per_lane(s, variant=2), per_lane(s), "capture"} | ({"ragged_capture"} if l <= 127 else set())
    assert reached == expect, (case["name"], reached, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("case", fixtures(), ids=lambda c: c["name"])
def test_per_lane_forms_by_length(case, pa, cfg, cus):
    """From 32 768 strings on the per-lane kernels can take the strings by length class (capture_by_length; the row kernel
    by default, no_length_order switches it off): the same answers either way."""
    from pire_amd import binding as pb

    blob = H.load_blob(case["blob"])
    t, o = pa.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s, l = shape_of(case, t)
    many = build_batch(case, 6) * 7
    n = len(many)
    assert n >= 32768 and n % 1024 != 0
    text, offs = H.pack(many)
    for flags in (3, 0):
        want = o.capture(*ob.pack_strings(many), flags=flags)
        for config, extra, variant in ((dict(capture_by_length=1), 0, 0), (dict(capture_by_length=1), pb.FLAG_GENERIC, 0),
                                       (dict(counting_variant=2), 0, 2), (dict(counting_variant=2, no_length_order=1), 0, 2)):
            cfg.set(ragged_act_always=0, no_ragged_act=1, counting_variant=0, capture_by_length=0, no_length_order=0)
            cfg.set(**config)
            got = t.capture(text, offs, flags=flags | extra)
            assert pb.last_kernel() == per_lane(s, generic=bool(extra), variant=variant, n=n, cus=cus), (case["name"], config, pb.last_kernel())
            assert same(got, want), (case["name"], flags, config, extra)
    assert 0 < want[2].sum() < n


@pytest.mark.gpu
@pytest.mark.parametrize("case", fixtures(), ids=lambda c: c["name"])
def test_small_batches_and_block_tails(case, pa, cfg, cus):
    """n = 1, below / at / above the ragged kernel's threshold of 256, and n that is no multiple of the block sizes of the
    three per-lane launches (64-string waves of the row kernel, 256, 1024)."""
    from pire_amd import binding as pb

    blob = H.load_blob(case["blob"])
    t, o = pa.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s, l = shape_of(case, t)
    wit = [bytes.fromhex(h) for h in case["witnesses_hex"]]
    pool = build_batch(case, 7)
    for n in (1, 2, 63, 65, 255, 256, 257, 1000, 1025, 2049):
        many = [wit[0]] + pool[:n - 1] if n % 2 else pool[:n - 1] + [wit[-1]]
        assert len(many) == n
        text, offs = H.pack(many)
        for flags in FLAGS:
            want = o.capture(*ob.pack_strings(many), flags=flags)
            if flags == 3:
                assert want[2].sum() > 0      # the witness is there
            for config, extra, names in (
                    (dict(), 0, with_ragged(s, l, n, False, cus=cus)),
                    (dict(ragged_act_always=1), 0, with_ragged(s, l, n, True, cus=cus)),
                    (dict(no_ragged_act=1), 0, {per_lane(s, n=n, cus=cus)}),
                    (dict(no_ragged_act=1, counting_variant=2), 0, {per_lane(s, variant=2, n=n, cus=cus)}),
                    (dict(), pb.FLAG_GENERIC, {"capture"})):
                cfg.set(ragged_act_always=0, no_ragged_act=0, counting_variant=0)
                cfg.set(**config)
                got = t.capture(text, offs, flags=flags | extra)
                assert pb.last_kernel() in names, (case["name"], n, flags, config, pb.last_kernel(), names)
                assert same(got, want), (case["name"], n, flags, config, extra, pb.last_kernel())


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 17, 127])
@pytest.mark.parametrize("case", fixtures(), ids=lambda c: c["name"])
def test_device_pointers_at_any_alignment(case, shift, pa, cfg, cus):
    """Device text that starts `shift` bytes into a 128-byte line in a buffer that ends with the text, offsets on the
    device, outputs of exactly n elements; then the same with out_state_idx and out_final NULL."""
    import torch
    from pire_amd import binding as pb

    blob = H.load_blob(case["blob"])
    t, o = pa.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s, l = shape_of(case, t)
    many = build_batch(case, 20 + shift, n_noise=800)
    n = len(many)
    text, offs = ob.pack_strings(many)
    buf = torch.zeros(shift + len(text), dtype=torch.uint8, device="cuda")
    buf[shift:] = torch.as_tensor(np.asarray(text, dtype=np.uint8).copy())
    doffs = torch.as_tensor(np.asarray(offs, dtype=np.uint64).astype(np.int64), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for flags in FLAGS:
        want = o.capture(text, offs, flags=flags)
        for config, extra, names in (
                (dict(), 0, with_ragged(s, l, n, False, cus=cus)),
                (dict(ragged_act_always=1), 0, with_ragged(s, l, n, True, cus=cus)),
                (dict(no_ragged_act=1), 0, {per_lane(s, n=n, cus=cus)}),
                (dict(no_ragged_act=1, counting_variant=2), 0, {per_lane(s, variant=2, n=n, cus=cus)}),
                (dict(), pb.FLAG_GENERIC, {"capture"})):
            cfg.set(ragged_act_always=0, no_ragged_act=0, counting_variant=0)
            cfg.set(**config)
            for null_outputs in (False, True):
                idx = torch.full((n,), -5, dtype=torch.int32, device="cuda")
                fin = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
                bg = torch.full((n,), -77, dtype=torch.int64, device="cuda")
                en = torch.full((n,), -77, dtype=torch.int64, device="cuda")
                t.capture_device(buf.data_ptr() + shift, doffs.data_ptr(), n, flags | extra, 0 if null_outputs else idx.data_ptr(),
                                 0 if null_outputs else fin.data_ptr(), bg.data_ptr(), en.data_ptr(), stream)
                torch.cuda.synchronize()
                where = (case["name"], shift, flags, config, extra, null_outputs, pb.last_kernel())
                assert pb.last_kernel() in names, where
                assert (bg.cpu().numpy() == want[3]).all() and (en.cpu().numpy() == want[4]).all(), where
                if null_outputs:
                    assert (idx == -5).all() and (fin == 77).all(), where
                else:
                    assert (idx.cpu().numpy().astype(np.uint32) == want[0]).all() and (fin.cpu().numpy() == want[1]).all(), where
    assert 0 < want[2].sum() < n


def edge_case():
    return H.golden()["capturing_edge"][0]


def test_begin_mark_fixture_against_golden_and_reference():
    case = edge_case()
    blob = H.load_blob(case["blob"])
    strings = [bytes.fromhex(h) for h in case["strings_hex"]]
    idx, fin, cap, b, e = ob.OracleCountingScanner(blob, 0).capture(*ob.pack_strings(strings))
    assert (idx.tolist(), fin.tolist(), cap.tolist(), b.tolist(), e.tolist()) == (case["idx"], case["final"], case["captured"], case["begin"], case["end"])
    assert 0 in case["begin"]
    if ob.ref_available():
        check_oracle_against_reference(ob.RefCapturingScanner.load(blob), ob.OracleCountingScanner(blob, 0), strings * 3)


@pytest.mark.gpu
def test_begin_capture_on_the_begin_mark_step(pa, cfg, cus):
    """Regression (found by test_random_capture_all_kernels): `([ab].{5})*\\dc{2}` takes BeginCapture on the BeginMark step,
    and after a match nothing re-arms it, so begin = 0 is the answer.  capture_rows applied that pending action on the
    first step of the string's first 128-byte line -- a byte in front of the string unless the string starts a line --
    and reported begin = -(offset in the line) as a 32-bit number; the same for empty strings.  Every form, the matching
    strings at every offset of a line."""
    from pire_amd import binding as pb

    case = edge_case()
    blob = H.load_blob(case["blob"])
    t, o = pa.CountingTable(blob, 0), ob.OracleCountingScanner(blob, 0)
    s, l = t.Size, t.LettersCount
    assert s <= 34
    rng = np.random.RandomState(3)
    a = np.frombuffer(b"ab1cc x", dtype=np.uint8)
    many = [bytes.fromhex(h) for h in case["strings_hex"]]
    for k in range(300):
        many += [b"1cc" + b"x" * (k % 7), b"", b"7cc" + bytes(a[rng.randint(0, len(a), size=k)])][:1 + k % 3]
    many += [bytes(a[rng.randint(0, len(a), size=int(rng.randint(0, 200)))]) for _ in range(600)]
    n = len(many)
    text, offs = H.pack(many)
    for flags in FLAGS:
        want = o.capture(text, offs, flags=flags)
        if flags & 1:
            assert (want[3] == 0).sum() > 100
        for config, extra, names in (
                (dict(), 0, with_ragged(s, l, n, False, cus=cus)),
                (dict(ragged_act_always=1), 0, {"ragged_capture"}),
                (dict(no_ragged_act=1), 0, {"capture_dense"}),
                (dict(no_ragged_act=1, counting_variant=2), 0, {"capture_rows"}),
                (dict(), pb.FLAG_GENERIC, {"capture"})):
            cfg.set(ragged_act_always=0, no_ragged_act=0, counting_variant=0)
            cfg.set(**config)
            got = t.capture(text, offs, flags=flags | extra)
            assert pb.last_kernel() in names, (flags, config, pb.last_kernel())
            assert same(got, want), (flags, config, extra, pb.last_kernel())


# ---- drawn capturing scanners ----

# (regexp, strings it matches); no atom has parentheses of its own, so the one group is always number 1
ATOMS = [("a", ["a"]), ("b", ["b"]), ("c", ["c"]), ("ab", ["ab"]), ("ba", ["ba"]), ("abc", ["abc"]), ("[a-c]", ["a", "b", "c"]),
         ("[^a]", ["b", "x", "="]), (".", ["a", "q", " "]), ("\\d", ["0", "1"]), ("\\w", ["a", "Z", "0"]), ("\\s", [" ", "\t"]),
         ("x", ["x"]), ("[a-z]", ["d", "q", "y"]), ("[0-9a-f]", ["0", "f"]), ("q+", ["q", "qqq"]), ("=", ["="]), (";", [";"]),
         ("id", ["id"]), ("xy", ["xy"]), (".{3}", ["abc", "x=1"]), ("[a-c]{2,5}", ["ab", "cabca"]), ("\\w{0,6}", ["", "id0", "abcdef"]),
         ("a.{4}", ["axxxx", "aaaaa"]), ("b.{0,6}", ["b", "bab=1;"]), ("[ab].{5}", ["a12345", "bababa"]), ("x.{6}", ["xxxxxxx", "x123456"])]
QUANT = [("", 1, 1), ("", 1, 1), ("", 1, 1), ("*", 0, 3), ("+", 1, 3), ("?", 0, 1), ("{2}", 2, 2), ("{1,3}", 1, 3), ("{0,4}", 0, 4)]
SEED_BASE = 4500
SEEDS = 24


def draw_pattern(rng):
    """(pattern, capture index, a sampler of matching strings): two to six quantified atoms, a run of them inside the one
    group -- first, last or in the middle, the group itself under a quantifier or able to match the empty string."""
    k = int(rng.randint(2, 8))
    parts = []
    for _ in range(k):
        atom, samples = ATOMS[rng.randint(0, len(ATOMS))]
        q, lo, hi = QUANT[rng.randint(0, len(QUANT))]
        parts.append((atom + q, samples, lo, hi))
    g0 = int(rng.randint(0, k))
    g1 = int(rng.randint(g0 + 1, k + 1))
    gq, glo, ghi = [("", 1, 1), ("", 1, 1), ("*", 0, 2), ("+", 1, 2), ("?", 0, 1)][rng.randint(0, 5)]
    head = "^" if rng.randint(0, 4) == 0 else ""
    tail = "$" if rng.randint(0, 4) == 0 else ""
    pat = head + "".join(p[0] for p in parts[:g0]) + "(" + "".join(p[0] for p in parts[g0:g1]) + ")" + gq + "".join(p[0] for p in parts[g1:]) + tail

    def one(p, r):
        return "".join(p[1][r.randint(0, len(p[1]))] for _ in range(r.randint(p[2], p[3] + 1)))

    def sample(r):
        mid = "".join("".join(one(p, r) for p in parts[g0:g1]) for _ in range(r.randint(glo, ghi + 1)))
        return ("".join(one(p, r) for p in parts[:g0]) + mid + "".join(one(p, r) for p in parts[g1:])).encode("utf-8")

    return pat, 1, sample


def draw_scanner(seed):
    """The seed's scanner: (pattern, options, blob, sampler), or None when 20 draws gave nothing the reference compiles."""
    rng = np.random.RandomState(SEED_BASE + seed)
    opt = ["", "i", "u"][int(rng.randint(0, 3))]
    for _ in range(20):
        pat, index, sample = draw_pattern(rng)
        try:
            ref = ob.RefCapturingScanner.compile(pat.encode("utf-8"), index, opt)
        except ValueError:
            continue                      # not compilable (a byte the lexer refuses, a wrong range): draw again
        return pat, opt, ref, sample
    return None


def random_strings(rng, sample, n):
    a = np.frombuffer("abcdxyq01 f\t=;Zi".encode(), dtype=np.uint8)
    out = []
    for _ in range(n):
        out.append(b"".join(sample(rng) if rng.randint(0, 3) == 0 else bytes(a[rng.randint(0, len(a), size=int(rng.randint(0, 30)))])
                            for _ in range(rng.randint(0, 7))))
    return out + [b"", sample(rng), sample(rng) * 2, bytes(a[rng.randint(0, len(a), size=5000)]) + sample(rng)]


def check_oracle_against_reference(ref, o, strings):
    for flags in FLAGS:
        a, b = ref.run_strings(strings, flags=flags), o.capture(*ob.pack_strings(strings), flags=flags)
        assert all((x == y).all() for x, y in zip(a, b)), flags


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_capture_all_kernels(pa, seed, cfg, cus):
    if not ob.ref_available():
        pytest.skip("oracle/_ref not built")
    from pire_amd import binding as pb

    drawn = draw_scanner(seed)
    if drawn is None:
        pytest.skip("nothing compilable drawn")
    pat, opt, ref, sample = drawn
    blob = ref.save()
    o, t = ob.OracleCountingScanner(blob, 0), pa.CountingTable(blob, 0)
    s, l = t.Size, t.LettersCount
    assert (s, l) == (o.size, o.letters) and s == ref.size
    rng = np.random.RandomState(9000 + seed)
    many = random_strings(rng, sample, 1500)
    n = len(many)
    check_oracle_against_reference(ref, o, many)
    text, offs = H.pack(many)
    for flags in FLAGS:
        want = o.capture(text, offs, flags=flags)
        for config, extra, names in (
                (dict(), 0, with_ragged(s, l, n, False, cus=cus)),
                (dict(ragged_act_always=1), 0, with_ragged(s, l, n, True, cus=cus)),
                (dict(no_ragged_act=1), 0, {per_lane(s, n=n, cus=cus)}),
                (dict(no_ragged_act=1, counting_variant=2), 0, {per_lane(s, variant=2, n=n, cus=cus)}),
                (dict(), pb.FLAG_GENERIC, {"capture"})):
            cfg.set(ragged_act_always=0, no_ragged_act=0, counting_variant=0)
            cfg.set(**config)
            got = t.capture(text, offs, flags=flags | extra)
            assert pb.last_kernel() in names, (pat, opt, flags, config, pb.last_kernel(), names)
            assert same(got, want), (pat, opt, s, l, flags, config, extra, pb.last_kernel())


def test_random_capture_draws_cover_the_classes():
    """The draw on the CPU: at most 3 of the seeds give nothing compilable, both classes of dense tables occur (<= 34
    states: capture_rows; 35..255: capture_dense alone), the samplers do produce captured strings, and the oracle
    equals the reference on every drawn scanner."""
    if not ob.ref_available():
        pytest.skip("oracle/_ref not built")
    sizes, nothing, captured = [], 0, 0
    for seed in range(SEEDS):
        drawn = draw_scanner(seed)
        if drawn is None:
            nothing += 1
            continue
        pat, opt, ref, sample = drawn
        o = ob.OracleCountingScanner(ref.save(), 0)
        many = random_strings(np.random.RandomState(9000 + seed), sample, 1500)
        check_oracle_against_reference(ref, o, many)
        cap = o.capture(*ob.pack_strings(many))[2]
        captured += 0 < cap.sum() < len(many)
        sizes.append(ref.size)
    assert nothing <= 3, nothing
    assert any(s <= 34 for s in sizes) and any(34 < s <= 255 for s in sizes), sizes
    # (a group under `*` or `?` that the reference never reports, `(q*)` that it reports in every string: such draws are
    # kept, they are scanners like any other -- but at least half of the batches must have both kinds of strings)
    assert captured >= SEEDS // 2, (captured, len(sizes))
