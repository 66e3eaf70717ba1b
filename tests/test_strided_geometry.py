"""Fixed-length records whose stride is not their length (pire_hip_run_strided and what stands behind it).

String i of a strided batch is text[i * stride, i * stride + len).  Every fixed-length kernel does its own arithmetic on the
stride -- the tiled kernel's tile bases, its byte-wise tail and the remainder behind it, the class-indexed walk, the generic
kernel, the three SlowScanner kernels, the segmented scan's cut, the host-pointer chunking -- and nearly every other test of
the suite passes stride == len at the start of a fresh allocation.  Here the records are PADDED, and the padding is poison:
a kernel that walks on into it, takes the next record from i * len, or cuts the remainder at the wrong byte ends in another
state (the CPU test of the batch builder pins that both mistakes change the answers of at least a quarter of the records).

Every expected value is the oracle's on a compact copy of the records (data[:, :len] made contiguous), every comparison is
exact, and every case asserts which kernel ran."""
import numpy as np
import pytest

from oracle import binding as ob
from pire_amd import workloads as W
from tests import helpers as H
from tests.test_gpu_parity import expected_counts, pa, torch_cuda  # noqa: F401  (fixtures)
from tests.test_wide import records_of

BE = ob.FLAG_BEGIN | ob.FLAG_END
SETS = ["set_a", "set_d", "c2_single"]
LENGTHS = [128, 256, 384, 1000, 4096 + 48]
COUNTS = [64, 64 * 9 + 3, 64 * 40 + 17]
WIDE_LENGTHS = [256, 384, 1000]


def r16(x):
    return (x + 15) // 16 * 16


def tiled_strides(length):
    return [r16(length), r16(length) + 16, r16(length) + 16 * 7, r16(length) + 4096]


def wide_strides(length):
    return [r16(length), r16(length) + 16 * 7]


# ------------------------------------------------------------------------------------------------ the batch builder (CPU)

def entry_of(name):
    return W.wide_set(name) if name == "dict_1k" else [b for b in H.big_sets() if b["name"] == name][0]


def blob_of(entry):
    return W.load_blob(entry["blob"]) if "words_file" in entry else H.load_blob(entry["blob"])


def witness_of(entry):
    """A planted match text of the table: the dictionary's word 11 (as tests/test_pair_seg_tails.py takes it: the Surround()ed
    scanner is absorbed in its Final state by it), the glued sets' first witness ("hello  world" for /hello\\s+w.+d$/, which
    set_a, set_d and c2_single share: a match only where the text ENDS with it)."""
    if "words_file" in entry:
        return W.dictionary_words(entry)[11]
    return bytes.fromhex(entry["witnesses_hex"][0])


def straddled(n):
    """Every second record: 4k and 4k + 3 (c2_single's corpus ends records 4k + 1 and 4k + 2 with a match; they keep it, so
    that half of that table's right answers are Final and a record read from the wrong place shows)."""
    i = np.arange(n) % 4
    return (i == 0) | (i == 3)


def padded_records(entry, n, length, stride, seed):
    """u8[n, stride].  Columns [0, length): the table's own corpus.  Columns [length, stride): 0xFF and then the whole witness,
    ending with the padding (where the padding is shorter than the witness: the witness's last bytes).  In every second record
    the witness also straddles the record's end: its first part are the record's last bytes, the rest the padding's first."""
    assert stride >= length
    w = np.frombuffer(witness_of(entry), dtype=np.uint8)
    out = np.full((n, stride), 0xFF, dtype=np.uint8)
    if "words_file" in entry:
        out[:, :length] = records_of(entry, "k128", seed, n, length)
    else:
        out[:, :length] = ob.corpus_fill(seed, 0, n, length, H.plants_for(entry), threads=4)
    pad = stride - length
    if pad == 0:
        return out
    out[:, length:] = np.concatenate([np.full(pad, 0xFF, dtype=np.uint8), w])[-pad:]
    rest = min(pad, len(w) // 2)
    out[straddled(n), length - (len(w) - rest):length + rest] = w
    return out


def compact(data, length):
    n = data.shape[0]
    return np.ascontiguousarray(data[:, :length]).reshape(-1), np.arange(n + 1, dtype=np.uint64) * length


def want_of(o, data, length, flags=BE, init=None):
    text, offs = compact(data, length)
    return o.run(text, offs, flags=flags, init_idx=init, threads=4)


@pytest.mark.parametrize("name", SETS + ["dict_1k"])
def test_padding_is_poison_for_both_wrong_readings(name):
    """The builder's sensitivity, on the oracle alone.  For every (len, stride) of the GPU cases below with stride > len, and
    BEGIN | END: the end states of (A) every record taken as `stride` bytes long and of (B) record i taken from i * len of
    the padded buffer ("len for stride") differ from the right ones in at least a quarter of the records.

    Shares of the records whose end state changes, minimum .. maximum over the shapes (n = 579):
        set_a      A 0.89 .. 0.94   B 0.46 .. 0.53
        set_d      A 0.50 .. 0.94   B 0.72 .. 0.91
        c2_single  A 0.50 .. 0.50   B 0.47 .. 0.55
        dict_1k    A 0.50 .. 1.00   B 0.49 .. 0.93
    (A is a half where the padding is 8 bytes -- len 1000, stride 1008: only the straddling witnesses fit -- and for
    c2_single, whose other records end with a match of the one pattern either way.)"""
    entry = entry_of(name)
    o = ob.OracleScanner(blob_of(entry))
    n = 64 * 9 + 3
    shapes = [(ln, st) for ln in (WIDE_LENGTHS if name == "dict_1k" else LENGTHS)
              for st in (wide_strides(ln) if name == "dict_1k" else tiled_strides(ln)) if st > ln]
    shapes += [(384, 400), (384, 464)]          # the alignment, hit-pass and host cases
    shares = []
    for length, stride in shapes:
        data = padded_records(entry, n, length, stride, n * 31 + length)
        ri, _ = want_of(o, data, length)
        ai, _ = o.run(data.reshape(-1), np.arange(n + 1, dtype=np.uint64) * stride, threads=4)
        bi, _ = o.run(data.reshape(-1), np.arange(n + 1, dtype=np.uint64) * length, threads=4)
        a, b = float((ai != ri).mean()), float((bi != ri).mean())
        shares.append((length, stride, round(a, 2), round(b, 2)))
        assert a >= 0.25 and b >= 0.25, (name, length, stride, a, b)
    print(name, "A %.2f .. %.2f  B %.2f .. %.2f" % (min(s[2] for s in shares), max(s[2] for s in shares),
                                                     min(s[3] for s in shares), max(s[3] for s in shares)))


def test_padded_records_keep_the_corpus_and_end_with_the_witness():
    entry = entry_of("set_a")
    w = witness_of(entry)
    d = padded_records(entry, 8, 256, 256 + 112, 5)
    plain = ob.corpus_fill(5, 0, 8, 256, H.plants_for(entry))
    assert (d[~straddled(8), :256] == plain[~straddled(8)]).all() and (d[:, :250] == plain[:, :250]).all()
    assert all(bytes(r[-len(w):]) == w for r in d) and (d[1, 256:256 + 112 - len(w)] == 0xFF).all()
    assert bytes(d[0, 250:262]) == w and bytes(d[3, 250:262]) == w and bytes(d[1, 250:262]) != w
    assert (padded_records(entry, 8, 256, 256, 5) == plain).all()
    assert bytes(padded_records(entry, 4, 1000, 1008, 5)[0, 994:]) == b"hello  worldld"


# ------------------------------------------------------------------------------------------------ device side

class _Out:
    """Outputs of one launch, poisoned before it; the counters start from non-zero values (they are accumulated into)."""

    def __init__(self, torch, t, n):
        self.torch, self.n = torch, n
        self.idx = torch.full((n,), -2, dtype=torch.int32, device="cuda")
        self.fin = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        self.base = np.arange(t.RegexpsCount + 2, dtype=np.int64) * 3 + 5
        self.cnt = torch.as_tensor(self.base, device="cuda")

    def get(self):
        self.torch.cuda.synchronize()
        return (self.idx.cpu().numpy().astype(np.uint32), self.fin.cpu().numpy(),
                (self.cnt.cpu().numpy() - self.base).astype(np.uint64))


def run_at(torch, t, ptr, n, length, stride, flags=BE, init=None, generic=False):
    """pire_hip_run_strided on device memory at `ptr`: numpy idx, final, counts (what the call added)."""
    from pire_amd import binding as pb

    out = _Out(torch, t, n)
    init_t = None if init is None else torch.as_tensor(np.asarray(init).astype(np.int32), device="cuda")
    t.run_strided_device(ptr, n, length, stride, flags | (pb.FLAG_GENERIC if generic else 0), out.idx.data_ptr(),
                         out.fin.data_ptr(), out.cnt.data_ptr(), init_t.data_ptr() if init_t is not None else 0,
                         torch.cuda.current_stream().cuda_stream)
    return out.get()


def same(got, o, oi, of, what=None):
    gi, gf, cnt = got
    bad = np.nonzero((gi != oi) | (gf != of))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10].tolist(), gi[bad[:5]].tolist(), oi[bad[:5]].tolist())
    assert (cnt == expected_counts(o, oi, of)).all(), what


def table_and_oracle(pa, name):
    entry = entry_of(name)
    blob = blob_of(entry)
    return entry, pa.Table(blob), ob.OracleScanner(blob)


# ------------------------------------------------------------------------------------------------ 1. tiled, stride > len

@pytest.mark.gpu
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("name", SETS)
def test_tiled_kernel_with_padded_records(pa, torch_cuda, name, length):
    """ScanTiledKernel and the generic remainder behind it: one whole task, nine and a remainder of 3, forty and one of 17; odd
    and even tile counts; tails of 0, 104 and 48 bytes behind the last tile; padding of 0 (stride == len, where len is a
    multiple of 16) to 4 096 + 8 bytes.  len 1000 with stride 1008 is the tiled kernel's: TiledEligible asks nothing of
    len % 16, and the byte-wise tail walks the 104 bytes.
    (A wave of this kernel takes a second task -- the chained prefetch -- only from 16 tasks per CU on: 262 144 records on 256
    CUs, more than a padded test batch may hold; tests/test_wide.py::test_early_out_between_chained_tasks has that with
    stride == len.)"""
    from pire_amd import binding as pb

    entry, t, o = table_and_oracle(pa, name)
    for stride in tiled_strides(length):
        for n in COUNTS:
            data = padded_records(entry, n, length, stride, n * 31 + length)
            oi, of = want_of(o, data, length)
            d = torch_cuda.as_tensor(data, device="cuda")
            got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
            assert pb.last_kernel() == "tiled" and pb.last_kernel_symbol().endswith("<16,2,nt,5>"), \
                (length, stride, n, pb.last_kernel(), pb.last_kernel_symbol())
            same(got, o, oi, of, (name, length, stride, n))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_tiled_kernel_with_padded_records_flags_and_resume_states(pa, torch_cuda, name):
    """Begin / End optional and a start state of its own for every record, on len 1000 in a stride of 1120."""
    from pire_amd import binding as pb

    entry, t, o = table_and_oracle(pa, name)
    n, length, stride = 64 * 9 + 3, 1000, 1000 + 8 + 16 * 7
    data = padded_records(entry, n, length, stride, 77)
    d = torch_cuda.as_tensor(data, device="cuda")
    init = np.random.RandomState(5).randint(0, o.size, size=n).astype(np.uint32)
    for flags in (0, ob.FLAG_BEGIN, ob.FLAG_END, BE):
        for ini in (None, init):
            oi, of = want_of(o, data, length, flags, ini)
            got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride, flags=flags, init=ini)
            assert pb.last_kernel() == "tiled"
            same(got, o, oi, of, (name, flags, ini is not None))


# ------------------------------------------------------------------------------------------------ 2. every tiled variant

VARIANTS = [(0, "<16,2,nt,5>"), (1, "<16,2,nt,5,rot>"), (2, "<16,2,plain,5>"), (20, "<16,2,nt,5,free-running>"),
            (22, "<16,2,nt,4,shadow>"), (23, "<16,2,nt,5,rotated columns>"), (24, "<16,2,nt,5>"),
            ("checked", "<16,2,nt,5,checked>")]

_VARIANT_BATCHES = {}


def _variant_batches(o, entry):
    """set_d with raw bytes in a third of the records (the walk leaves the dense rows), shared by the variants."""
    if not _VARIANT_BATCHES:
        rng = np.random.RandomState(23)
        for n, length, stride in ((64 * 9 + 3, 1024, 1024), (256, 128 * 3 + 16, 128 * 3 + 80), (64, 1000, 1008)):
            data = padded_records(entry, n, length, stride, n + length)
            k = rng.randint(0, n, size=n // 3)
            data[k, :length // 2] = rng.randint(0, 256, size=(len(k), length // 2), dtype=np.uint8)
            _VARIANT_BATCHES[(n, length, stride)] = (data,) + tuple(want_of(o, data, length))
    return _VARIANT_BATCHES


@pytest.mark.gpu
@pytest.mark.parametrize("variant,symbol", VARIANTS, ids=[str(v[0]) for v in VARIANTS])
def test_every_tiled_variant_gives_the_oracles_answers(pa, torch_cuda, cfg, variant, symbol):
    """pire_hip_config.tiled_variant is public: 1 (rows 260 bytes apart), 2 (no `nt`), 20 (waves not kept in step), 22 (the
    transpose hidden in the walk), 23 / 24 and the checked build "give the same results" -- on text that leaves the dense rows,
    with padded records and a tail that is no multiple of 16."""
    from pire_amd import binding as pb

    entry, t, o = table_and_oracle(pa, "set_d")
    if variant == "checked":
        cfg.set(checked=1)
    else:
        cfg.set(tiled_variant=variant)
    for (n, length, stride), (data, oi, of) in _variant_batches(o, entry).items():
        d = torch_cuda.as_tensor(data, device="cuda")
        got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
        assert pb.last_kernel() == "tiled" and pb.last_kernel_symbol() == "pirehip::ScanTiledKernel" + symbol, pb.last_kernel_symbol()
        same(got, o, oi, of, (variant, n, length, stride))
    if variant == "checked":
        assert t.check_failures() == 0


# ------------------------------------------------------------------------------------------------ 3. alignment of the text

@pytest.mark.gpu
def test_text_pointer_alignment_chooses_the_kernel_not_the_answers(pa, torch_cuda):
    """One device buffer, the batch at byte 16, 48, 112 and 144 of it (16-byte aligned, tile lines straddle 128-byte lines:
    tiled) and at byte 1, 8 and 17 (generic)."""
    from pire_amd import binding as pb

    torch = torch_cuda
    entry, t, o = table_and_oracle(pa, "set_a")
    n, length, stride = 64 * 5 + 1, 384, 400
    data = padded_records(entry, n, length, stride, 11)
    oi, of = want_of(o, data, length)
    src = torch.as_tensor(data.reshape(-1), device="cuda")
    buf = torch.full((n * stride + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 128 == 0
    for off, kernel in ((0, "tiled"), (16, "tiled"), (48, "tiled"), (112, "tiled"), (128 + 16, "tiled"), (1, "generic"),
                        (8, "generic"), (17, "generic")):
        buf.fill_(0xFF)
        buf[off:off + n * stride].copy_(src)
        got = run_at(torch, t, buf.data_ptr() + off, n, length, stride)
        assert pb.last_kernel() == kernel, (off, pb.last_kernel())
        same(got, o, oi, of, off)


@pytest.mark.gpu
@pytest.mark.parametrize("n,length,stride", [(64 * 5 + 1, 1000, 1001), (63, 384, 400), (64 * 5 + 1, 127, 128)],
                         ids=["stride 1001", "63 records", "len 127"])
def test_shapes_outside_the_tiled_contract_take_the_generic_kernel(pa, torch_cuda, n, length, stride):
    """A stride that is no multiple of 16, fewer than 64 records, a record shorter than a tile: generic, same answers."""
    from pire_amd import binding as pb

    entry, t, o = table_and_oracle(pa, "set_a")
    data = padded_records(entry, n, length, stride, 12)
    oi, of = want_of(o, data, length)
    d = torch_cuda.as_tensor(data, device="cuda")
    got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
    assert pb.last_kernel() == "generic"
    same(got, o, oi, of)


# ------------------------------------------------------------------------------------------------ 4. the 2^31 limit

@pytest.mark.gpu
def test_strides_at_the_limit_of_the_32_bit_tile_offset(pa, torch_cuda):
    """The tiled kernel's per-lane offset is a 32-bit register: TiledEligible asks 64 * stride < 2^31.  stride = 2^25 - 16 is
    the largest it takes (64 * stride = 2^31 - 1024; lane 56's offset is 56 * stride + 112, the second task's base lies 2 GiB
    into the buffer), stride = 2^25 goes to the generic kernel.  Two tasks of 64 records of 256 bytes in 4.3 GB."""
    from pire_amd import binding as pb

    torch = torch_cuda
    entry, t, o = table_and_oracle(pa, "set_a")
    n, length, width = 128, 256, 256 + 16 * 7
    data = padded_records(entry, n, length, width, 13)
    oi, of = want_of(o, data, length)
    src = torch.as_tensor(data, device="cuda")
    buf = torch.zeros(n << 25, dtype=torch.uint8, device="cuda")
    try:
        for stride, kernel in (((1 << 25) - 16, "tiled"), (1 << 25, "generic")):
            assert (n - 1) * stride + width <= buf.numel()
            torch.as_strided(buf, (n, width), (stride, 1)).copy_(src)
            got = run_at(torch, t, buf.data_ptr(), n, length, stride)
            assert pb.last_kernel() == kernel, (stride, pb.last_kernel())
            same(got, o, oi, of, stride)
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 5. the class-indexed walk

@pytest.mark.gpu
@pytest.mark.parametrize("length", WIDE_LENGTHS)
@pytest.mark.parametrize("walk,zipv", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_wide_walk_with_padded_records(pa, torch_cuda, cfg, walk, zipv, length):
    """wide.hip, one and two strings per lane, plain and zipped rows: three tasks of 64, and 454 records -- a remainder of 6
    behind seven tasks of 64, of 70 (more than a task of the other form) behind three tasks of 128."""
    from pire_amd import binding as pb

    cfg.set(walk_variant=walk, zip_variant=zipv)
    entry, t, o = table_and_oracle(pa, "dict_1k")
    for stride in wide_strides(length):
        for n in (64 * 3, 128 * 3 + 70):
            data = padded_records(entry, n, length, stride, n * 7 + length)
            oi, of = want_of(o, data, length)
            d = torch_cuda.as_tensor(data, device="cuda")
            got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
            sym = pb.last_kernel_symbol()
            assert pb.last_kernel() == "wide" and ("ScanWide2Kernel" if walk == 3 else "ScanWideKernel<") in sym and \
                ("zipped" in sym) == (zipv == 2), (pb.last_kernel(), sym)
            same(got, o, oi, of, (walk, zipv, length, stride, n))


@pytest.mark.gpu
@pytest.mark.parametrize("length,stride", [(128, 240), (200, 208), (255, 256)])
def test_wide_tables_keep_the_dense_rows_below_two_tiles(pa, torch_cuda, cfg, length, stride):
    """len 128 .. 255 with a table on the class-indexed walk: tiled (Dispatch asks len >= 256 of the wide walk)."""
    from pire_amd import binding as pb

    cfg.set(walk_variant=2)
    entry, t, o = table_and_oracle(pa, "dict_1k")
    n = 64 * 3 + 5
    data = padded_records(entry, n, length, stride, 3)
    oi, of = want_of(o, data, length)
    d = torch_cuda.as_tensor(data, device="cuda")
    got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
    assert pb.last_kernel() == "tiled"
    same(got, o, oi, of)


# ------------------------------------------------------------------------------------------------ 6. the segmented scan

def segmented_eligible(n, total):
    """segmented.hip SegmentedEligible under the default configuration."""
    if n == 0 or n >= 1 << 20:
        return False
    mean = total / n
    if mean < 8192.0:
        return False
    plain = np.ceil(n / (256.0 * 1024.0)) * mean / 25e6
    return plain > 1.5 * (total / 2.0e12 + 80e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [5000 + 8, 8192, 65536 + 40])
@pytest.mark.parametrize("n", [1, 3, 64])
@pytest.mark.parametrize("name", ["set_a", "set_d"])
def test_segmented_scan_of_padded_records(pa, torch_cuda, cfg, name, n, length):
    """Few long records with padding between them: the segmented scan cuts record i at i * stride + k * segment (for n > 1
    nothing of it lies on the grid of the tiled pass: segmented.hip asks stride == len for that) and must end every record
    at its len.  The table's witnesses straddle every multiple of 1 024 bytes (the segment ends) as well as the record's end.
    Once as the library routes it by itself (SegmentedEligible's own formula says which kernel that is), once with
    segment_bytes = 1024, and against PIRE_HIP_RUN_GENERIC on the same buffer."""
    from pire_amd import binding as pb

    entry, t, o = table_and_oracle(pa, name)
    ws = [np.frombuffer(bytes.fromhex(h), dtype=np.uint8) for h in entry["witnesses_hex"] if len(h) >= 8]
    for stride in (r16(length) + 16, r16(length) + 4096 + 48):
        data = padded_records(entry, n, length, stride, n + length)
        for j, cut in enumerate(range(1024, length - 32, 1024)):
            w = ws[j % len(ws)]
            data[j % 2::2, cut - len(w) // 2:cut - len(w) // 2 + len(w)] = w
        oi, of = want_of(o, data, length)
        d = torch_cuda.as_tensor(data, device="cuda")
        by_itself = "segmented" if segmented_eligible(n, n * length) else "tiled" if n >= 64 else "generic"
        got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
        assert pb.last_kernel().startswith(by_itself), (n, length, stride, pb.last_kernel())
        same(got, o, oi, of, ("default", n, length, stride))
        cfg.set(segment_bytes=1024)
        got = run_at(torch_cuda, t, d.data_ptr(), n, length, stride)
        assert pb.last_kernel().startswith("segmented"), (n, length, stride, pb.last_kernel())
        same(got, o, oi, of, ("segment_bytes", n, length, stride))
        gen = run_at(torch_cuda, t, d.data_ptr(), n, length, stride, generic=True)
        assert pb.last_kernel() == "generic"
        same(gen, o, oi, of, ("generic", n, length, stride))
        cfg.unset("segment_bytes")


# ------------------------------------------------------------------------------------------------ 7. SlowScanner

def _slow_case(name):
    return W.slow_case(name)


@pytest.mark.gpu
@pytest.mark.parametrize("no_list", [0, 1])
@pytest.mark.parametrize("name", ["slow_x40_utf8", "slow_x300"])
def test_slow_scanner_with_an_odd_stride(pa, torch_cuda, cfg, name, no_list):
    """3 000 records of 200 bytes, 213 bytes apart (the slow kernels ask no alignment).  /x.{40}$/: an x 41 bytes in front of
    the record's end in every third record (a match), 41 bytes in front of the STRIDE's end in the others (a match only for a
    kernel that walks on into the padding); /x.{300}$/ never matches 200 bytes, its state sets say where every x was."""
    import pire_amd
    from pire_amd import binding as pb

    torch = torch_cuda
    cfg.set(slow_no_list=no_list)
    blob = H.load_blob(_slow_case(name)["blob"])
    t, o = pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)
    n, length, stride = 3000, 200, 200 + 13
    rng = np.random.RandomState(3)
    data = rng.choice(np.frombuffer(b"yzw abc", dtype=np.uint8), size=(n, stride)).astype(np.uint8)
    data[rng.randint(0, n, size=n), rng.randint(0, stride, size=n)] = ord("x")
    third = np.arange(n) % 3 == 0
    data[third, length - 41] = ord("x")
    data[~third, stride - 41] = ord("x")
    text, offs = compact(data, length)
    of, obits = o.run(text, offs)
    if name == "slow_x40_utf8":
        assert of[third].all() and of.sum() < n // 2
        assert o.run(data.reshape(-1), np.arange(n + 1, dtype=np.uint64) * stride)[0][~third].all()   # the padding is poison
    d = torch.as_tensor(data, device="cuda")
    fin = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    bits = torch.full((n, t.words), -2, dtype=torch.int32, device="cuda")
    cnt = torch.as_tensor(np.array([7, 11], dtype=np.int64), device="cuda")
    t.run_strided_device(d.data_ptr(), n, length, stride, BE, fin.data_ptr(), bits.data_ptr(), cnt.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert pb.last_kernel() == ("slow_list" if not no_list else "slow" if o.size <= 256 else "slow_wide"), pb.last_kernel()
    assert (fin.cpu().numpy() == of).all()
    assert (bits.cpu().numpy().view(np.uint32) == obits).all()
    assert cnt.cpu().numpy().tolist() == [7 + int(of.sum()), 11 + n]


# ------------------------------------------------------------------------------------------------ 8. the hit passes

@pytest.mark.gpu
def test_select_and_route_pass_the_stride_on(pa, torch_cuda):
    """pire_hip_run_select_strided and pire_hip_run_route_strided are wrappers of the scan: 579 records of 384 bytes in a
    stride of 464, the hit lists against the oracle's end states."""
    from pire_amd import binding as pb

    torch = torch_cuda
    entry, t, o = table_and_oracle(pa, "set_a")
    n, length, stride = 64 * 9 + 3, 384, 464
    data = padded_records(entry, n, length, stride, 21)
    oi, of = want_of(o, data, length)
    d = torch.as_tensor(data, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out = _Out(torch, t, n)
    hits = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    t.run_select_strided_device(d.data_ptr(), n, length, stride, BE, count.data_ptr(), out_hits_ptr=hits.data_ptr(), hit_cap=n,
                                out_idx_ptr=out.idx.data_ptr(), out_final_ptr=out.fin.data_ptr(), out_counts_ptr=out.cnt.data_ptr(),
                                stream=stream)
    same(out.get(), o, oi, of, "select")
    assert pb.last_kernel() == "tiled"
    want = np.nonzero(of)[0]
    assert 0 < len(want) < n and int(count.item()) == len(want)
    assert hits.cpu().numpy()[:len(want)].tolist() == want.tolist() and (hits.cpu().numpy()[len(want):] == -1).all()
    regexps = t.RegexpsCount
    out = _Out(torch, t, n)
    rows = torch.full((regexps, n), -1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(regexps, dtype=torch.int64, device="cuda")
    t.run_route_strided_device(d.data_ptr(), n, length, stride, BE, counts.data_ptr(), out_hits_ptr=rows.data_ptr(), hit_cap=n,
                               out_idx_ptr=out.idx.data_ptr(), out_final_ptr=out.fin.data_ptr(), out_counts_ptr=out.cnt.data_ptr(),
                               stream=stream)
    same(out.get(), o, oi, of, "route")
    assert pb.last_kernel() == "tiled"
    accepted = {s: set(o.accepted(s)) for s in set(oi.tolist())}
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    for r in range(regexps):
        want = [i for i in range(n) if r in accepted[int(oi[i])]]
        assert int(counts[r]) == len(want) and rows[r, :len(want)].tolist() == want and (rows[r, len(want):] == -1).all(), r
    assert counts.sum() > 0


# ------------------------------------------------------------------------------------------------ 9. host pointers

def run_host(t, data, length, flags=BE):
    """pire_hip_run_strided on a host buffer that ends with the last record's len: idx, final, what the call added to counts."""
    from pire_amd import binding as pb

    n, stride = data.shape
    buf = data.reshape(-1)[:(n - 1) * stride + length].copy()
    idx = np.full(n, 0xFFFFFFFE, dtype=np.uint32)
    fin = np.full(n, 9, dtype=np.uint8)
    base = np.arange(t.RegexpsCount + 2, dtype=np.uint64) * 3 + 5
    cnt = base.copy()
    pb._check(pb.lib().pire_hip_run_strided(t._h, buf.ctypes.data, n, length, stride, flags, None, idx.ctypes.data,
                                            fin.ctypes.data, cnt.ctypes.data, None))
    return idx, fin, cnt - base


HOST_CASES = [
    # table, n, len, stride, configuration, kernel
    ("set_a", 163 * 6, 384, 400, {}, "tiled"),                 # 65 536 // 400 = 163 records a chunk: six chunks
    ("set_a", 163 * 6 + 100, 384, 400, {}, "tiled"),           # seven, the last of 100 records
    ("set_a", 320, 1000, 1040, {}, "tiled"),                   # stride > chunk / 64: staged in one piece
    ("set_a", 1000, 384, 400, {"host_one_shot": 1}, "tiled"),
    ("dict_1k", 132 * 6, 384, 496, {"walk_variant": 2}, "wide"),   # 132 records a chunk
    ("dict_1k", 132 * 6 + 70, 384, 496, {"walk_variant": 2}, "wide"),
    ("dict_1k", 300, 1000, 1120, {"walk_variant": 2}, "wide"),
    ("dict_1k", 800, 384, 496, {"walk_variant": 2, "host_one_shot": 1}, "wide"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,length,stride,knobs,kernel", HOST_CASES,
                         ids=["%s-%d-%d-%d%s" % (c[0], c[1], c[2], c[3], "-one shot" if "host_one_shot" in c[4] else "") for c in HOST_CASES])
def test_host_pointer_batches_with_padded_records(pa, cfg, name, n, length, stride, knobs, kernel):
    """The host-pointer form cuts the batch into chunks of whole records by the stride (api.cpp RunHostPipelined: chunk
    c is bytes [f * stride, (f + cnt - 1) * stride + len)), an even and an odd number of them; a stride too large for 64
    records a chunk and host_one_shot take the one-piece staging.  The caller's buffer ends with the last record."""
    from pire_amd import binding as pb

    cfg.set(host_chunk_bytes=65536, **knobs)
    entry, t, o = table_and_oracle(pa, name)
    data = padded_records(entry, n, length, stride, n + 1)
    assert (n - 1) * stride + length > 300 * 1024          # not the small-call arena
    oi, of = want_of(o, data, length)
    got = run_host(t, data, length)
    assert pb.last_kernel() == kernel, pb.last_kernel()
    same(got, o, oi, of, (name, n, length, stride))
