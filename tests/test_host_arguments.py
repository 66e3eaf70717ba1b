"""The batch entry points take their arrays from the host or (PIRE_HIP_RUN_ON_DEVICE) from the device, through one path
(internal.h BatchIO): what a host-pointer call refuses, and that both forms of a call give the oracle's answer under every
pire_hip_config.host_staging mode.

The entry points: pire_hip_run, pire_hip_run_half_final, pire_hip_prefix, pire_hip_suffix, pire_hip_counting_run,
pire_hip_capture_run and pire_hip_slow_run; pire_hip_run / pire_hip_run_half_final also with resident text and host
offsets (ON_DEVICE | HOST_OFFSETS)."""
import numpy as np
import pytest

from oracle import binding as ob
from tests import helpers as H

pytestmark = pytest.mark.gpu

BE = ob.FLAG_BEGIN | ob.FLAG_END
EINVAL = -1   # include/pire_hip.h PIRE_HIP_EINVAL
ALPHABET = b"abcdeaxHeadInnerTailhello wd0123456789 xxx=/'\"google_id"


def _golden(section, name):
    return [c for c in H.golden()[section] if c["name"] == name][0]


class Entry:
    """One entry point on one golden table: call(text_ptr, offsets_ptr, n, flags, out_ptrs) is the C call; outs(n) the
    (dtype, shape) of its result arrays, in the order of the C arguments; oracle(text, offsets) the same arrays."""

    def __init__(self, name, call, outs, oracle, host_offsets=False):
        self.name, self.call, self.outs, self.oracle, self.host_offsets = name, call, outs, oracle, host_offsets


def entries():
    import pire_amd
    from pire_amd import binding as pb

    L = pb.lib()
    blob = H.load_blob(_golden("big", "set_d")["blob"])
    t, o = pire_amd.Table(blob), ob.OracleScanner(blob)
    R = t.RegexpsCount
    cc = _golden("counting", "count2_basic")
    cblob = H.load_blob(cc["blob"])
    ct, co = pire_amd.CountingTable(cblob, cc["kind"]), ob.OracleCountingScanner(cblob, cc["kind"])
    kblob = H.load_blob(_golden("capturing", "capture_digits")["blob"])
    kt, ko = pire_amd.CountingTable(kblob, 0), ob.OracleCountingScanner(kblob, 0)
    sblob = H.load_blob(_golden("slow", "slow_alt")["blob"])
    st, so = pire_amd.SlowTable(sblob), ob.OracleSlowScanner(sblob)

    def capture_oracle(text, offs):
        idx, fin, _, b, e = ko.capture(text, offs)
        return idx, fin, b, e

    return [
        Entry("run", lambda tx, of, n, fl, p: L.pire_hip_run(t._h, tx, of, n, BE | fl, None, p[0], p[1], None, None),
              lambda n: [(np.uint32, (n,)), (np.uint8, (n,))], lambda text, offs: o.run(text, offs), host_offsets=True),
        Entry("half_final", lambda tx, of, n, fl, p: L.pire_hip_run_half_final(t._h, tx, of, n, BE | fl, p[0], p[1], p[2], None),
              lambda n: [(np.uint32, (n,)), (np.uint8, (n,)), (np.uint32, (n, R))], lambda text, offs: o.run_half_final(text, offs),
              host_offsets=True),
        Entry("prefix", lambda tx, of, n, fl, p: L.pire_hip_prefix(t._h, tx, of, n, 1, 0, 0, fl, p[0], None),
              lambda n: [(np.int64, (n,))], lambda text, offs: (o.prefix(text, offs, True),)),
        Entry("suffix", lambda tx, of, n, fl, p: L.pire_hip_suffix(t._h, tx, of, n, 1, 0, 0, fl, p[0], None),
              lambda n: [(np.int64, (n,))], lambda text, offs: (o.suffix(text, offs, True),)),
        Entry("counting", lambda tx, of, n, fl, p: L.pire_hip_counting_run(ct._h, ct.kind, tx, of, n, BE | fl, p[0], p[1], None),
              lambda n: [(np.uint32, (n,)), (np.uint32, (n, ct.RegexpsCount))], lambda text, offs: co.run(text, offs)),
        Entry("capture", lambda tx, of, n, fl, p: L.pire_hip_capture_run(kt._h, tx, of, n, BE | fl, p[0], p[1], p[2], p[3], None),
              lambda n: [(np.uint32, (n,)), (np.uint8, (n,)), (np.int64, (n,)), (np.int64, (n,))], capture_oracle),
        Entry("slow", lambda tx, of, n, fl, p: L.pire_hip_slow_run(st._h, tx, of, n, BE | fl, p[0], p[1], None, None),
              lambda n: [(np.uint8, (n,)), (np.uint32, (n, st.words))], lambda text, offs: so.run(text, offs)),
    ]


NAMES = ["run", "half_final", "prefix", "suffix", "counting", "capture", "slow"]


@pytest.fixture(scope="module")
def by_name():
    return {e.name: e for e in entries()}


def _host_call(e, text, offs, flags=0, sentinel=0xA5, null=()):
    """The host-pointer form; the result arrays start out filled with `sentinel` bytes.  null: the indices of the result
    arrays that the call gets a null pointer for."""
    n = len(offs) - 1
    outs = [np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, sentinel, dtype=np.uint8).view(dt).reshape(shape)
            for dt, shape in e.outs(n)]
    rc = e.call(text.ctypes.data if text is not None and text.size else None, offs.ctypes.data, n, flags,
                [None if k in null else a.ctypes.data for k, a in enumerate(outs)])
    return rc, outs


def _device_call(e, text, offs, host_offsets=False):
    """The same call with every array on the device (host_offsets: all but the offsets)."""
    import torch
    from pire_amd import binding as pb

    n = len(offs) - 1
    d_text = torch.as_tensor(text if text.size else np.zeros(1, dtype=np.uint8), device="cuda")
    d_offs = torch.as_tensor(offs.view(np.int64), device="cuda")
    outs = [torch.zeros(max(int(np.prod(shape)) * np.dtype(dt).itemsize, 1), dtype=torch.uint8, device="cuda") for dt, shape in e.outs(n)]
    torch.cuda.synchronize()
    flags = pb.FLAG_ON_DEVICE | (pb.FLAG_HOST_OFFSETS if host_offsets else 0)
    rc = e.call(d_text.data_ptr(), offs.ctypes.data if host_offsets else d_offs.data_ptr(), n, flags, [a.data_ptr() for a in outs])
    torch.cuda.synchronize()
    got = [a.cpu().numpy()[:int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape) for a, (dt, shape) in zip(outs, e.outs(n))]
    return rc, got


def _last_error():
    from pire_amd import binding as pb

    return pb.lib().pire_hip_last_error().decode()


def _untouched(outs, sentinel=0xA5):
    return all((a.view(np.uint8) == sentinel).all() for a in outs)


def _batch():
    text, offs = H.pack([b"hello world", b"abcde", b"", b"x=12 y", b"google_id = 'a1'"])
    return np.ascontiguousarray(text), offs


# ---- refusals ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_decreasing_host_offsets_are_refused(name, by_name):
    """Offsets that decrease: PIRE_HIP_EINVAL, "offsets must be non-decreasing", nothing written.  (pire_hip_slow_run did
    not make this check before the entry points shared one validator -- it launched on such offsets: the slow case is the
    one that fails on the commit before.)"""
    e = by_name[name]
    text, offs = _batch()
    offs[3] = 10          # 0, 11, 16, 10, 22, 38
    assert offs[2] > offs[3]
    rc, outs = _host_call(e, text, offs)
    assert rc == EINVAL
    assert "offsets must be non-decreasing" in _last_error()
    assert _untouched(outs)


@pytest.mark.parametrize("name", ["run", "half_final"])
def test_decreasing_host_offsets_of_resident_text_are_refused(name, by_name):
    import torch
    from pire_amd import binding as pb

    e = by_name[name]
    text, offs = _batch()
    offs[3] = 10
    n = len(offs) - 1
    d_text = torch.as_tensor(text, device="cuda")
    outs = [torch.full((max(int(np.prod(shape)) * np.dtype(dt).itemsize, 1),), 0xA5, dtype=torch.uint8, device="cuda") for dt, shape in e.outs(n)]
    torch.cuda.synchronize()
    rc = e.call(d_text.data_ptr(), offs.ctypes.data, n, pb.FLAG_ON_DEVICE | pb.FLAG_HOST_OFFSETS, [a.data_ptr() for a in outs])
    assert rc == EINVAL
    assert "offsets must be non-decreasing" in _last_error()
    torch.cuda.synchronize()
    assert all(bool((a == 0xA5).all()) for a in outs)


@pytest.mark.parametrize("name", NAMES)
def test_null_text_is_refused_unless_every_string_is_empty(name, by_name):
    e = by_name[name]
    _, offs = _batch()
    rc, outs = _host_call(e, None, offs)
    assert rc == EINVAL
    assert "null text pointer" in _last_error()
    assert _untouched(outs)
    empty = np.zeros(6, dtype=np.uint64)
    rc, outs = _host_call(e, None, empty)
    assert rc == 0, _last_error()
    want = e.oracle(np.zeros(0, dtype=np.uint8), empty)
    assert all((g == w).all() for g, w in zip(outs, want))


# ---- one path ------------------------------------------------------------------------------------------------------------

def _random_batch(seed, n, max_len):
    rng = np.random.RandomState(seed)
    strings = H.random_strings(rng, n, max_len, ALPHABET)
    strings[n // 2] = b""
    text, offs = H.pack(strings)
    return np.ascontiguousarray(text), offs


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_host_and_device_forms_agree_with_the_oracle(name, by_name, cfg):
    e = by_name[name]
    for seed, n, max_len in ((1, 300, 60), (2, 700, 200)):
        text, offs = _random_batch(seed, n, max_len)
        want = [np.asarray(w) for w in e.oracle(text, offs)]
        rc, dev = _device_call(e, text, offs)
        assert rc == 0, _last_error()
        assert _same(dev, want), (name, "device")
        if e.host_offsets:
            rc, dev = _device_call(e, text, offs, host_offsets=True)
            assert rc == 0, _last_error()
            assert _same(dev, want), (name, "device, host offsets")
        for mode in (0, 1, 2):
            cfg.set(host_staging=mode)
            rc, host = _host_call(e, text, offs)
            assert rc == 0, _last_error()
            assert _same(host, want), (name, "host", mode)


@pytest.mark.parametrize("name", ["counting", "capture", "slow"])
@pytest.mark.parametrize("text_bytes", [256 * 1024 - 9000, 256 * 1024 - 300, 256 * 1024 + 4096])
def test_calls_around_the_size_of_the_staging_arena(name, text_bytes, by_name, cfg):
    """As tests/test_host_staging.py for run / prefix / half-final: inputs and results that fit the 256 KiB arena, fit it
    in part, or not at all -- host and device forms against the oracle, the host form in every staging mode."""
    e = by_name[name]
    rng = np.random.RandomState(text_bytes % 9973)
    n = 900
    lens = rng.multinomial(text_bytes - n, np.ones(n) / n) + 1
    alphabet = np.frombuffer(ALPHABET, dtype=np.uint8)
    text = np.ascontiguousarray(alphabet[rng.randint(0, len(alphabet), size=text_bytes)])
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    assert int(offs[n]) == text_bytes
    want = [np.asarray(w) for w in e.oracle(text, offs)]
    rc, dev = _device_call(e, text, offs)
    assert rc == 0, _last_error()
    assert _same(dev, want)
    for mode in (0, 1, 2, 0):
        cfg.set(host_staging=mode)
        rc, host = _host_call(e, text, offs)
        assert rc == 0, _last_error()
        assert _same(host, want), mode


# ---- nullable outputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("null", [(0,), (1,), (0, 1)])
def test_capture_host_call_without_state_or_final_array(null, by_name, cfg):
    """out_state_idx and out_final of pire_hip_capture_run may each be null: the arrays that were asked for hold the
    oracle's answer, the others are not touched -- a batch inside the staging arena and one beyond it."""
    e = by_name["capture"]
    for seed, n, max_len in ((3, 40, 60), (4, 2000, 300)):
        text, offs = _random_batch(seed, n, max_len)
        want = [np.asarray(w) for w in e.oracle(text, offs)]
        for mode in (0, 1, 2):
            cfg.set(host_staging=mode)
            rc, got = _host_call(e, text, offs, null=null)
            assert rc == 0, _last_error()
            for k in range(4):
                if k in null:
                    assert _untouched([got[k]]), (mode, k)
                else:
                    assert (got[k] == want[k]).all(), (mode, k)


@pytest.fixture(scope="module")
def slow():
    import pire_amd

    blob = H.load_blob(_golden("slow", "slow_alt")["blob"])
    return pire_amd.SlowTable(blob), ob.OracleSlowScanner(blob)


# (out_final, out_state_bits) asked for next to out_counts
@pytest.mark.parametrize("asked", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("strided", [False, True])
def test_slow_host_call_accumulates_counts_with_any_other_outputs(asked, strided, slow, cfg):
    """out_counts of a host-pointer pire_hip_slow_run[_strided] is an input as well as a result ([0] += strings ending
    Final, [1] += n), and out_final / out_state_bits may be null next to it -- with both null the counters are the
    call's only array besides the text, and the kernels must still see the staged text, offsets and counters."""
    from pire_amd import binding as pb

    st, so = slow
    L = pb.lib()
    for seed, n, max_len in ((5, 10, 40), (6, 600, 120), (7, 4000, 150)):   # the last one: beyond the staging arena
        if strided:
            rng = np.random.RandomState(seed)
            length = max_len // 2
            text = np.ascontiguousarray(rng.choice(np.frombuffer(ALPHABET, dtype=np.uint8), size=n * length))
            offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
        else:
            text, offs = _random_batch(seed, n, max_len)
        want_final, want_bits = (np.asarray(w) for w in so.run(text, offs))
        for mode in (0, 1, 2):
            cfg.set(host_staging=mode)
            final = np.full(n, 0xA5, dtype=np.uint8)
            bits = np.full((n, st.words), 0xA5A5A5A5, dtype=np.uint32)
            counts = np.array([5, 7], dtype=np.uint64)
            pf = final.ctypes.data if asked[0] else None
            pbits = bits.ctypes.data if asked[1] else None
            if strided:
                rc = L.pire_hip_slow_run_strided(st._h, text.ctypes.data, n, length, length, BE, pf, pbits, counts.ctypes.data, None)
            else:
                rc = L.pire_hip_slow_run(st._h, text.ctypes.data, offs.ctypes.data, n, BE, pf, pbits, counts.ctypes.data, None)
            assert rc == 0, _last_error()
            assert counts.tolist() == [5 + int(want_final.astype(bool).sum()), 7 + n], (mode, n)
            assert (final == want_final).all() if asked[0] else _untouched([final]), (mode, n)
            assert (bits == want_bits).all() if asked[1] else _untouched([bits]), (mode, n)
