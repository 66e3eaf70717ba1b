"""pire_hip_search and pire_hip_search_run_select at byte offsets past 4 GiB (modelled on tests/test_past_4gib.py, Part A).

A batch of a few hundred short strings is laid across byte 2^32 of one device buffer of 2^32 + 2^20 bytes -- 2^32 between two
strings, inside one in the middle of a 16-byte chunk, inside one on a chunk's edge, on an empty string (helpers.across_4gib) --
and addressed twice: pointer = the buffer, offsets[0] = lead (every offset near or past 2^32 is used), and pointer = buffer +
lead, offsets from 0 (only the address is large).  Both legs of the kernel compute addresses from 64-bit offsets and keep
positions relative to the string; the spans of the pass are absolute and do not fit 32 bits.  The rest of the buffer holds
digits, which would match if a leg read outside its string.  Expected: tests/test_search.py's model on the strings alone.

Skipped where the device has not that much free memory.  Not covered: pire_hip_search_lines_gather on a raw buffer of more than
4 GiB (its split and gather are tests/test_past_4gib.py's; the search behind them is the one tested here)."""
import numpy as np
import pytest

from pire_amd import binding as pb
from tests import helpers as H
from tests.test_search import S, mixed_strings, model_search, model_select, tables_of

G4 = H.FOUR_GIB
BIG_BYTES = G4 + (1 << 20)
gpu = pytest.mark.gpu


@gpu
def test_both_legs_and_the_spans_across_byte_2_to_the_32():
    import torch

    assert torch.cuda.is_available()
    free = torch.cuda.mem_get_info()[0]
    if free < BIG_BYTES + (1 << 28):
        pytest.skip("%.1f GiB of device memory free, the test needs %.1f" % (free / 2 ** 30, BIG_BYTES / 2 ** 30 + 0.25))
    big = torch.empty(BIG_BYTES, dtype=torch.uint8, device="cuda")
    try:
        big.fill_(ord("7"))
        stream = torch.cuda.current_stream().cuda_stream
        base = mixed_strings(5, 300)
        for name, opts in (("num", 0), ("gap", 0), ("num", S)):
            tr, tf = tables_of(name)
            for where, mod in zip(H.ACROSS_WHERE, H.ACROSS_LEAD_MODS):
                strings, lead, k, d = H.across_4gib(base, where, mod, b"x" * 127)
                n = len(strings)
                text, offs = H.pack(strings)
                assert lead < G4 < lead + len(text) and lead + len(text) < BIG_BYTES
                big[lead:lead + len(text)] = torch.as_tensor(text.copy(), device="cuda")
                begin, end, _, _ = model_search(name, strings, opts)
                assert 50 < (begin >= 0).sum() < n
                for shifted in (True, False):
                    what = (name, opts, where, "offsets" if shifted else "pointer")
                    ptr = big.data_ptr() + (0 if shifted else lead)
                    o = offs + np.uint64(lead if shifted else 0)
                    d_offs = torch.as_tensor(o.view(np.int64), device="cuda")
                    d_b = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
                    d_e = torch.full((n + 2,), -77, dtype=torch.int64, device="cuda")
                    pb.search_device(tr, tf, ptr, d_offs.data_ptr(), n, d_b.data_ptr(), d_e.data_ptr(), opts, stream)
                    torch.cuda.synchronize()
                    gb, ge = d_b.cpu().numpy(), d_e.cpu().numpy()
                    assert (gb[n:] == -77).all() and (ge[n:] == -77).all(), what
                    bad = np.flatnonzero((gb[:n] != begin) | (ge[:n] != end))
                    assert bad.size == 0, (what, bad[:8], k, d)
                    # the pass behind it: spans past 2^32 where the offsets are
                    exp = model_select(begin, end, o)
                    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                    d_spans = torch.full((n + 1, 2), -77, dtype=torch.int64, device="cuda")
                    pb.search_run_select_device(tr, tf, ptr, d_offs.data_ptr(), n, cnt.data_ptr(), opts, out_spans_ptr=d_spans.data_ptr(),
                                                hit_cap=n, stream=stream)
                    torch.cuda.synchronize()
                    c = exp["count"]
                    spans = d_spans.cpu().numpy()
                    assert cnt.cpu().tolist() == [c] and (spans[:c].view(np.uint64) == exp["spans"]).all() and (spans[c:] == -77).all(), what
                    if shifted:
                        assert int(exp["spans"].max()) > G4 > int(exp["spans"].min())
                big[lead:lead + len(text)] = ord("7")
    finally:
        del big
        torch.cuda.empty_cache()
