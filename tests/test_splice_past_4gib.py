"""pire_hip_splice at byte offsets past 4 GiB (modelled on tests/test_search_past_4gib.py).

One device buffer of 2^32 + 2^20 bytes and an output of that size; a small span list is laid across SOURCE byte 2^32 -- a span
that straddles it, an insertion on it, spans next to it -- behind one early span that shifts everything, so that OUTPUT byte
2^32 falls a few bytes beside it, inside the same window, once with a result that shrinks and once with one that grows.  The
pass computes every position from 64-bit sums; positions, offsets and the byte count do not fit 32 bits.  Only the window around
the crossing, the first bytes and the end of the output are compared: with tests/test_splice.py's model on the window alone (the
bytes in front of the window are copied as they are, so the model of the window is the output there, moved by the early span's
growth).

Skipped where the device has not that much free memory."""
import numpy as np
import pytest

from pire_amd import binding as pb
from tests import helpers as H
from tests.test_splice import KEEP, POISON, model_splice, some_bytes

G4 = H.FOUR_GIB
BIG_BYTES = G4 + (1 << 20)
HALF = 256
gpu = pytest.mark.gpu


@gpu
def test_spans_across_source_and_output_byte_2_to_the_32():
    import torch

    assert torch.cuda.is_available()
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * BIG_BYTES + (1 << 28):
        pytest.skip("%.1f GiB of device memory free, the test needs %.1f" % (free / 2 ** 30, 2 * BIG_BYTES / 2 ** 30 + 0.25))
    big = torch.empty(BIG_BYTES, dtype=torch.uint8, device="cuda")
    out = torch.empty(BIG_BYTES + 4096, dtype=torch.uint8, device="cuda")
    try:
        big.fill_(ord("a"))
        stream = torch.cuda.current_stream().cuda_stream
        w0 = G4 - HALF
        window = some_bytes(2 * HALF, 61).upper()
        big[w0:w0 + 2 * HALF] = torch.as_tensor(np.frombuffer(window, dtype=np.uint8).copy(), device="cuda")
        early = (100, 110)
        near = [(G4 - 40, G4 - 37), (G4 - 9, G4 - 9), (G4 - 2, G4 + 3), (G4 + 3, G4 + 3), (G4 + 5, G4 + 9), (G4 + 9, G4 + 10), (G4 + 30, G4 + 47)]
        spans = np.array([early] + near, dtype=np.uint64)
        offsets = np.array([0, 110, G4 - 9, G4 + 1, G4 + 3, BIG_BYTES], dtype=np.uint64)
        d_spans = torch.as_tensor(spans.view(np.int64), device="cuda")
        d_offs = torch.as_tensor(offsets.view(np.int64), device="cuda")
        k = len(spans)
        for head, tail, mode in ((b"XYZ", b"", 0), (b"<", b">", KEEP), (b"", b"", 0)):
            what = (head, tail, mode)
            out.fill_(POISON)
            d_pos = torch.full((k + 2,), -77, dtype=torch.int64, device="cuda")
            d_out_offs = torch.full((len(offsets) + 2,), -77, dtype=torch.int64, device="cuda")
            d_bytes = torch.full((3,), -77, dtype=torch.int64, device="cuda")
            pb.splice_device(big.data_ptr(), BIG_BYTES, d_spans.data_ptr(), k, d_bytes[1:].data_ptr(), head=head, tail=tail, mode=mode,
                             offsets_ptr=d_offs.data_ptr(), n=len(offsets) - 1, out_text_ptr=out.data_ptr(), text_cap=out.numel(),
                             out_pos_ptr=d_pos.data_ptr(), out_offsets_ptr=d_out_offs.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            # the model: the first bytes with the early span, the window with the spans near 2^32 (counted from the window's first byte)
            first = model_splice(b"a" * 300, [early], head, tail, mode)
            d0 = first["bytes"] - 300                                           # what the early span grows by
            rel = [(b - w0, e - w0) for b, e in near]
            rel_offs = [int(o) - w0 for o in offsets[2:5]]
            win = model_splice(window, rel, head, tail, mode, offsets=rel_offs)
            total = BIG_BYTES + d0 + win["bytes"] - len(window)
            assert d_bytes.cpu().tolist() == [-77, total, -77], what
            pos = d_pos.cpu().numpy()
            assert pos[:k].tolist() == [100] + [int(p) + w0 + d0 for p in win["pos"]] and (pos[k:] == -77).all(), what
            got_offs = d_out_offs.cpu().numpy()
            want_offs = [0, 110 + d0] + [int(o) + w0 + d0 for o in win["offsets"]] + [total]
            assert got_offs[:len(offsets)].tolist() == want_offs and (got_offs[len(offsets):] == -77).all(), what
            assert out[:200].cpu().numpy().tobytes() == first["text"][:200], what
            at = w0 + d0                                                        # where the window begins in the output
            assert at < G4 < at + win["bytes"] and w0 < G4 < w0 + len(window)    # both crossings lie inside it
            assert out[at - 64:at].cpu().numpy().tobytes() == b"a" * 64, what
            got = out[at:at + win["bytes"]].cpu().numpy().tobytes()
            assert got == win["text"], (what, got[HALF - 48:HALF + 64], win["text"][HALF - 48:HALF + 64])
            end = out[total - 64:total + 64].cpu().numpy()
            assert end[:64].tobytes() == b"a" * 64 and (end[64:] == POISON).all(), what
            assert int(pos[:k].max()) > G4 and int(got_offs[3]) > G4 - 64 and total > G4
        assert big[w0:w0 + 2 * HALF].cpu().numpy().tobytes() == window and int(big[G4 + 4096]) == ord("a")
    finally:
        del big, out
        torch.cuda.empty_cache()
