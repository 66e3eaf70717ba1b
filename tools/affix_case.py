#!/usr/bin/env python3
"""What the matched heads and tails cost on the device, and what they replace.

Input: 2^20 log lines (tools/split_case.py log_lines: the set_a corpus cut into lines of 64..1023 bytes), resident on the
device; every third line begins with a date ("2024-01-02 "), two lines of three end in blanks.  The scanners are
tests/golden/affix's `stamp` (forward) and `blanks` (from Fsm::Reverse()): the part asked for is REST, the line without its
date and without its trailing blanks, of the lines that have both.
  (a) the pass alone: pire_hip_affix_select (both length arrays, hits + spans) beside pire_hip_capture_select on the same n --
      positions made from the same lengths, so that both passes select the same strings and write the same spans; need_final
      with every flag set: 17 bytes a string against 16.  Device events around `--inner` back-to-back enqueue-only calls,
      median of `--reps` warmed repetitions, the two sides alternating repetition by repetition.
  (b) the lines form: pire_hip_affix_lines_gather on the resident buffer, hits, spans and the gathered text left on the device,
      beside what a caller does without it: pire_hip_split, pire_hip_prefix and pire_hip_suffix on the device, the n + 1 offsets
      and 2 n lengths fetched, the spans made in NumPy, staged back, pire_hip_gather_spans.  Host wall clock around a call that
      ends in a synchronise, median of `--reps`, alternating.
The answers of both sides are compared before anything is timed.

    python tools/affix_case.py [--reps 7] [--inner 10] [--out profiles/affix_case.txt] [--small]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pire_amd  # noqa: E402
from pire_amd import binding as pb  # noqa: E402
from split_case import log_lines  # noqa: E402

AFFIX = os.path.join(ROOT, "tests", "golden", "affix")
STAMP = b"2024-01-02 "


def blob(name):
    with open(os.path.join(AFFIX, name), "rb") as f:
        return f.read()


def stamped_lines(n):
    """(raw u8 on the device): log_lines with a date in front of every third line and blanks at the end of two lines of three"""
    _, raw = log_lines(n)
    ends = torch.nonzero(raw == 10).reshape(-1)                    # the newline of every line
    assert ends.numel() == n
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends[:-1] + 1])
    i = torch.arange(n, device="cuda")
    stamp = torch.as_tensor(np.frombuffer(STAMP, dtype=np.uint8).copy(), device="cuda")
    at = starts[i % 3 == 0]
    raw[(at[:, None] + torch.arange(len(STAMP), device="cuda")[None, :]).reshape(-1)] = stamp.repeat(at.numel())
    last = ends[i % 3 != 2]
    raw[last - 1] = 32
    raw[last - 2] = 9
    return raw


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(sides, reps, once):
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            samples[k].append(once(fn))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affix_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    head, tail = pire_amd.Table(blob("stamp.n.blob")), pire_amd.Table(blob("blanks.nr.blob"))
    raw = stamped_lines(n)
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")

    # the lines as a batch, and their lengths: the inputs of (a)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, **i64)
    words = torch.zeros(4, **i64)
    head_len, tail_len = torch.empty(n, **i64), torch.empty(n, **i64)

    def scans():
        pb.split_device(raw.data_ptr(), size, words.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
        head.prefix_device(text.data_ptr(), offs.data_ptr(), n, True, head_len.data_ptr(), stream=stream)
        tail.suffix_device(text.data_ptr(), offs.data_ptr(), n, True, tail_len.data_ptr(), stream=stream)

    scans()
    torch.cuda.synchronize()
    assert int(words.cpu()[0]) == n
    lens = offs[1:] - offs[:-1]
    sel = (head_len >= 0) & (tail_len >= 0)
    selected = int(sel.sum().cpu())
    # capture positions that mean the same spans under PIRE_HIP_RUN_BEGIN: begin = h + 1, end = len - r + 1
    h = torch.minimum(head_len.clamp(min=0), lens)
    r = torch.minimum(tail_len.clamp(min=0), lens - h)
    begin = torch.where(sel, h + 1, torch.full_like(h, -1))
    end = torch.where(sel, lens - r + 1, torch.full_like(h, -1))
    fin = torch.ones(n, dtype=torch.uint8, device="cuda")
    hits = torch.zeros((2, n), **i64)
    spans = torch.zeros((2, n, 2), **i64)
    counts = torch.zeros(2, **i64)
    sides = {
        "affix": lambda: pb.affix_select_device(offs.data_ptr(), n, counts[0:].data_ptr(), head_len.data_ptr(), tail_len.data_ptr(), pb.AFFIX_REST,
                                                hits[0].data_ptr(), spans[0].data_ptr(), n, stream),
        "capture": lambda: pb.capture_select_device(offs.data_ptr(), n, pb.FLAG_BEGIN, begin.data_ptr(), end.data_ptr(), counts[1:].data_ptr(),
                                                    fin.data_ptr(), True, hits[1].data_ptr(), spans[1].data_ptr(), n, stream),
    }
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    same_pass = counts.cpu().tolist() == [selected, selected] and bool((hits[0, :selected] == hits[1, :selected]).all().item()) \
        and bool((spans[0, :selected] == spans[1, :selected]).all().item())
    a_ms = alternate(sides, a.reps, lambda fn: event_ms(fn, a.inner))

    # (b) the lines form against the host's spans
    f_hits, f_spans = torch.zeros(n, **i64), torch.zeros((n, 2), **i64)
    f_text, f_offs = torch.empty(size + n, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, **i64)
    f_words = torch.zeros(3, **i64)                                  # lines, hits, bytes
    g_text, g_offs = torch.empty(size + n, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, **i64)
    g_spans = torch.zeros((n, 2), **i64)
    g_words = torch.zeros(1, **i64)
    g_count = [0]

    def fused():
        pb.affix_lines_gather_device(head, tail, raw.data_ptr(), size, f_words.data_ptr(), f_words[1:].data_ptr(), pb.AFFIX_REST,
                                     f_words[2:].data_ptr(), 10, out_hits_ptr=f_hits.data_ptr(), out_spans_ptr=f_spans.data_ptr(), hit_cap=n,
                                     out_text_ptr=f_text.data_ptr(), text_cap=size + n, out_offsets_ptr=f_offs.data_ptr(), stream=stream)

    def by_hand():
        scans()
        o = offs.cpu().numpy()
        hl, tl = head_len.cpu().numpy(), tail_len.cpu().numpy()
        ln = o[1:] - o[:-1]
        keep = (hl >= 0) & (tl >= 0)
        hh = np.minimum(hl[keep], ln[keep])
        rr = np.minimum(tl[keep], ln[keep] - hh)
        sp = np.stack([o[:-1][keep] + hh, o[1:][keep] - rr], axis=1)
        k = len(sp)
        g_spans[:k] = torch.as_tensor(sp, device="cuda")
        g_count[0] = k
        pb.gather_spans_device(text.data_ptr(), size, g_spans.data_ptr(), g_words.data_ptr(), span_cap=k, tail=10, out_text_ptr=g_text.data_ptr(),
                               text_cap=size + n, out_offsets_ptr=g_offs.data_ptr(), stream=stream)

    fused()
    by_hand()
    torch.cuda.synchronize()
    lines_n, f_count, f_bytes = f_words.cpu().tolist()
    same_lines = (lines_n, f_count) == (n, selected) and g_count[0] == selected and int(g_words.cpu()[0]) == f_bytes \
        and bool((f_text[:f_bytes] == g_text[:f_bytes]).all().item()) and bool((f_offs[:selected + 1] == g_offs[:selected + 1]).all().item()) \
        and bool((f_hits[:selected] == hits[0, :selected]).all().item())
    b_ms = alternate({"fused": fused, "by_hand": by_hand}, a.reps, wall_ms)

    fmt = lambda m: "%.4f ms (min %.4f, max %.4f)" % m   # noqa: E731
    ratio = a_ms["affix"][0] / a_ms["capture"][0]
    out = ["# tools/affix_case.py: %d log lines, %.1f MB, resident; head `stamp` (%s...), tail `blanks` reversed, part REST" % (n, size / 1e6, STAMP.decode()),
           "# (a) device events around %d back-to-back enqueue-only calls; (b) host wall clock around one call and a synchronise;" % a.inner,
           "# median (min, max) of %d warmed repetitions, the two sides alternating, one run" % a.reps,
           "selected %d of %d lines (%.1f %%)   same answer: pass %s, lines %s" % (selected, n, 100.0 * selected / n, same_pass, same_lines),
           "(a) pire_hip_affix_select, both arrays, hits + spans (16 B a string read):      %s" % fmt(a_ms["affix"]),
           "(a) pire_hip_capture_select, need_final, hits + spans (17 B a string read):    %s" % fmt(a_ms["capture"]),
           "(a) affix / capture = %.2f" % ratio,
           "(b) pire_hip_affix_lines_gather, hits, spans and %.1f MB of text left on the device: %s" % (f_bytes / 1e6, fmt(b_ms["fused"])),
           "(b) split + prefix + suffix on the device, %.1f MB of offsets and lengths fetched, spans in NumPy, staged," % (24.0 * n / 1e6),
           "    pire_hip_gather_spans:                                                       %s" % fmt(b_ms["by_hand"]),
           "(b) by hand / fused = %.2f" % (b_ms["by_hand"][0] / b_ms["fused"][0])]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same_pass and same_lines else 1


if __name__ == "__main__":
    sys.exit(main())
