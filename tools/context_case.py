#!/usr/bin/env python3
"""What the lines around a match cost on the device, and what they replace.

Input: 2^20 log lines (tools/split_case.py log_lines: the set_a corpus cut into lines of 64..1023 bytes), resident on the
device.
  (a) the pass alone: pire_hip_context on a hit list of about 1 % of the lines, drawn at random, before = after = 2 -- lines,
      flags and both counts written -- beside pire_hip_final_select on the same n (a flag array with the same lines set).
      Device events around `--inner` back-to-back enqueue-only calls, median of `--reps` warmed repetitions, the two sides
      alternating repetition by repetition.
  (b) the same list with after = 2^20: every tile behind the first hit takes its neighbour from outside its slice of the list,
      and every line behind it is selected.
  (c) the lines form: pire_hip_run_lines_context_gather (the table's Final lines, before = after = 2) on the resident buffer,
      lines, flags and the gathered text left on the device, beside what a caller does without it: pire_hip_split and
      pire_hip_run_lines_select on the device, the n + 1 offsets and the hits fetched, the windows made in NumPy, the lines
      joined on the host from a copy of the buffer that is there already (the copy is not timed).  Host wall clock around a
      call that ends in a synchronise, median of `--reps`, alternating.
The answers are compared with the NumPy formula before anything is timed.

    python tools/context_case.py [--reps 7] [--inner 10] [--out profiles/context_case.txt] [--small]
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

from pire_amd import binding as pb  # noqa: E402
from split_case import log_lines  # noqa: E402


def windows(hits, n, before, after):
    """include/pire_hip.h: the selected lines, their flags, the number of runs"""
    h, i = hits.astype(np.int64), np.arange(n, dtype=np.int64)
    pred, succ = np.searchsorted(h, i, side="right") - 1, np.searchsorted(h, i, side="left")
    sel = ((pred >= 0) & (i - h[np.maximum(pred, 0)] <= after)) | ((succ < h.size) & (h[np.minimum(succ, h.size - 1)] - i <= before))
    group = sel & ~np.concatenate([[False], sel[:-1]])
    lines = np.flatnonzero(sel)
    mark = np.zeros(n, dtype=np.uint8)
    mark[h] = pb.CONTEXT_HIT
    return lines, mark[lines] | (group[lines] * pb.CONTEXT_GROUP).astype(np.uint8), int(group.sum())


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    table, raw = log_lines(n)
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")
    be = pb.FLAG_BEGIN | pb.FLAG_END

    # (a), (b): a list of the test's own
    mask = np.random.RandomState(20).randint(0, 100, size=n) == 0
    hits_np = np.flatnonzero(mask)
    k = len(hits_np)
    hits = torch.as_tensor(hits_np, device="cuda")
    fin = torch.as_tensor(mask.astype(np.uint8), device="cuda")
    lines = torch.zeros((3, n), **i64)
    flags = torch.zeros((2, n), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(6, **i64)                                    # near: lines, runs; far: lines, runs; final: hits

    def context(row, before, after):
        return lambda: pb.context_device(hits.data_ptr(), k, n, counts[2 * row:].data_ptr(), before, after, out_lines_ptr=lines[row].data_ptr(),
                                         out_line_flags_ptr=flags[row].data_ptr(), line_cap=n, out_group_count_ptr=counts[2 * row + 1:].data_ptr(),
                                         stream=stream)

    sides = {"near": context(0, 2, 2), "far": context(1, 2, n),
             "final": lambda: pb.final_select_device(fin.data_ptr(), n, counts[4:].data_ptr(), out_hits_ptr=lines[2].data_ptr(), hit_cap=n, stream=stream)}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    got = counts.cpu().tolist()
    same_pass = got[4] == k and bool((lines[2, :k] == hits).all().item())
    selected = {}
    for row, (name, before, after) in enumerate((("near", 2, 2), ("far", 2, n))):
        want_lines, want_flags, want_runs = windows(hits_np, n, before, after)
        m = len(want_lines)
        selected[name] = m
        same_pass = same_pass and got[2 * row:2 * row + 2] == [m, want_runs] and (lines[row, :m].cpu().numpy() == want_lines).all() \
            and (flags[row, :m].cpu().numpy() == want_flags).all()
    a_ms = alternate(sides, a.reps, lambda fn: event_ms(fn, a.inner))

    # (c) the lines form against the host's windows and the host's join
    f_lines, f_flags = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.uint8, device="cuda")
    f_text, f_offs = torch.empty(size + n, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, **i64)
    f_words = torch.zeros(5, **i64)                                   # lines of the buffer, selected, runs, hits, bytes
    g_offs, g_hits, g_words = torch.zeros(n + 1, **i64), torch.zeros(n, **i64), torch.zeros(3, **i64)
    host_raw = raw.cpu().numpy()
    joined = [b""]

    def fused():
        table.run_lines_context_device(raw.data_ptr(), size, be, f_words.data_ptr(), f_words[1:].data_ptr(), 2, 2, out_lines_ptr=f_lines.data_ptr(),
                                       out_line_flags_ptr=f_flags.data_ptr(), line_cap=n, out_group_count_ptr=f_words[2:].data_ptr(),
                                       out_hit_count_ptr=f_words[3:].data_ptr(), out_bytes_ptr=f_words[4:].data_ptr(), out_text_ptr=f_text.data_ptr(),
                                       text_cap=size + n, out_offsets_ptr=f_offs.data_ptr(), stream=stream)

    def by_hand():
        pb.split_device(raw.data_ptr(), size, g_words.data_ptr(), 10, 0, g_offs.data_ptr(), n, stream)
        table.run_lines_select_device(raw.data_ptr(), size, be, g_words[1:].data_ptr(), g_words[2:].data_ptr(), out_hits_ptr=g_hits.data_ptr(),
                                      hit_cap=n, stream=stream)
        count = int(g_words.cpu()[2])
        o = g_offs.cpu().numpy()
        sel, _, _ = windows(g_hits[:count].cpu().numpy(), n, 2, 2)
        joined[0] = b"".join([host_raw[o[i]:o[i + 1]].tobytes() for i in sel.tolist()])   # (the split kept every delimiter)

    fused()
    by_hand()
    torch.cuda.synchronize()
    lines_n, f_sel, f_runs, f_hits, f_bytes = f_words.cpu().tolist()
    same_lines = lines_n == n and f_bytes == len(joined[0]) and f_text[:f_bytes].cpu().numpy().tobytes() == joined[0]
    c_ms = alternate({"fused": fused, "by_hand": by_hand}, a.reps, wall_ms)

    fmt = lambda m: "%.4f ms (min %.4f, max %.4f)" % m   # noqa: E731
    out = ["# tools/context_case.py: %d log lines, %.1f MB, resident; (a), (b): %d hits drawn at random (%.2f %%); (c): table set_a, its Final lines"
           % (n, size / 1e6, k, 100.0 * k / n),
           "# (a), (b) device events around %d back-to-back enqueue-only calls; (c) host wall clock around one call and a synchronise;" % a.inner,
           "# median (min, max) of %d warmed repetitions, the sides alternating, one run" % a.reps,
           "same answer as the NumPy formula: pass %s, lines %s" % (bool(same_pass), bool(same_lines)),
           "(a) pire_hip_context, before = after = 2, %d lines selected, lines + flags + both counts:   %s" % (selected["near"], fmt(a_ms["near"])),
           "(a) pire_hip_final_select on the same n, %d hits:                                       %s" % (k, fmt(a_ms["final"])),
           "(a) context / final = %.2f" % (a_ms["near"][0] / a_ms["final"][0]),
           "(b) pire_hip_context, before = 2, after = 2^20, %d lines selected:                      %s" % (selected["far"], fmt(a_ms["far"])),
           "(b) far / near = %.2f" % (a_ms["far"][0] / a_ms["near"][0]),
           "(c) pire_hip_run_lines_context_gather, %d hits, %d lines in %d runs, %.1f MB of text left on the device: %s"
           % (f_hits, f_sel, f_runs, f_bytes / 1e6, fmt(c_ms["fused"])),
           "(c) split + run_lines_select on the device, %.1f MB of offsets and hits fetched, windows in NumPy, join on the host: %s"
           % ((8.0 * (n + 1) + 8.0 * f_hits) / 1e6, fmt(c_ms["by_hand"])),
           "(c) by hand / fused = %.2f" % (c_ms["by_hand"][0] / c_ms["fused"][0])]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same_pass and same_lines else 1


if __name__ == "__main__":
    sys.exit(main())
