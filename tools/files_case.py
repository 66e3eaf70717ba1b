#!/usr/bin/env python3
"""What hits by file cost on the device, and what one call for many files replaces.

Input: 2^20 log lines (tools/split_case.py log_lines: the set_a corpus cut into lines of 64..1023 bytes), resident on the
device.
  (a) the pass alone: pire_hip_files on a hit list of about 1 % of the lines, drawn at random, for 1, 4 096 and 2^18 files of
      equal size -- first, the file and the line of every hit, the file list and its count written -- beside pire_hip_select
      (the state indices of a scan of the same lines, hits written) and pire_hip_context (the same list, before = after = 2) on
      the same n.  Device events around `--inner` back-to-back enqueue-only calls, median of `--reps` warmed repetitions, the
      sides alternating repetition by repetition.
  (b) the lines form: the buffer cut into 4 096 files of 256 lines, pire_hip_run_lines_files_select in ONE call (everything left
      on the device), beside 4 096 calls of pire_hip_run_lines_select, one per file, on the same resident bytes (what a grep
      that calls once per file does; every call reads its line count back), and beside one pire_hip_split + one
      pire_hip_run_lines_select with the offsets and the hits fetched and the grouping done in NumPy on the host.  Host wall
      clock around a side that ends in a synchronise, median of `--reps`, alternating.
The answers are compared with the NumPy formula before anything is timed.

    python tools/files_case.py [--reps 7] [--inner 10] [--out profiles/files_case.txt] [--small]
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


def by_file(hits, bounds):
    """include/pire_hip.h: first, the file and the line of every hit, the files with a hit"""
    h, b = hits.astype(np.int64), bounds.astype(np.int64)
    first = np.searchsorted(h, b, side="left")
    hit_file = np.searchsorted(b, h, side="right") - 1
    return first, hit_file, h - b[hit_file], np.flatnonzero(np.diff(first) > 0)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "files_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    table, raw = log_lines(n)
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")
    be = pb.FLAG_BEGIN | pb.FLAG_END

    # (a) a list of the test's own; the state indices of a scan of the lines for pire_hip_select
    mask = np.random.RandomState(20).randint(0, 100, size=n) == 0
    hits_np = np.flatnonzero(mask)
    k = len(hits_np)
    hits = torch.as_tensor(hits_np, device="cuda")
    file_counts = (1, 4096, n // 4)
    bounds_np = {f: (np.arange(f + 1, dtype=np.int64) * (n // f)) for f in file_counts}
    bounds = {f: torch.as_tensor(b, device="cuda") for f, b in bounds_np.items()}
    first = torch.zeros(n // 4 + 1, **i64)
    hit_file, hit_line, listed = torch.zeros(k, **i64), torch.zeros(k, **i64), torch.zeros(n // 4, **i64)
    counts = torch.zeros(8, **i64)                                     # files: count; select: hits; context: lines, runs; split: n
    text, offs = torch.empty(size + 16, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, **i64)
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    pb.split_device(raw.data_ptr(), size, counts[4:].data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    table.run_device(text.data_ptr(), offs.data_ptr(), n, be, out_idx_ptr=idx.data_ptr(), stream=stream)
    sel_hits, ctx_lines, ctx_flags = torch.zeros(n, **i64), torch.zeros(n, **i64), torch.zeros(n, dtype=torch.uint8, device="cuda")

    def files_pass(f):
        return lambda: pb.files_device(hits.data_ptr(), k, n, bounds[f].data_ptr(), f, counts.data_ptr(), out_file_first_ptr=first.data_ptr(),
                                       out_hit_file_ptr=hit_file.data_ptr(), out_hit_line_ptr=hit_line.data_ptr(), out_files_ptr=listed.data_ptr(),
                                       file_cap=f, stream=stream)

    same_pass = True
    for f in file_counts:
        files_pass(f)()
        torch.cuda.synchronize()
        w_first, w_file, w_line, w_listed = by_file(hits_np, bounds_np[f])
        same_pass = same_pass and int(counts[0]) == len(w_listed) and (first[:f + 1].cpu().numpy() == w_first).all() \
            and (hit_file.cpu().numpy() == w_file).all() and (hit_line.cpu().numpy() == w_line).all() \
            and (listed[:len(w_listed)].cpu().numpy() == w_listed).all()
    sides = {"files %d" % f: files_pass(f) for f in file_counts}
    sides["select"] = lambda: table.select_device(idx.data_ptr(), n, counts[1:].data_ptr(), out_hits_ptr=sel_hits.data_ptr(), hit_cap=n, stream=stream)
    sides["context"] = lambda: pb.context_device(hits.data_ptr(), k, n, counts[2:].data_ptr(), 2, 2, out_lines_ptr=ctx_lines.data_ptr(),
                                                 out_line_flags_ptr=ctx_flags.data_ptr(), line_cap=n, out_group_count_ptr=counts[3:].data_ptr(),
                                                 stream=stream)
    a_ms = alternate(sides, a.reps, lambda fn: event_ms(fn, a.inner))
    sel_count = int(counts[1])

    # (b) 4 096 files of n / 4 096 lines: one call, a call per file, one call and NumPy
    files = 4096
    per = n // files
    o = offs.cpu().numpy()
    fb_np = np.concatenate([(o[::per] + np.arange(0, n + 1, per))[:files], [size]]).astype(np.int64)   # line i begins at o[i] + i of raw
    fb = torch.as_tensor(fb_np, device="cuda")
    f_hits, f_file, f_line = torch.zeros(n, **i64), torch.zeros(n, **i64), torch.zeros(n, **i64)
    f_first, f_lines, f_listed = torch.zeros(files + 1, **i64), torch.zeros(files + 1, **i64), torch.zeros(files, **i64)
    f_words = torch.zeros(4, **i64)                                    # lines, hits, listed files, straddles
    p_hits, p_words = torch.zeros(n, **i64), torch.zeros((files, 2), **i64)
    g_offs, g_hits, g_words = torch.zeros(n + 1, **i64), torch.zeros(n, **i64), torch.zeros(3, **i64)
    grouped = [None]

    def one_call():
        table.run_lines_files_device(raw.data_ptr(), size, be, fb.data_ptr(), files, f_words.data_ptr(), f_words[1:].data_ptr(),
                                     f_words[2:].data_ptr(), f_words[3:].data_ptr(), out_hits_ptr=f_hits.data_ptr(), out_hit_file_ptr=f_file.data_ptr(),
                                     out_hit_line_ptr=f_line.data_ptr(), hit_cap=n, out_file_lines_ptr=f_lines.data_ptr(),
                                     out_file_first_ptr=f_first.data_ptr(), out_files_ptr=f_listed.data_ptr(), file_cap=files, stream=stream)

    raw_ptr, p_hits_ptr, p_words_ptr = raw.data_ptr(), p_hits.data_ptr(), p_words.data_ptr()
    fb_list = fb_np.tolist()

    def per_file():
        for f in range(files):
            table.run_lines_select_device(raw_ptr + fb_list[f], fb_list[f + 1] - fb_list[f], be, p_words_ptr + 16 * f, p_words_ptr + 16 * f + 8,
                                          out_hits_ptr=p_hits_ptr + 8 * per * f, hit_cap=per, stream=stream)

    def one_call_and_numpy():
        pb.split_device(raw.data_ptr(), size, g_words.data_ptr(), 10, 0, g_offs.data_ptr(), n, stream)
        table.run_lines_select_device(raw.data_ptr(), size, be, g_words[1:].data_ptr(), g_words[2:].data_ptr(), out_hits_ptr=g_hits.data_ptr(),
                                      hit_cap=n, stream=stream)
        count = int(g_words.cpu()[2])
        starts = g_offs.cpu().numpy()[:-1]                             # (the split kept every delimiter: offsets into raw)
        file_lines = np.searchsorted(starts, fb_np, side="left")
        grouped[0] = (file_lines,) + by_file(g_hits[:count].cpu().numpy(), file_lines)

    one_call()
    per_file()
    one_call_and_numpy()
    torch.cuda.synchronize()
    lines_n, f_count, f_with, f_straddles = f_words.cpu().tolist()
    w_lines, w_first, w_file, w_line, w_listed = grouped[0]
    per_counts = p_words.cpu().numpy()
    same_lines = lines_n == n and f_straddles == 0 and f_count == len(w_file) and f_with == len(w_listed) \
        and (f_lines.cpu().numpy() == w_lines).all() and (f_first.cpu().numpy() == w_first).all() \
        and (f_file[:f_count].cpu().numpy() == w_file).all() and (f_line[:f_count].cpu().numpy() == w_line).all() \
        and (f_listed[:f_with].cpu().numpy() == w_listed).all() and (per_counts[:, 0] == per).all() and (per_counts[:, 1] == np.diff(w_first)).all()
    b_ms = alternate({"one": one_call, "per_file": per_file, "numpy": one_call_and_numpy}, a.reps, wall_ms)

    fmt = lambda m: "%.4f ms (min %.4f, max %.4f)" % m   # noqa: E731
    out = ["# python tools/files_case.py --reps %d --inner %d%s" % (a.reps, a.inner, " --small" if a.small else ""),
           "# tools/files_case.py: %d log lines, %.1f MB, resident; (a): %d hits drawn at random (%.2f %%); (b): table set_a, its Final lines"
           % (n, size / 1e6, k, 100.0 * k / n),
           "# (a) device events around %d back-to-back enqueue-only calls; (b) host wall clock around one side and a synchronise;" % a.inner,
           "# median (min, max) of %d warmed repetitions, the sides alternating, one run" % a.reps,
           "same answer as the NumPy formula: pass %s, lines %s" % (bool(same_pass), bool(same_lines))]
    for f in file_counts:
        out.append("(a) pire_hip_files, %7d files of %7d lines, first + file and line of every hit + file list: %s" % (f, n // f, fmt(a_ms["files %d" % f])))
    out += ["(a) pire_hip_select on the same n, %d hits written:                                          %s" % (sel_count, fmt(a_ms["select"])),
            "(a) pire_hip_context on the same list, before = after = 2:                                      %s" % fmt(a_ms["context"]),
            "(a) files(4096) / select = %.2f, files(4096) / context = %.2f"
            % (a_ms["files 4096"][0] / a_ms["select"][0], a_ms["files 4096"][0] / a_ms["context"][0]),
            "(b) pire_hip_run_lines_files_select, %d files in ONE call, %d hits in %d files, everything left on the device: %s"
            % (files, f_count, f_with, fmt(b_ms["one"])),
            "(b) %d calls of pire_hip_run_lines_select, one per file of %d lines, the same resident bytes:       %s" % (files, per, fmt(b_ms["per_file"])),
            "(b) split + run_lines_select once, %.1f MB of offsets and hits fetched, grouping in NumPy:              %s"
            % ((8.0 * (n + 1) + 8.0 * f_count) / 1e6, fmt(b_ms["numpy"])),
            "(b) per file / one call = %.1f, NumPy / one call = %.2f, per call of the per-file side: %.1f us"
            % (b_ms["per_file"][0] / b_ms["one"][0], b_ms["numpy"][0] / b_ms["one"][0], 1e3 * b_ms["per_file"][0] / files)]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same_pass and same_lines else 1


if __name__ == "__main__":
    sys.exit(main())
