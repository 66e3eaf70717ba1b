#!/usr/bin/env python3
"""What gathering the selected strings on the device costs, and what it replaces.

The two workloads of tools/split_case.py, resident on the device -- log lines (the synthetic corpus of set_a cut into
lines of 64..1023 bytes) and URLs for the dict_1k blacklist scanner --, and a third batch of short lines with a few lines of
1 MiB and more among them.  Medians of warmed repetitions:
  (a) pire_hip_gather alone, device pointers, on the split text + offsets with a random ascending hit list of about 1 %,
      25 % and 90 % of the lines, a newline behind every string, in OUTPUT bytes per second (device events around `--inner`
      back-to-back calls), next to a device-to-device copy of the same number of bytes timed in the same run (torch's copy_
      of a contiguous tensor: hipMemcpyAsync) -- the floor of any pass that reads and writes every byte once;
  (b) pire_hip_run_lines_gather on the resident raw buffer, the gathered text and offsets left on the device for the next
      scan, against the route it replaces: pire_hip_run_lines_select, hits and spans fetched, the lines joined on the
      host (one slice per span and one bytes.join, on one core), text and offsets uploaded again.  Host wall
      clock around call + synchronise.  The hit rate is the scanner's own on that workload.

    python tools/gather_case.py [--reps 7] [--inner 10] [--out profiles/gather_case.txt] [--small] [--only-gather] [--trace-db DB]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pire_amd import binding as pb  # noqa: E402
from split_case import event_ms, log_lines, median_ms, urls  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def long_lines(n, seed=4321):
    """log_lines with five lines of 1..3 MiB among the short ones"""
    table, raw = log_lines(n, seed)
    host = raw.cpu().numpy()
    nl = np.flatnonzero(host == 10)
    rng = np.random.RandomState(seed)
    for start in rng.choice(len(nl) - 40000, size=5, replace=False):
        first = int(nl[start]) + 1
        stop = min(first + (1 << 20) * int(rng.randint(1, 4)), len(host) - 2)
        seg = host[first:stop]
        seg[seg == 10] = 32
    return table, torch.as_tensor(host, device="cuda")


def join_on_host(raw_bytes, spans, k):
    """The lines raw[b, e) and a newline behind each, back to back, and their offsets: one slice per span, one join, on one
    core -- what a caller without the gather writes"""
    b, e = spans[0:2 * k:2].astype(np.int64), spans[1:2 * k:2].astype(np.int64)
    view = memoryview(raw_bytes)
    joined = b"\n".join([view[i:j] for i, j in zip(b.tolist(), e.tolist())]) + (b"\n" if k else b"")
    offs = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(e - b + 1, out=offs[1:])
    return np.frombuffer(joined, dtype=np.uint8), offs


def trace_summary(db, out_path):
    """Medians per kernel and launch shape of the gather's kernels in a rocprofv3 --kernel-trace database (a run of
    `--only-gather` under the profiler): the copy kernel's rows are one per workload and hit rate, in the tool's order."""
    import sqlite3

    con = sqlite3.connect(db)
    rows = con.execute("select name, duration, grid_x, vgpr_count, static_lds_size from kernels where name like '%Gather%' "
                       "order by start").fetchall()
    import re

    calls, order, cur = {}, [], []
    for name, dur, grid, vgpr, lds in rows:             # a call = Lengths, Scan, Offsets, Copy, in that order
        kernel = re.search(r"Gather(\w+)Kernel", name).group(1)
        if kernel == "Lengths":
            cur = []
        cur.append((kernel, dur, grid, vgpr, lds))
        if kernel == "Copy" and len(cur) == 4:
            key = (cur[0][2], cur[3][2])                # strings (rounded up to 1 024) and the copy's grid: one per workload and hit rate
            if key not in calls:
                calls[key] = []
                order.append(key)
            calls[key].append(cur)
    lines = ["# tools/gather_case.py --trace-db: rocprofv3 --kernel-trace --stats of `gather_case.py --only-gather`; per workload and hit rate,",
             "# in the tool's order, the median over the calls of every kernel's time in us (copy: VGPRs, static LDS bytes)"]
    for key in order:
        c = calls[key]
        med = [float(np.median([call[i][1] for call in c])) / 1e3 for i in range(4)]
        lines.append("%8d strings  x%-3d lengths %6.1f  scan %6.1f  offsets %6.1f  copy %7.1f us  (%d VGPRs, %d B LDS)"
                     % (key[0], len(c), med[0], med[1], med[2], med[3], c[0][3][3], c[0][3][4]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)


def case(title, table, raw, a, out):
    size = raw.numel()
    stream = torch.cuda.current_stream().cuda_stream
    host_raw = raw.cpu().numpy()
    n = int((host_raw == 10).sum()) + (1 if host_raw[-1] != 10 else 0)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    host_offs = offs.cpu().numpy()
    lens = np.diff(host_offs)
    out.append(title)
    out.append("  raw %.1f MB, %d lines, %.1f B a line, longest %d B" % (size / 1e6, n, size / n, int(lens.max())))
    g_text = torch.empty(size + n + 16, dtype=torch.uint8, device="cuda")
    g_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    g_bytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    rng = np.random.RandomState(7)
    for rate in (0.01, 0.25, 0.9):
        pick = np.flatnonzero(rng.rand(n) < rate)
        if "1 MiB" in title:
            pick = np.union1d(pick, np.argsort(lens)[-5:])           # the long lines are among the selected ones
        k = len(pick)
        idx = torch.as_tensor(pick.astype(np.int64), device="cuda")
        kdev = torch.as_tensor(np.array([k], dtype=np.int64), device="cuda")
        total = int(lens[pick].sum()) + k

        def gather():
            pb.gather_device(text.data_ptr(), offs.data_ptr(), n, g_bytes.data_ptr(), idx_ptr=idx.data_ptr(), idx_count_ptr=kdev.data_ptr(),
                             idx_cap=k, tail=10, out_text_ptr=g_text.data_ptr(), text_cap=size + n, out_offsets_ptr=g_offs.data_ptr(),
                             stream=stream)

        src, dst = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
        gather_ms = event_ms(gather, a.reps, a.inner)
        copy_ms = event_ms(lambda: dst.copy_(src), a.reps, a.inner)
        torch.cuda.synchronize()
        assert int(g_bytes.cpu()[0]) == total
        j = k // 2                                                   # spot checks: the offsets' end, one string in the middle
        go = g_offs[:k + 1].cpu().numpy()
        assert int(go[k]) == total
        got = g_text[int(go[j]):int(go[j + 1])].cpu().numpy()
        want = text[int(host_offs[pick[j]]):int(host_offs[pick[j] + 1])].cpu().numpy()
        assert (got[:-1] == want).all() and got[-1] == 10, "the gathered string differs from its source"
        out.append("  (a) hit rate %.2f: %d strings, %.1f MB out   pire_hip_gather %.4f ms = %.0f GB/s of output   device-to-device copy "
                   "%.4f ms = %.0f GB/s   gather / copy rate %.2f"
                   % (rate, k, total / 1e6, gather_ms, total / gather_ms / 1e6, copy_ms, total / copy_ms / 1e6, copy_ms / gather_ms))
        del src, dst
    if a.only_gather:
        return
    # (b) end to end: the gathered batch on the device, ready for the next scan
    cap = n
    hits = torch.empty(cap, dtype=torch.int64, device="cuda")
    spans = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    got = {}
    raw_bytes = host_raw.tobytes()

    def new_route():
        table.run_lines_gather_device(raw.data_ptr(), size, BE, counts.data_ptr(), counts.data_ptr() + 8, counts.data_ptr() + 16,
                                      out_hits_ptr=hits.data_ptr(), hit_cap=cap, out_text_ptr=g_text.data_ptr(), text_cap=size + n,
                                      out_offsets_ptr=g_offs.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        got["new"] = (g_text, g_offs)

    def old_route():
        table.run_lines_select_device(raw.data_ptr(), size, BE, counts.data_ptr(), counts.data_ptr() + 8, out_hits_ptr=hits.data_ptr(),
                                      out_hit_spans_ptr=spans.data_ptr(), hit_cap=cap, stream=stream)
        k = int(counts.cpu()[1])
        hs = spans[:2 * k].cpu().numpy()
        joined, joffs = join_on_host(raw_bytes, hs, k)
        got["old"] = (torch.as_tensor(joined, device="cuda"), torch.as_tensor(joffs, device="cuda"), k)

    new_ms = median_ms(new_route, a.reps)
    kernel = pb.last_kernel()
    old_ms = median_ms(old_route, a.reps)
    torch.cuda.synchronize()
    ot, oo, k = got["old"]
    total = int(counts.cpu()[2])
    same = total == ot.numel() and bool((g_text[:total] == ot).all()) and bool((g_offs[:k + 1] == oo).all())
    out.append("  (b) run_lines_gather, text + offsets left on the device %.3f ms (scan kernel %s)   run_lines_select, hits + spans fetched, "
               "host join, upload %.3f ms" % (new_ms, kernel, old_ms))
    out.append("      hits %d of %d lines (%.3f), %.1f MB gathered, same bytes and offsets %s, old / new = %.1f"
               % (k, n, k / n, total / 1e6, same, old_ms / new_ms))
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines per workload (a quick check of the tool)")
    ap.add_argument("--only-gather", action="store_true", help="(a) alone: the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--trace-db", default="", help="summarise the gather's kernels of a rocprofv3 database into --out, measure nothing")
    a = ap.parse_args()
    if a.trace_db:
        trace_summary(a.trace_db, a.out)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("tools/gather_case.py measures on the GPU: no HIP device here")
    out = ["# tools/gather_case.py: medians of %d warmed repetitions; (a) device events around %d back-to-back calls, (b) host wall clock"
           % (a.reps, a.inner),
           "# around call + synchronise.  The gather reads every selected byte once and writes it once, a newline behind every string."]
    for title, make, n in (("log lines 64..1023 B (set_a)", log_lines, 1 << 20), ("URLs (dict_1k)", urls, 1 << 19),
                           ("log lines with five lines of 1 MiB or more (set_a)", long_lines, 1 << 18)):
        table, raw = make(1 << 16 if a.small and make is long_lines else 1 << 14 if a.small else n)
        table.upload()
        case(title, table, raw, a, out)
        del raw
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
