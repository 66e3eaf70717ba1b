#!/usr/bin/env python3
"""What a boolean query over hit lists costs on the device, and what it replaces.

  (a) the pass alone: pire_hip_combine over 2^20 lines, k_lists = 2 and 6, lists of 1 % and of 50 % of the lines drawn at
      random, a truth table drawn at random (bit 0 cleared) -- hits, member bytes and the count written -- beside its sister
      passes on the same n: pire_hip_context (before = after = 0: the first list comes back) and pire_hip_select (state index
      0 for every string: its cost does not depend on the states), and beside the same answer from lists fetched and combined
      with NumPy.  The device sides: device events around `--inner` back-to-back enqueue-only calls; the NumPy side: host wall
      clock around the copies and the combination; median of `--reps` warmed repetitions, the sides alternating.
  (b) the lines form: pire_hip_lines_combine_select with two terms on 2^20 log lines (tools/split_case.py log_lines: the set_a
      corpus cut into lines of 64..1023 bytes), resident on the device -- term 0: the table's Final lines, term 1: the lines of
      regexps 5..7, "the first and not the second" --, hits and members left on the device, beside what a caller does without
      it: one pire_hip_run_lines_select per term on the device, both lists fetched, combined with NumPy.  Host wall clock
      around calls that end in a synchronise, median of `--reps`, alternating.
The answers are compared with the NumPy formula before anything is timed.  With --trace-only the tool makes `--inner` calls of
every device side of (a) and exits: for a `rocprofv3 --kernel-trace --stats` run of its own.

    python tools/combine_case.py [--reps 7] [--inner 10] [--out profiles/combine_case.txt] [--small] [--trace-only]
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


def combine(lists, n, truth):
    """include/pire_hip.h: the selected lines and their member masks"""
    i = np.arange(n, dtype=np.int64)
    m = np.zeros(n, dtype=np.int64)
    for j, l in enumerate(lists):
        m |= np.isin(i, l, assume_unique=True).astype(np.int64) << j
    hits = np.flatnonzero((np.uint64(truth) >> m.astype(np.uint64)) & np.uint64(1))
    return hits, m[hits].astype(np.uint8)


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


def alternate(sides, reps):
    """sides: name -> (fn, clock)"""
    for fn, _ in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in sides}
    for _ in range(reps):
        for k, (fn, once) in sides.items():
            samples[k].append(once(fn))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    ap.add_argument("--trace-only", action="store_true", help="the device sides of (a), --inner calls each, nothing timed or written")
    a = ap.parse_args()
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    i64 = dict(dtype=torch.int64, device="cuda")
    be = pb.FLAG_BEGIN | pb.FLAG_END
    table, raw = log_lines(n)
    size = raw.numel()
    fmt = lambda m: "%.4f ms (min %.4f, max %.4f)" % m   # noqa: E731
    out = ["# tools/combine_case.py: %d lines; (a) lists drawn at random; (b) %.1f MB of log lines, resident, table set_a" % (n, size / 1e6),
           "# (a) device events around %d back-to-back enqueue-only calls, the NumPy side and (b) host wall clock around calls that end in a"
           % a.inner,
           "# synchronise; median (min, max) of %d warmed repetitions, the sides alternating, one run" % a.reps]
    same = True

    # (a) the pass alone
    hits, members = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.uint8, device="cuda")
    c_lines, c_flags = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.uint8, device="cuda")
    s_hits, idx = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, **i64)
    for density in (100, 2):
        for k in (2, 6):
            rng = np.random.RandomState(1000 * density + k)
            lists_np = [np.flatnonzero(rng.randint(0, density, size=n) == 0) for _ in range(k)]
            lists = [torch.as_tensor(l, device="cuda") for l in lists_np]
            truth = (int(rng.randint(0, 1 << 32)) | (int(rng.randint(0, 1 << 32)) << 32)) & ((1 << (1 << k)) - 1) & ~1
            ptrs, caps = [l.data_ptr() for l in lists], [len(l) for l in lists_np]

            def on_device():
                pb.combine_device(ptrs, caps, n, truth, counts.data_ptr(), out_hits_ptr=hits.data_ptr(), out_hit_members_ptr=members.data_ptr(),
                                  hit_cap=n, stream=stream)

            def context():
                pb.context_device(ptrs[0], caps[0], n, counts[1:].data_ptr(), 0, 0, out_lines_ptr=c_lines.data_ptr(),
                                  out_line_flags_ptr=c_flags.data_ptr(), line_cap=n, out_group_count_ptr=counts[2:].data_ptr(), stream=stream)

            def select():
                table.select_device(idx.data_ptr(), n, counts[3:].data_ptr(), out_hits_ptr=s_hits.data_ptr(), hit_cap=n, stream=stream)

            got = [None]

            def by_numpy():
                got[0] = combine([l.cpu().numpy() for l in lists], n, truth)

            if a.trace_only:
                for fn in (on_device, context, select):
                    for _ in range(a.inner):
                        fn()
                torch.cuda.synchronize()
                continue
            on_device()
            by_numpy()
            torch.cuda.synchronize()
            count = int(counts.cpu()[0])
            ok = count == len(got[0][0]) and (hits[:count].cpu().numpy() == got[0][0]).all() and (members[:count].cpu().numpy() == got[0][1]).all()
            same = same and bool(ok)
            ms = alternate({"combine": (on_device, lambda fn: event_ms(fn, a.inner)), "context": (context, lambda fn: event_ms(fn, a.inner)),
                            "select": (select, lambda fn: event_ms(fn, a.inner)), "numpy": (by_numpy, wall_ms)}, a.reps)
            out += ["(a) k_lists = %d, %.0f %% of the lines in every list, %d lines selected, same answer as NumPy: %s" % (k, 100.0 / density, count, bool(ok)),
                    "    pire_hip_combine, hits + members + count:                  %s" % fmt(ms["combine"]),
                    "    pire_hip_context on list 0, before = after = 0:            %s" % fmt(ms["context"]),
                    "    pire_hip_select on the same n:                             %s" % fmt(ms["select"]),
                    "    %d lists (%.1f MB) fetched, np.isin per list, table lookup:  %s" % (k, 8.0 * sum(caps) / 1e6, fmt(ms["numpy"])),
                    "    combine / context = %.2f, combine / select = %.2f, NumPy / combine = %.0f"
                    % (ms["combine"][0] / ms["context"][0], ms["combine"][0] / ms["select"][0], ms["numpy"][0] / ms["combine"][0])]
    if a.trace_only:
        return 0

    # (b) the lines form against one lines call per term and the host's combination
    want = torch.as_tensor(table.want_mask([5, 6, 7]).view(np.int64), device="cuda")
    terms = [pb.line_term(table=table), pb.line_term(table=table, want_ptr=want.data_ptr())]
    truth = pb.truth(2, lambda m: m == 1)
    f_words, f_terms = torch.zeros(2, **i64), torch.zeros(2, **i64)
    g_hits, g_words = torch.zeros((2, n), **i64), torch.zeros(4, **i64)
    answer = [None]

    def fused():
        pb.lines_combine_device(terms, truth, raw.data_ptr(), size, f_words.data_ptr(), f_words[1:].data_ptr(), out_hits_ptr=hits.data_ptr(),
                                out_hit_members_ptr=members.data_ptr(), hit_cap=n, out_term_counts_ptr=f_terms.data_ptr(), stream=stream)

    def by_hand():
        for j, w in enumerate((0, want.data_ptr())):
            table.run_lines_select_device(raw.data_ptr(), size, be, g_words[2 * j:].data_ptr(), g_words[2 * j + 1:].data_ptr(), want_ptr=w,
                                          out_hits_ptr=g_hits[j].data_ptr(), hit_cap=n, stream=stream)
        c = g_words.cpu().tolist()
        answer[0] = combine([g_hits[0, :c[1]].cpu().numpy(), g_hits[1, :c[3]].cpu().numpy()], n, truth)

    fused()
    by_hand()
    torch.cuda.synchronize()
    lines_n, count = f_words.cpu().tolist()
    ok = lines_n == n and count == len(answer[0][0]) and (hits[:count].cpu().numpy() == answer[0][0]).all()
    same = same and bool(ok)
    ms = alternate({"fused": (fused, wall_ms), "by_hand": (by_hand, wall_ms)}, a.reps)
    out += ["(b) two terms (Final: %d lines; regexps 5..7: %d lines), the first and not the second: %d lines, same answer: %s"
            % (tuple(f_terms.cpu().tolist()) + (count, bool(ok))),
            "    pire_hip_lines_combine_select, one call, hits and members left on the device:        %s" % fmt(ms["fused"]),
            "    two pire_hip_run_lines_select, both lists fetched, np.isin and the table on the host: %s" % fmt(ms["by_hand"]),
            "    by hand / fused = %.2f" % (ms["by_hand"][0] / ms["fused"][0])]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
