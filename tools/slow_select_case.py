#!/usr/bin/env python3
"""What turning a SlowScanner's Final flags into hit lists and matching lines on the device costs, and what it replaces
(DESIGN.md section 4.18).

2^20 log lines resident on the device -- the corpus of tools/split_case.py (the synthetic corpus of set_a cut into lines of
64..1023 bytes), an `x` planted 41 bytes in front of the end of every third line --, scanned by the slow_x40_utf8 SlowScanner
(x.{40}$, UTF-8: BASELINE config 5b's).  Medians (and the spread, min..max) of warmed repetitions:
  (a) pire_hip_final_select alone, device pointers, on the flags the scan left on the device, in both modes: device events
      around `--inner` back-to-back calls; next to it pire_hip_select on the same n (the end states of the set_a scanner on the
      same lines, hits only), timed in the same run;
  (b) pire_hip_slow_run alone against pire_hip_slow_run_select with the flags in scratch (what the pass adds to the scan);
  (c) pire_hip_slow_lines_select and pire_hip_slow_lines_gather on the resident raw buffer, everything left on the device,
      against today's route to the same answer: the split on the host (numpy), text and offsets uploaded, pire_hip_slow_run,
      n flag bytes fetched, the threshold and -- for the gather form -- the join of the matching lines in numpy.  Host wall
      clock around call + synchronise.

    python tools/slow_select_case.py [--reps 7] [--inner 10] [--out profiles/slow_select_case.txt] [--small]
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
from pire_amd import workloads as W  # noqa: E402
from capture_select_case import fmt, spread_ms, wall_ms  # noqa: E402
from count_select_case import fixture  # noqa: E402
from split_case import log_lines  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slow_select_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/slow_select_case.py measures on the GPU: no HIP device here")
    stream = torch.cuda.current_stream().cuda_stream
    plain, raw = log_lines(1 << 14 if a.small else 1 << 20, 1234)
    plain.upload()
    slow = pb.SlowTable(W.load_blob(fixture("slow", "slow_x40_utf8")["blob"]))
    size = raw.numel()
    host_raw = raw.cpu().numpy()
    ends = np.flatnonzero(host_raw == 10)
    assert host_raw[-1] == 10
    n = len(ends)
    host_raw[ends[::3] - 41] = ord("x")                          # (lines have 64 bytes or more)
    raw.copy_(torch.as_tensor(host_raw, device="cuda"))
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n
    text_bytes = int(offs.cpu()[n])
    hits = torch.empty(n, dtype=torch.int64, device="cuda")
    fin = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = ["# tools/slow_select_case.py: median (min..max) of %d warmed repetitions; (a), (b) device events around %d back-to-back"
           % (a.reps, a.inner),
           "# calls, (c) host wall clock around call + synchronise",
           "2^20 log lines 64..1023 B (set_a corpus), x.{40}$ UTF-8 (slow_x40_utf8)" if not a.small else "2^14 log lines (--small)",
           "  raw %.1f MB, %d lines" % (size / 1e6, n)]

    # (a) the pass alone, next to pire_hip_select on the same n
    sidx = torch.empty(n, dtype=torch.int32, device="cuda")
    plain.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_idx_ptr=sidx.data_ptr(), stream=stream)

    def scan():
        slow.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_final_ptr=fin.data_ptr(), stream=stream)

    scan()
    torch.cuda.synchronize()
    kernel = pb.last_kernel()
    host_fin = fin.cpu().numpy()
    want = {False: np.flatnonzero(host_fin != 0), True: np.flatnonzero(host_fin == 0)}
    assert len(want[False]) >= n // 3

    def select():
        plain.select_device(sidx.data_ptr(), n, cnt.data_ptr() + 16, out_hits_ptr=hits.data_ptr(), hit_cap=n, stream=stream)

    select_t = spread_ms(select, a.reps, a.inner)
    select_hits = int(cnt.cpu()[2])
    pass_ms = {}
    for invert in (False, True):
        def the_pass(invert=invert):
            pb.final_select_device(fin.data_ptr(), n, cnt.data_ptr() + 8, invert=invert, out_hits_ptr=hits.data_ptr(), hit_cap=n, stream=stream)

        the_pass()
        torch.cuda.synchronize()
        got = int(cnt.cpu()[1])
        assert got == len(want[invert]) and (hits[:got].cpu().numpy() == want[invert]).all(), "the pass's list differs from the host's"
        pass_t = spread_ms(the_pass, a.reps, a.inner)
        pass_ms[invert] = pass_t[0]
        moved = n + 8 * got
        out.append("  (a) pire_hip_final_select, mode %d (flags of pire_hip_slow_run, kernel %s), %d selected (%.1f %%), %.1f MB read + written:"
                   % (int(invert), kernel, got, 100.0 * got / n, moved / 1e6))
        out.append("      %s = %.0f GB/s   pire_hip_select, same n, %d hits (hits only): %s   pass / select %.2f"
                   % (fmt(pass_t), moved / pass_t[0] / 1e6, select_hits, fmt(select_t), pass_t[0] / select_t[0]))

    # (b) what the pass adds to the scan, the flags in scratch
    for invert in (False, True):
        def run_select(invert=invert):
            slow.run_select_device(text.data_ptr(), offs.data_ptr(), n, BE, cnt.data_ptr() + 8, invert=invert, out_hits_ptr=hits.data_ptr(),
                                   hit_cap=n, stream=stream)

        run_select()
        torch.cuda.synchronize()
        assert int(cnt.cpu()[1]) == len(want[invert]) and (hits[:len(want[invert])].cpu().numpy() == want[invert]).all()
        run_t = spread_ms(scan, a.reps, a.inner)
        both_t = spread_ms(run_select, a.reps, a.inner)
        out.append("  (b) pire_hip_slow_run %s = %.0f GB/s of text   pire_hip_slow_run_select, mode %d (flags in scratch) %s   + %.4f ms = %.1f %% = %.1f x the pass alone"
                   % (fmt(run_t), text_bytes / run_t[0] / 1e6, int(invert), fmt(both_t), both_t[0] - run_t[0], 100.0 * (both_t[0] / run_t[0] - 1),
                      (both_t[0] - run_t[0]) / pass_ms[invert]))

    # (c) raw bytes in, matching lines out: one call against the host detour
    spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    out_text = torch.empty(size + n, dtype=torch.uint8, device="cuda")
    out_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    found = {}

    def host_split():
        p = np.flatnonzero(host_raw == 10)
        htext = host_raw[host_raw != 10]
        hoffs = np.zeros(n + 1, dtype=np.int64)
        hoffs[1:] = p - np.arange(n)                                         # (line i ends i newlines further on in raw)
        dt, do = torch.as_tensor(htext, device="cuda"), torch.as_tensor(hoffs, device="cuda")
        slow.run_device(dt.data_ptr(), do.data_ptr(), n, BE, out_final_ptr=fin.data_ptr(), stream=stream)
        return fin.cpu().numpy()                                              # (synchronises; n bytes over PCIe)

    for invert in (False, True):
        k = len(want[invert])

        def lines_select(invert=invert):
            slow.lines_select_device(raw.data_ptr(), size, BE, cnt.data_ptr(), cnt.data_ptr() + 8, invert=invert, out_hits_ptr=hits.data_ptr(),
                                     out_hit_spans_ptr=spans.data_ptr(), hit_cap=n, stream=stream)

        def lines_gather(invert=invert):
            slow.lines_gather_device(raw.data_ptr(), size, BE, cnt.data_ptr(), cnt.data_ptr() + 8, cnt.data_ptr() + 24, invert=invert,
                                     out_hits_ptr=hits.data_ptr(), hit_cap=n, out_text_ptr=out_text.data_ptr(), text_cap=size + n,
                                     out_offsets_ptr=out_offs.data_ptr(), stream=stream)

        def detour_select(invert=invert):
            f = host_split()
            found["hits"] = np.flatnonzero((f != 0) != invert)

        def detour_gather(invert=invert):
            f = host_split()
            sel = np.flatnonzero((f != 0) != invert)
            starts = np.concatenate([[0], ends[:-1] + 1])
            step = np.zeros(size + 1, dtype=np.int8)
            step[starts[sel]] += 1
            step[ends[sel] + 1] -= 1                                          # (the line and its newline)
            found["hits"] = sel
            found["text"] = host_raw[np.cumsum(step[:-1], dtype=np.int8) > 0]

        lines_select()
        torch.cuda.synchronize()
        c = cnt.cpu().numpy()
        assert int(c[0]) == n and int(c[1]) == k and (hits[:k].cpu().numpy() == want[invert]).all()
        detour_select()
        assert (found["hits"] == want[invert]).all(), "the two routes differ"
        lines_gather()
        torch.cuda.synchronize()
        total = int(cnt.cpu()[3])
        detour_gather()
        assert total == len(found["text"]) and (out_text[:total].cpu().numpy() == found["text"]).all(), "the two routes' bytes differ"
        for label, new, old in (("select", lines_select, detour_select), ("gather", lines_gather, detour_gather)):
            new_t = wall_ms(new, a.reps)
            old_t = wall_ms(old, a.reps)
            what = "hits + spans" if label == "select" else "hits + %.1f MB of lines" % (total / 1e6)
            out.append("  (c) pire_hip_slow_lines_%s, mode %d, %d lines (%s), left on the device: %s" % (label, int(invert), k, what, fmt(new_t)))
            out.append("      host split + upload + pire_hip_slow_run, %.1f MB of flags fetched, threshold%s in numpy: %s   old / new %.1f"
                       % (n / 1e6, "" if label == "select" else " and join", fmt(old_t), old_t[0] / new_t[0]))
    result = "\n".join(out) + "\n"
    print(result, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(result)
    return 0


if __name__ == "__main__":
    sys.exit(main())
