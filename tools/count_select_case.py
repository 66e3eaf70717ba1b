#!/usr/bin/env python3
"""What turning counted matches into hit lists and totals on the device costs, and what it replaces.

2^20 log lines resident on the device -- the corpus of tools/gather_case.py (the synthetic corpus of set_a cut into lines of
64..1023 bytes) --, scanned by the count_glued3_advanced counting scanner (R = 3) and the half_5 HalfFinalScanner (R = 5).
The thresholds: one regexp asked -- the (regexp, threshold) that selects nearest to half of the lines --, the others not.
Medians (and the spread, min..max) of warmed repetitions:
  (a) pire_hip_count_select alone, device pointers, on the rows the scan left on the device, totals + hits + hit rows, for
      R = 3 and R = 5: device events around `--inner` back-to-back calls, in bytes read + written per second (4 R bytes in per
      string, 8 + 4 R out per selected string); next to it pire_hip_select on the same n (the end states of the set_a scanner
      on the same lines, hits only) and a device-to-device copy of the same number of bytes, timed in the same run;
  (b) pire_hip_counting_run alone against pire_hip_counting_run_select with the rows in scratch, and the same for
      pire_hip_run_half_final (what the pass adds to a scan);
  (c) pire_hip_counting_lines_select on the resident raw buffer, everything left on the device, against today's route: the
      split and pire_hip_counting_run on the device, n * R * 4 bytes fetched, the threshold in numpy.  Host wall clock around
      call + synchronise.

    python tools/count_select_case.py [--reps 7] [--inner 10] [--out profiles/count_select_case.txt] [--small]
"""
import argparse
import json
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
from split_case import log_lines  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def fixture(group, name):
    with open(os.path.join(W.GOLDEN, "cases.json")) as f:
        return [c for c in json.load(f)[group] if c["name"] == name][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_select_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/count_select_case.py measures on the GPU: no HIP device here")
    stream = torch.cuda.current_stream().cuda_stream
    plain, raw = log_lines(1 << 14 if a.small else 1 << 20, 1234)
    plain.upload()
    cf = fixture("counting", "count_glued3_advanced")
    counting = pb.CountingTable(W.load_blob(cf["blob"]), cf["kind"])
    half = pb.Table(W.load_blob(fixture("half_final", "half_5")["blob"]))
    size = raw.numel()
    host_raw = raw.cpu().numpy()
    n = int((host_raw == 10).sum()) + (1 if host_raw[-1] != 10 else 0)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    text_bytes = int(offs.cpu()[n])
    hits = torch.empty(n, dtype=torch.int64, device="cuda")
    out = ["# tools/count_select_case.py: median (min..max) of %d warmed repetitions; (a), (b) device events around %d back-to-back"
           % (a.reps, a.inner),
           "# calls, (c) host wall clock around call + synchronise",
           "2^20 log lines 64..1023 B (set_a corpus)" if not a.small else "2^14 log lines (--small)",
           "  raw %.1f MB, %d lines" % (size / 1e6, n)]
    sidx = torch.empty(n, dtype=torch.int32, device="cuda")
    plain.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_idx_ptr=sidx.data_ptr(), stream=stream)
    torch.cuda.synchronize()

    def select():
        plain.select_device(sidx.data_ptr(), n, cnt.data_ptr() + 16, out_hits_ptr=hits.data_ptr(), hit_cap=n, stream=stream)

    select_t = spread_ms(select, a.reps, a.inner)
    select_hits = int(cnt.cpu()[2])
    pass_ms, scans = {}, {}
    for label, tab, R in (("pire_hip_counting_run", counting, 3), ("pire_hip_run_half_final", half, 5)):
        res = torch.empty(n * R, dtype=torch.int32, device="cuda")
        rows = torch.empty(n * R, dtype=torch.int32, device="cuda")
        totals = torch.zeros(R, dtype=torch.int64, device="cuda")

        def scan(tab=tab, res=res):
            if tab is counting:
                tab.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_results_ptr=res.data_ptr(), stream=stream)
            else:
                tab.run_half_final_device(text.data_ptr(), offs.data_ptr(), n, BE, out_results_ptr=res.data_ptr(), stream=stream)

        scan()
        torch.cuda.synchronize()
        kernel = pb.last_kernel()
        host = res.cpu().numpy().view(np.uint32).reshape(n, R)
        # one regexp asked, the others not: the (regexp, threshold) whose share of the lines is nearest to a half
        share, col, least = min((abs(float((host[:, r] >= t).mean()) - 0.5), r, t) for r in range(R)
                                for t in sorted({max(1, int(np.percentile(host[:, r], q)) + d) for q in (25, 50, 75, 90) for d in (0, 1)}))
        m = np.zeros(R, dtype=np.uint32)
        m[col] = least
        dmin = torch.as_tensor(m.view(np.int32), device="cuda")
        want = np.flatnonzero(host[:, col] >= least)

        def the_pass(res=res, R=R, dmin=dmin, totals=totals, rows=rows):
            pb.count_select_device(res.data_ptr(), n, R, cnt.data_ptr() + 8, min_count_ptr=dmin.data_ptr(), out_totals_ptr=totals.data_ptr(),
                                   out_hits_ptr=hits.data_ptr(), out_hit_results_ptr=rows.data_ptr(), hit_cap=n, stream=stream)

        the_pass()
        torch.cuda.synchronize()
        got = int(cnt.cpu()[1])
        assert got == len(want) and (hits[:got].cpu().numpy() == want).all(), "the pass's list differs from the host's"
        assert (totals.cpu().numpy() == host.astype(np.uint64).sum(axis=0).astype(np.int64)).all(), "the pass's totals differ from the host's"
        assert (rows[:got * R].cpu().numpy().view(np.uint32).reshape(got, R) == host[want]).all()
        moved = 4 * R * n + (8 + 2 * 4 * R) * got             # the rows; hits, and the hit rows read again and written
        pass_t = spread_ms(the_pass, a.reps, a.inner)
        src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
        copy_t = spread_ms(lambda: dst.copy_(src), a.reps, a.inner)
        pass_ms[R] = pass_t[0]
        out.append("  (a) pire_hip_count_select R = %d (rows of %s, kernel %s; min_count[%d] = %d), totals + hits + hit rows, %d selected (%.1f %%),"
                   % (R, label, kernel, col, least, got, 100.0 * got / n))
        out.append("      %.1f MB read + written: %s = %.0f GB/s" % (moved / 1e6, fmt(pass_t), moved / pass_t[0] / 1e6))
        out.append("      pire_hip_select, same n, %d hits (hits only): %s   pass / select %.2f" % (select_hits, fmt(select_t), pass_t[0] / select_t[0]))
        out.append("      device-to-device copy of %.1f MB: %s = %.0f GB/s   pass / copy %.2f"
                   % (moved / 1e6, fmt(copy_t), moved / copy_t[0] / 1e6, pass_t[0] / copy_t[0]))
        scans[R] = (label, tab, scan, dmin, totals, rows, m, want)

    # (b) what the pass adds to a scan, the rows in scratch
    for R in (3, 5):
        label, tab, scan, dmin, totals, rows, m, want = scans[R]

        def run_select(tab=tab, dmin=dmin, totals=totals, rows=rows):
            kw = dict(min_count_ptr=dmin.data_ptr(), out_totals_ptr=totals.data_ptr(), out_hits_ptr=hits.data_ptr(),
                      out_hit_results_ptr=rows.data_ptr(), hit_cap=n, stream=stream)
            if tab is counting:
                tab.run_select_device(text.data_ptr(), offs.data_ptr(), n, BE, cnt.data_ptr() + 8, **kw)
            else:
                tab.run_half_final_select_device(text.data_ptr(), offs.data_ptr(), n, BE, cnt.data_ptr() + 8, **kw)

        run_select()
        torch.cuda.synchronize()
        assert int(cnt.cpu()[1]) == len(want)
        run_t = spread_ms(scan, a.reps, a.inner)
        both_t = spread_ms(run_select, a.reps, a.inner)
        out.append("  (b) %s %s = %.0f GB/s of text   %s_select (rows in scratch) %s   + %.4f ms = %.1f %% = %.1f x the pass alone"
                   % (label, fmt(run_t), text_bytes / run_t[0] / 1e6, label, fmt(both_t), both_t[0] - run_t[0], 100.0 * (both_t[0] / run_t[0] - 1),
                      (both_t[0] - run_t[0]) / pass_ms[R]))

    # (c) raw bytes in, counted lines out: one call against the host detour
    label, tab, scan, dmin, totals, rows, m, want = scans[3]
    spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    res3 = torch.empty(n * 3, dtype=torch.int32, device="cuda")

    def fused():
        counting.lines_select_device(raw.data_ptr(), size, BE, cnt.data_ptr(), cnt.data_ptr() + 8, min_count_ptr=dmin.data_ptr(),
                                     out_totals_ptr=totals.data_ptr(), out_hits_ptr=hits.data_ptr(), out_hit_spans_ptr=spans.data_ptr(),
                                     out_hit_results_ptr=rows.data_ptr(), hit_cap=n, stream=stream)

    fused()
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert int(c[0]) == n and int(c[1]) == len(want) and (hits[:len(want)].cpu().numpy() == want).all()
    found = {}

    def detour():
        pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
        counting.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_results_ptr=res3.data_ptr(), stream=stream)
        h = res3.cpu().numpy().view(np.uint32).reshape(n, 3)                          # (synchronises; n * R * 4 bytes over PCIe)
        found["hits"] = np.flatnonzero((h >= np.maximum(m, 1)[None, :])[:, m > 0].any(axis=1))
        found["totals"] = h.sum(axis=0, dtype=np.uint64)

    detour()
    assert (found["hits"] == want).all(), "the two routes differ"
    fused_t = wall_ms(fused, a.reps)
    detour_t = wall_ms(detour, a.reps)
    out.append("  (c) pire_hip_counting_lines_select, %d counted lines (hits, spans, rows, totals), left on the device: %s" % (len(want), fmt(fused_t)))
    out.append("      split + counting_run on the device, %.1f MB of rows fetched, threshold and totals on the host (numpy): %s   old / new %.1f"
               % (n * 12 / 1e6, fmt(detour_t), detour_t[0] / fused_t[0]))
    result = "\n".join(out) + "\n"
    print(result, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(result)
    return 0


if __name__ == "__main__":
    sys.exit(main())
