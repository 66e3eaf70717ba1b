#!/usr/bin/env python3
"""What Pire::SlowCapturingScanner costs on the device, and against the reference itself.

2^20 log lines resident on the device -- the corpus of tools/split_case.py (the synthetic corpus of set_a cut into lines of
64..1023 bytes), `id=<digits>&` planted in every third line and an `a`, 70 bytes on, a `b` in every third of the others --,
under two tables of tests/golden/slow_capture: `id` (.*?id=(\\d+?)\\d*&, 30 states) and `wide` (.*?(a.{70}b), 368 states).
Medians (and the spread, min..max) of warmed repetitions:
  (a) pire_hip_slow_capture_run alone, device pointers: device events around `--inner` back-to-back calls;
  (b) pire_hip_slow_capture_run_select with the positions in scratch, the same way;
  (c) pire_hip_slow_capture_lines_gather on the resident raw buffer, everything left on the device: host wall clock around
      call + synchronise;
  (d) the yardstick: the reference's own walk on ONE core over the first `--ref-lines` of the same lines
      (oracle/_ref/bin/slow_capture_golden --time: tests/cpp/slow_capture_golden.cpp), its number of captures and the sum of
      their positions held against the device's on those lines, and its rate scaled by 16 -- the reference spread perfectly
      over sixteen cores.  The tool FAILS unless the device scan (a) is faster than that.

    python tools/slow_capture_case.py [--reps 5] [--inner 3] [--ref-lines 20000] [--out profiles/slow_capture_case.txt] [--small]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pire_amd import binding as pb  # noqa: E402
from capture_select_case import fmt, spread_ms, wall_ms  # noqa: E402
from split_case import log_lines  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "slow_capture")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "slow_capture_golden")


def case(name):
    with open(os.path.join(GOLDEN, "cases.json")) as f:
        c = [c for c in json.load(f)["cases"] if c["name"] == name][0]
    with open(os.path.join(GOLDEN, c["blob"]), "rb") as f:
        return c, f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--ref-lines", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slow_capture_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/slow_capture_case.py measures on the GPU: no HIP device here")
    stream = torch.cuda.current_stream().cuda_stream
    _, raw = log_lines(1 << 14 if a.small else 1 << 20, 1234)
    size = raw.numel()
    host = raw.cpu().numpy()
    ends = np.flatnonzero(host == 10)
    assert host[-1] == 10
    n = len(ends)
    starts = np.concatenate([[0], ends[:-1] + 1])
    host[host == ord("&")] = ord("+")                              # the planted `&` is the only one of its line
    wit = np.frombuffer(b"id=12345&", dtype=np.uint8)
    for i in range(0, n, 3):                                        # (lines have 64 bytes or more)
        at = starts[i] + (int(ends[i] - starts[i]) - len(wit)) * (i % 7) // 7
        host[at:at + len(wit)] = wit
    for i in range(1, n, 9):
        if ends[i] - starts[i] >= 80:
            host[starts[i] + 3], host[starts[i] + 74] = ord("a"), ord("b")
    raw.copy_(torch.as_tensor(host, device="cuda"))
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n
    text_bytes = int(offs.cpu()[n])
    captured = torch.empty(n, dtype=torch.uint8, device="cuda")
    begin = torch.empty(n, dtype=torch.int64, device="cuda")
    end = torch.empty(n, dtype=torch.int64, device="cuda")
    hits = torch.empty(n, dtype=torch.int64, device="cuda")
    spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    out_text = torch.empty(size + n, dtype=torch.uint8, device="cuda")
    out_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    out = ["# tools/slow_capture_case.py: median (min..max) of %d warmed repetitions; (a), (b) device events around %d back-to-back"
           % (a.reps, a.inner),
           "# calls, (c) host wall clock around call + synchronise, (d) the reference's walk on one core",
           "2^20 log lines 64..1023 B (set_a corpus)" if not a.small else "2^14 log lines (--small)",
           "  raw %.1f MB, %d lines, %.1f MB of text" % (size / 1e6, n, text_bytes / 1e6)]
    ref_n = min(a.ref_lines, n)
    failed = False
    for name, ref_lines in (("id", ref_n), ("wide", max(1, ref_n // 10))):
        c, blob = case(name)
        t = pb.SlowCaptureTable(blob)
        out.append("%s: %s, %d states, %d list entries, longest list %d" % (name, bytes.fromhex(c["pattern_hex"]).decode(), t.info.states,
                                                                          t.info.entries, t.info.longest_list))

        def scan():
            t.run_device(text.data_ptr(), offs.data_ptr(), n, captured.data_ptr(), begin.data_ptr(), end.data_ptr(), 0, 0, stream)

        def run_select():
            t.run_select_device(text.data_ptr(), offs.data_ptr(), n, cnt.data_ptr() + 8, out_hits_ptr=hits.data_ptr(),
                                out_spans_ptr=spans.data_ptr(), hit_cap=n, stream=stream)

        def lines_gather():
            t.lines_gather_device(raw.data_ptr(), size, cnt.data_ptr(), cnt.data_ptr() + 8, cnt.data_ptr() + 24, out_hits_ptr=hits.data_ptr(),
                                  out_spans_ptr=spans.data_ptr(), hit_cap=n, out_text_ptr=out_text.data_ptr(), text_cap=size + n,
                                  out_offsets_ptr=out_offs.data_ptr(), stream=stream)

        scan()
        torch.cuda.synchronize()
        assert pb.last_kernel() == "slow_capture"
        cap_h, b_h, e_h = captured.cpu().numpy(), begin.cpu().numpy(), end.cpu().numpy()
        k = int(np.count_nonzero(cap_h))
        run_select()
        torch.cuda.synchronize()
        assert int(cnt.cpu()[1]) == k and (hits[:k].cpu().numpy() == np.flatnonzero(cap_h)).all()
        lines_gather()
        torch.cuda.synchronize()
        got = cnt.cpu().numpy()
        assert int(got[0]) == n and int(got[1]) == k
        sel = np.flatnonzero(cap_h)
        assert (spans[:2 * k].cpu().numpy().reshape(-1, 2) == np.stack([starts[sel] + b_h[sel], starts[sel] + e_h[sel]], axis=1)).all()
        scan_t = spread_ms(scan, a.reps, a.inner)
        select_t = spread_ms(run_select, a.reps, a.inner)
        gather_t = wall_ms(lines_gather, a.reps)
        rate = text_bytes / scan_t[0] / 1e3                                   # MB/s
        out.append("  (a) pire_hip_slow_capture_run, %d of %d lines capture (%.1f %%): %s = %.1f MB/s of text"
                   % (k, n, 100.0 * k / n, fmt(scan_t), rate))
        out.append("  (b) pire_hip_slow_capture_run_select (positions in scratch, hits + spans): %s   + %.4f ms" % (fmt(select_t), select_t[0] - scan_t[0]))
        out.append("  (c) pire_hip_slow_capture_lines_gather, %d captured fields, %.2f MB gathered, left on the device: %s"
                   % (k, int(got[3]) / 1e6, fmt(gather_t)))
        # (d) the yardstick
        if not os.path.exists(REF_BIN):
            out.append("  (d) %s is not built: no yardstick, the condition is NOT checked" % os.path.relpath(REF_BIN, ROOT))
            failed = True
            continue
        with tempfile.NamedTemporaryFile(suffix=".txt") as f:
            f.write(host[:ends[ref_lines - 1] + 1].tobytes())
            f.flush()
            r = subprocess.run([REF_BIN, "--time", c["pattern_hex"], str(c["index"]), f.name], stdout=subprocess.PIPE, text=True, check=True)
        lines_, bytes_, ref_cap, seconds, ref_sum = r.stdout.split()
        ref_rate = (int(bytes_) - int(lines_)) / float(seconds) / 1e6
        same = (int(lines_) == ref_lines and int(ref_cap) == int(np.count_nonzero(cap_h[:ref_lines]))
                and int(ref_sum) == int((b_h[:ref_lines] + e_h[:ref_lines])[cap_h[:ref_lines] != 0].sum()))
        ok = rate > 16 * ref_rate
        out.append("  (d) the reference on one core, the first %d lines: %.2f s = %.3f MB/s; captures and positions %s the device's"
                   % (ref_lines, float(seconds), ref_rate, "equal" if same else "DIFFER FROM"))
        out.append("      16 x the reference = %.2f MB/s; the device scan is %.0f x the reference, %.1f x the 16-core yardstick: condition %s"
                   % (16 * ref_rate, rate / ref_rate, rate / (16 * ref_rate), "met" if ok else "NOT MET"))
        out.append("      the lines form against the reference's rate on all %d lines: %.1f ms against %.0f s" % (n, gather_t[0], text_bytes / 1e6 / ref_rate))
        failed = failed or not ok or not same
    result = "\n".join(out) + "\n"
    print(result, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(result)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
