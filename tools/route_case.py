#!/usr/bin/env python3
"""What one hit list per regexp costs on the device, and what it replaces.

Input: the end states of 2^20 log lines (tools/split_case.py log_lines: the set_a corpus cut into lines of 64..1023 bytes)
under the 8-regexp set_a table, resident on the device.  Device time (events around `--inner` back-to-back enqueue-only
calls, median of `--reps` warmed repetitions, the two sides alternating repetition by repetition) of
  (a) one pire_hip_route pass: all 8 rows and their counts;
  (b) the only way to the same lists without it: 8 pire_hip_select calls, each with a one-bit `want`.
The two answers are compared before anything is timed.  --select-lib PATH: (b) once more in a process of its own that loads
another build of the library (PIRE_HIP_LIB) -- the commit in front of this feature, whose select pass this one keeps as it is.

    python tools/route_case.py [--reps 15] [--inner 20] [--out profiles/route_case.txt] [--small] [--select-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pire_amd import binding as pb  # noqa: E402
from split_case import log_lines  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def end_states(n):
    """(table, int32[n] end states on the device) of n log lines, scanned by the library itself"""
    table, raw = log_lines(n)
    stream = torch.cuda.current_stream().cuda_stream
    size = raw.numel()
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    table.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_idx_ptr=idx.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n
    return table, idx


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def measure(a):
    n = 1 << 16 if a.small else 1 << 20
    table, idx = end_states(n)
    regexps = table.RegexpsCount
    stream = torch.cuda.current_stream().cuda_stream
    wants = [torch.as_tensor(table.want_mask([r]).view(np.int64), device="cuda") for r in range(regexps)]
    sel_hits = torch.zeros((regexps, n), dtype=torch.int64, device="cuda")
    sel_counts = torch.zeros(regexps, dtype=torch.int64, device="cuda")
    hits = torch.zeros((regexps, n), dtype=torch.int64, device="cuda")
    counts = torch.zeros(regexps, dtype=torch.int64, device="cuda")

    def selects():
        for r in range(regexps):
            table.select_device(idx.data_ptr(), n, sel_counts.data_ptr() + 8 * r, want_ptr=wants[r].data_ptr(),
                                out_hits_ptr=sel_hits.data_ptr() + 8 * n * r, hit_cap=n, stream=stream)

    res = {"n": n, "regexps": regexps}
    have_route = hasattr(pb.lib(), "pire_hip_route")
    sides = {"select_x%d" % regexps: selects}
    if have_route and not a.select_only:
        sides["route"] = lambda: table.route_device(idx.data_ptr(), n, counts.data_ptr(), out_hits_ptr=hits.data_ptr(), hit_cap=n,
                                                    stream=stream)
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if "route" in sides:
        c, sc = counts.cpu().numpy(), sel_counts.cpu().numpy()
        same = (c == sc).all() and all((hits[r, :c[r]] == sel_hits[r, :c[r]]).all().item() for r in range(regexps))
        res["same_answer"] = bool(same)
        res["counts"] = c.tolist()
    samples = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            samples[k].append(timed(fn, a.inner))
    for k, v in samples.items():
        res[k + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 strings (a quick check of the tool)")
    ap.add_argument("--select-lib", default="", help="another build of the library: its 8 select calls, in a process of its own")
    ap.add_argument("--select-only", action="store_true", help="(the child of --select-lib) time the select calls, print JSON")
    a = ap.parse_args()
    res = measure(a)
    if a.select_only:
        print(json.dumps(res))
        return 0
    fmt = lambda m: "%.4f ms (min %.4f, max %.4f)" % (m["median"], m["min"], m["max"])   # noqa: E731
    sel_key = "select_x%d" % res["regexps"]
    out = ["# tools/route_case.py: device events around %d back-to-back enqueue-only calls, median (min, max) of %d warmed"
           % (a.inner, a.reps),
           "# repetitions, the two sides alternating; input: end states of %d log lines (set_a, %d regexps), resident" % (res["n"], res["regexps"]),
           "hits per regexp %s   same answer %s" % (res["counts"], res["same_answer"]),
           "(a) one pire_hip_route pass (3 kernels, 1 scratch allocation):          %s" % fmt(res["route_ms"]),
           "(b) %d pire_hip_select calls, one-bit want (%d kernels, %d allocations): %s"
           % (res["regexps"], 3 * res["regexps"], res["regexps"], fmt(res[sel_key + "_ms"])),
           "(b) / (a) = %.2f" % (res[sel_key + "_ms"]["median"] / res["route_ms"]["median"])]
    ok = res["same_answer"]
    if a.select_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--select-only", "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), env=dict(os.environ, PIRE_HIP_LIB=os.path.abspath(a.select_lib)),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("the --select-lib process failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        other = json.loads(r.stdout.strip().splitlines()[-1])
        out.append("(b') the same %d calls on %s, a process of its own:  %s"
                   % (res["regexps"], os.path.relpath(os.path.abspath(a.select_lib), ROOT), fmt(other[sel_key + "_ms"])))
        out.append("(b') / (a) = %.2f" % (other[sel_key + "_ms"]["median"] / res["route_ms"]["median"]))
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
