#!/usr/bin/env python3
"""What reporting matches on the device costs, and what it replaces ("matches on the device").

Per workload three medians of warmed repetitions, measured in ONE C++ process (tests/cpp/select_host_loop.cpp, built by
`make -C tests/cpp` where the reference headers exist -- the host loop is the reference's own accessor code):
  (a) the scan alone, results left on the device
  (b) pire_hip_run_select with out_hits + out_hit_masks, the hits fetched to the host
  (c) the scan, 5 bytes per string to the host, one Final / AcceptedRegexps lookup per string
Workloads: the headline shape (set_a, 2^20 x 4 KiB, resident) and a URL offsets batch for the dict_1k blacklist scanner.

    python tools/select_case.py [--reps 11] [--out profiles/select_case.txt] [--small]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from pire_amd import binding as pb  # noqa: E402
from pire_amd import workloads as W  # noqa: E402

BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "select_host_loop")


def run(args):
    r = subprocess.run([BIN] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("select_host_loop failed (%d): %s %s" % (r.returncode, r.stdout[-500:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 strings per workload (a quick check of the tool)")
    a = ap.parse_args()
    if not os.path.exists(BIN):
        raise SystemExit(BIN + " is missing: `make -C tests/cpp` builds it where the reference headers exist")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        def put(name, data):
            path = os.path.join(tmp, name)
            with open(path, "wb") as f:
                f.write(data)
            return path

        # the headline shape
        big = W.pattern_set("set_a")
        n, length = (1 << 16 if a.small else 1 << 20), 4096
        res = run([put("set_a.blob", W.load_blob(big["blob"])), "strided", n, length, 1234,
                   put("plants.bin", bytes(W.plants_for(big))), a.reps])
        words = pb.Table(W.load_blob(big["blob"])).mask_words
        lines.append(("set_a, %d x %d B, resident (kernel %s)" % (n, length, res["kernel"]), res, length + 5, words))
        # a URL offsets batch
        entry = W.wide_set("dict_1k")
        nurl = 1 << 16 if a.small else 1 << 19
        text, offs = W.wide_urls(entry, 0x5EED5EED, nurl)
        res = run([put("dict_1k.blob", W.load_blob(entry["blob"])), "offsets", put("urls.txt", text.tobytes()),
                   put("urls.offs", np.ascontiguousarray(offs, dtype=np.uint64).tobytes()), a.reps])
        words = pb.Table(W.load_blob(entry["blob"])).mask_words
        lines.append(("dict_1k, %d URLs, %.1f B on average, offsets on the device (kernel %s)"
                      % (nurl, float(offs[-1]) / nurl, res["kernel"]), res, float(offs[-1]) / nurl + 8 + 5, words))
    out = ["# tools/select_case.py: medians of %d warmed repetitions, host wall clock around call + synchronise, one process" % a.reps,
           "# (a) scan alone  (b) pire_hip_run_select, hits + hit masks fetched to the host  (b') the same, left on the device",
           "# (c) scan + 5 B/string to the host + one Final / AcceptedRegexps lookup per string (the loop of INTEGRATION.md section 2)"]
    ok = True
    for title, r, scan_bytes, w in lines:
        est = (4 + 8 * w) * r["n"] + 8 * (1 + w) * r["hits"]
        out.append(title)
        out.append("  strings %d  hits %d  hit rate %.4f  same answer %s" % (r["n"], r["hits"], r["hit_rate"], r["same_answer"]))
        out.append("  (a) %.4f ms   (b) %.4f ms   (b') %.4f ms   (c) %.4f ms" % (r["scan_ms"], r["run_select_ms"],
                                                                              r["run_select_on_device_ms"], r["host_loop_ms"]))
        out.append("  select passes on the device: (b') - (a) = %.4f ms for an estimated %.2f MB read + written (the scan reads %.0f MB)"
                   % (r["run_select_on_device_ms"] - r["scan_ms"], est / 1e6, scan_bytes * r["n"] / 1e6))
        out.append("  (b) / (c) = %.3f" % (r["run_select_ms"] / r["host_loop_ms"]))
        ok = ok and r["run_select_ms"] <= r["host_loop_ms"] and r["same_answer"]
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
