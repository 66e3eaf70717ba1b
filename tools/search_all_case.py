#!/usr/bin/env python3
"""What every match of every line costs on the device, beside the first match alone.

Input: tools/search_case.py's -- 2^20 log lines of 64..1023 bytes, resident on the device, split once, an IPv4-like address in
every third line.  Two pairs of tests/golden/search: `ipv4` (a match in every third line) and `num` (several in every line).
  (a)  pire_hip_search_all with rows, owners and spans: the marks of one backward pass, the forward leg over them, the lists.
  (b)  pire_hip_search_run_select on the same text: the first match only -- the floor, and the code this one was added to.
  (c)  pire_hip_suffix with R alone: the backward leg, every byte read once.
  (a') pire_hip_search_all_lines_gather on the raw buffer, spans only: host wall clock, it splits the buffer itself.
  (d)  re.finditer on the host over the same bytes, one pass (both patterns mean the same to POSIX and to Python).
(a), (b), (c): device events around `--inner` back-to-back enqueue-only calls; (a'): host wall clock around a call that ends in
a synchronise; median (min, max) of `--reps` warmed repetitions, the sides alternating repetition by repetition, one run.  (d)
is timed once.  All sides that answer the same question are compared before anything is timed: (a') and (d) span by span, (a)
and (a') span by span (line i lies i bytes further into raw), the first match of every row of (a) with (b), the lines with a
match with (c).

    python tools/search_all_case.py [--reps 7] [--inner 3] [--out profiles/search_all_case.txt] [--small]
"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pire_amd  # noqa: E402
from pire_amd import binding as pb  # noqa: E402
from search_case import ADDRESS, alternate, blob, event_ms, lines_with_addresses, wall_ms  # noqa: E402

PATTERNS = {"ipv4": rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}", "num": rb"[0-9]+"}


def measure(name, raw, text, offs, n, text_bytes, a):
    stream = torch.cuda.current_stream().cuda_stream
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")
    rev, fwd = pire_amd.Table(blob(name + ".nr.blob")), pire_amd.Table(blob(name + ".n.blob"))
    words = torch.zeros(8, **i64)
    # how many there are: the call with no room says so
    pb.search_all_device(rev, fwd, text.data_ptr(), text_bytes, offs.data_ptr(), n, words.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    count = int(words.cpu()[0])
    cap = count + 1
    a_rows, a_owners, a_spans = torch.zeros(n + 1, **i64), torch.zeros(cap, **i64), torch.zeros((cap, 2), **i64)
    b_hits, b_spans = torch.zeros(n, **i64), torch.zeros((n, 2), **i64)
    c_len = torch.empty(n, **i64)
    f_owners, f_spans = torch.zeros(cap, **i64), torch.zeros((cap, 2), **i64)

    def every():
        pb.search_all_device(rev, fwd, text.data_ptr(), text_bytes, offs.data_ptr(), n, words.data_ptr(), out_rows_ptr=a_rows.data_ptr(),
                             out_owners_ptr=a_owners.data_ptr(), out_spans_ptr=a_spans.data_ptr(), match_cap=cap, stream=stream)

    def first():
        pb.search_run_select_device(rev, fwd, text.data_ptr(), offs.data_ptr(), n, words[1:].data_ptr(), out_hits_ptr=b_hits.data_ptr(),
                                    out_spans_ptr=b_spans.data_ptr(), hit_cap=n, stream=stream)

    def floor():
        rev.suffix_device(text.data_ptr(), offs.data_ptr(), n, True, c_len.data_ptr(), stream=stream)

    def every_lines():
        pb.search_all_lines_gather_device(rev, fwd, raw.data_ptr(), size, words[2:].data_ptr(), words[3:].data_ptr(),
                                          out_owners_ptr=f_owners.data_ptr(), out_spans_ptr=f_spans.data_ptr(), match_cap=cap, stream=stream)

    every(), first(), floor(), every_lines()
    torch.cuda.synchronize()
    w = words.cpu().tolist()
    found = w[1]
    host = raw.cpu().numpy().tobytes()
    t0 = time.perf_counter()
    py = np.fromiter((x for m in re.finditer(PATTERNS[name], host) for x in m.span()), dtype=np.int64).reshape(-1, 2)
    d_ms = (time.perf_counter() - t0) * 1e3
    del host
    ok_py = w[2] == n and w[3] == count == len(py) and bool((f_spans[:count].cpu().numpy() == py).all())
    ok_lines = bool((f_owners[:count] == a_owners[:count]).all().item()) and \
        bool((f_spans[:count] == a_spans[:count] + a_owners[:count, None]).all().item())
    rows = a_rows[b_hits[:found]]                                               # the first match of every line that has one
    ok_first = w[0] == count and int(a_rows[-1].cpu()) == count and bool((a_rows[1:] > a_rows[:-1]).sum().item() == found) and \
        bool((a_spans[rows] == b_spans[:found]).all().item())
    ok_floor = int((c_len > 0).sum().cpu()) == found
    same = ok_py and ok_lines and ok_first and ok_floor

    ev = alternate({"a": every, "b": first, "c": floor}, a.reps, lambda fn: event_ms(fn, a.inner))
    wl = alternate({"a'": every_lines}, max(a.reps // 2, 3), wall_ms)
    gbs = lambda m: text_bytes / (m[0] * 1e-3) / 1e9   # noqa: E731
    fmt = lambda m: "%.4f ms (min %.4f, max %.4f) = %.1f GB/s of text" % (m + (gbs(m),))   # noqa: E731
    out = ["pair `%s`: %d matches in %d of %d lines (%.2f a line that has one)   same answer: re.finditer %s, lines %s, first match %s, floor %s" % (
               name, count, found, n, count / max(found, 1), ok_py, ok_lines, ok_first, ok_floor),
           "(a)  pire_hip_search_all, rows + owners + spans:                     %s" % fmt(ev["a"]),
           "(b)  pire_hip_search_run_select, the first match only, hits + spans: %s" % fmt(ev["b"]),
           "(c)  pire_hip_suffix with R alone (every byte read once):            %s" % fmt(ev["c"]),
           "(a) / (b) = %.2f   (a) / (c) = %.2f" % (ev["a"][0] / ev["b"][0], ev["a"][0] / ev["c"][0]),
           "(a') pire_hip_search_all_lines_gather, raw in, spans out:            %s" % fmt(wl["a'"]),
           "(d)  re.finditer on the host, one pass over the buffer, timed once:  %.0f ms   (d) / (a') = %.0f" % (d_ms, d_ms / wl["a'"][0])]
    return same, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_all_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/search_all_case.py measures on the GPU: no HIP device here")
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    raw = lines_with_addresses(n)
    size = raw.numel()
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    words = torch.zeros(1, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, words.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert int(words.cpu()[0]) == n
    text_bytes = int(offs[-1].cpu())
    out = ["# tools/search_all_case.py: %d log lines, %.1f MB of text, resident; %s in every third line" % (n, text_bytes / 1e6, ADDRESS.decode()),
           "# (a), (b), (c) device events around %d back-to-back enqueue-only calls; (a') host wall clock around one call and a synchronise;" % a.inner,
           "# median (min, max) of %d (%d) warmed repetitions, the sides alternating, one run" % (a.reps, max(a.reps // 2, 3))]
    same = True
    for name in ("ipv4", "num"):
        ok, lines = measure(name, raw, text, offs, n, text_bytes, a)
        same = same and ok
        out += lines
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
