#!/usr/bin/env python3
"""What the leftmost-longest search costs on the device, beside what it replaces.

Input: 2^20 log lines (tools/split_case.py log_lines: the set_a corpus cut into lines of 64..1023 bytes), resident on the
device, split once; an IPv4-like address is written into every third line, 40..89 bytes from its start.  The scanners are
tests/golden/search's pair `ipv4` (F: `re`, R: `(re).*` from Fsm::Reverse()) and its SlowCapturingScanner of `.*?(re)`.
  (a) pire_hip_search_run_select: both legs in one launch, then the capture pass; positions in scratch, hits + spans.
  (b) the same answer from the entry points the project had before: pire_hip_affix_run_select TAIL with R (LongestSuffix, its
      spans), pire_hip_gather_spans of those tails into a batch of their own, pire_hip_prefix with F on that batch.  Device
      pointers throughout, nothing read back.
  (c) pire_hip_suffix with R alone: the floor of (a), whose backward leg reads every byte.
  (d) pire_hip_slow_capture_lines_gather with `.*?(re)` on the raw buffer, spans only: the only one-call route before -- beside
      (a') pire_hip_search_lines_gather on the same buffer, spans only.  Both split the buffer themselves.
(a), (b), (c): device events around `--inner` back-to-back enqueue-only calls.  (a'), (d): host wall clock around a call that
ends in a synchronise.  Median (min, max) of `--reps` warmed repetitions, the sides alternating repetition by repetition, one
run.  The answers of all sides are compared before anything is timed.

    python tools/search_case.py [--reps 7] [--inner 5] [--out profiles/search_case.txt] [--small]
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

import pire_amd  # noqa: E402
from pire_amd import binding as pb  # noqa: E402
from split_case import log_lines  # noqa: E402

SEARCH = os.path.join(ROOT, "tests", "golden", "search")
ADDRESS = b"192.168.10.254"


def blob(name):
    with open(os.path.join(SEARCH, name), "rb") as f:
        return f.read()


def lines_with_addresses(n):
    """(raw u8 on the device): log_lines without digits next to a dot, and ADDRESS in every third line"""
    _, raw = log_lines(n)
    raw[raw == ord(".")] = ord(",")                                # (no address of the corpus's own: the planted ones are the answer)
    ends = torch.nonzero(raw == 10).reshape(-1)                    # the newline of every line
    assert ends.numel() == n
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends[:-1] + 1])
    i = torch.arange(n, device="cuda")
    at = (starts + 40 + i % 50)[i % 3 == 0]                        # lines have 64 bytes or more... and 40 + 49 + 14 > 64:
    at = torch.minimum(at, (ends - len(ADDRESS) - 1)[i % 3 == 0])  # ... never across the line's end
    addr = torch.as_tensor(np.frombuffer(ADDRESS, dtype=np.uint8).copy(), device="cuda")
    raw[(at[:, None] + torch.arange(len(ADDRESS), device="cuda")[None, :]).reshape(-1)] = addr.repeat(at.numel())
    raw[at - 1] = 32
    raw[at + len(ADDRESS)] = 32
    return raw


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
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/search_case.py measures on the GPU: no HIP device here")
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
    rev, fwd = pire_amd.Table(blob("ipv4.nr.blob")), pire_amd.Table(blob("ipv4.n.blob"))
    slow = pb.SlowCaptureTable(blob("ipv4.slow.blob"))
    raw = lines_with_addresses(n)
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")

    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, **i64)
    words = torch.zeros(8, **i64)
    pb.split_device(raw.data_ptr(), size, words.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    torch.cuda.synchronize()
    assert int(words.cpu()[0]) == n
    text_bytes = int(offs[-1].cpu())

    # (a) the fused call
    a_hits, a_spans = torch.zeros(n, **i64), torch.zeros((n, 2), **i64)

    def fused():
        pb.search_run_select_device(rev, fwd, text.data_ptr(), offs.data_ptr(), n, words[1:].data_ptr(), out_hits_ptr=a_hits.data_ptr(),
                                    out_spans_ptr=a_spans.data_ptr(), hit_cap=n, stream=stream)

    # (b) the chain: the tails' spans, the tails gathered, the prefix search on them
    b_hits, b_spans = torch.zeros(n, **i64), torch.zeros((n, 2), **i64)
    b_text, b_offs = torch.empty(size + 16, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, **i64)
    b_len = torch.full((n,), -7, **i64)
    k_known = [0]

    def chain():
        pb.affix_run_select_device(None, rev, text.data_ptr(), offs.data_ptr(), n, words[2:].data_ptr(), part=pb.AFFIX_TAIL,
                                   tail_opts=pb.AFFIX_LONGEST, out_hits_ptr=b_hits.data_ptr(), out_spans_ptr=b_spans.data_ptr(), hit_cap=n,
                                   stream=stream)
        pb.gather_spans_device(text.data_ptr(), size, b_spans.data_ptr(), words[3:].data_ptr(), span_count_ptr=words[2:].data_ptr(), span_cap=n,
                               tail=None, out_text_ptr=b_text.data_ptr(), text_cap=size + 16, out_offsets_ptr=b_offs.data_ptr(), stream=stream)
        # (the host knows the number of tails from the first, checked call: the prefix scan takes n as a number)
        fwd.prefix_device(b_text.data_ptr(), b_offs.data_ptr(), k_known[0], True, b_len.data_ptr(), stream=stream)

    # (c) the backward leg alone
    c_len = torch.empty(n, **i64)

    def floor():
        rev.suffix_device(text.data_ptr(), offs.data_ptr(), n, True, c_len.data_ptr(), stream=stream)

    # (a'), (d) raw bytes in, spans out
    f_spans, d_spans = torch.zeros((n, 2), **i64), torch.zeros((n, 2), **i64)

    def fused_lines():
        pb.search_lines_gather_device(rev, fwd, raw.data_ptr(), size, words[4:].data_ptr(), words[5:].data_ptr(), out_spans_ptr=f_spans.data_ptr(),
                                      hit_cap=n, stream=stream)

    def slow_lines():
        slow.lines_gather_device(raw.data_ptr(), size, words[6:].data_ptr(), words[7:].data_ptr(), out_spans_ptr=d_spans.data_ptr(), hit_cap=n,
                                 stream=stream)

    # the answers, compared before anything is timed
    fused()
    torch.cuda.synchronize()
    found = int(words.cpu()[1])
    chain()
    torch.cuda.synchronize()
    k_known[0] = int(words.cpu()[2])
    chain()
    floor()
    fused_lines()
    slow_lines()
    torch.cuda.synchronize()
    w = words.cpu().tolist()
    k = k_known[0]
    starts = b_spans[:k, 0]                                                      # where the tail of hit j begins: the match's begin
    ok_chain = k == found and bool((b_hits[:k] == a_hits[:k]).all().item()) and bool((starts == a_spans[:k, 0]).all().item()) \
        and bool((b_len[:k] >= 0).all().item()) and bool((starts + b_len[:k] == a_spans[:k, 1]).all().item())
    ok_floor = int((c_len >= 0).sum().cpu()) == found
    shift = a_hits[:found]                                                       # line i lies i bytes further into raw
    ok_lines = w[4] == n and w[5] == found and bool((f_spans[:found] == a_spans[:found] + shift[:, None]).all().item())
    ok_slow = w[6] == n and w[7] == found and bool((d_spans[:found] == f_spans[:found]).all().item())
    expected = (n + 2) // 3
    same = ok_chain and ok_floor and ok_lines and ok_slow and found == expected

    ev = alternate({"a": fused, "b": chain, "c": floor}, a.reps, lambda fn: event_ms(fn, a.inner))
    wl = alternate({"a'": fused_lines, "d": slow_lines}, max(a.reps // 2, 3), wall_ms)

    gbs = lambda m: text_bytes / (m[0] * 1e-3) / 1e9   # noqa: E731
    fmt = lambda m: "%.4f ms (min %.4f, max %.4f) = %.1f GB/s of text" % (m + (gbs(m),))   # noqa: E731
    out = ["# tools/search_case.py: %d log lines, %.1f MB of text, resident; pair `ipv4`, %s in every third line" % (n, text_bytes / 1e6, ADDRESS.decode()),
           "# (a), (b), (c) device events around %d back-to-back enqueue-only calls; (a'), (d) host wall clock around one call and a" % a.inner,
           "# synchronise; median (min, max) of %d (%d) warmed repetitions, the sides alternating, one run" % (a.reps, max(a.reps // 2, 3)),
           "found %d of %d lines (%.1f %%)   same answer: chain %s, floor %s, lines %s, slow capture %s" % (
               found, n, 100.0 * found / n, ok_chain, ok_floor, ok_lines, ok_slow),
           "(a)  pire_hip_search_run_select, positions in scratch, hits + spans:               %s" % fmt(ev["a"]),
           "(b)  affix_run_select TAIL with R -> gather_spans -> prefix with F (device pointers): %s" % fmt(ev["b"]),
           "(c)  pire_hip_suffix with R alone (the backward leg: every byte read once):        %s" % fmt(ev["c"]),
           "(a) / (b) = %.2f   (a) / (c) = %.2f" % (ev["a"][0] / ev["b"][0], ev["a"][0] / ev["c"][0]),
           "(a') pire_hip_search_lines_gather, raw in, spans out:                              %s" % fmt(wl["a'"]),
           "(d)  pire_hip_slow_capture_lines_gather with .*?(re), raw in, spans out:           %s" % fmt(wl["d"]),
           "(d) / (a') = %.1f" % (wl["d"][0] / wl["a'"][0])]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
