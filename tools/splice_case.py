#!/usr/bin/env python3
"""What replacing every match of a resident buffer costs on the device.

Input: tools/search_all_case.py's -- 2^20 log lines of 64..1023 bytes, resident on the device, an IPv4-like address in every
third line.  Two pairs of tests/golden/search: `ipv4` (a match in every third line) and `num` (several in every line).  Three
pieces: a 1-byte replacement (`#`), deletion, and a Wrap of 5 + 4 bytes around the match (`grep --color`'s escapes).
  (a)  pire_hip_splice alone on device pointers, over the span list of pire_hip_search_all_lines_gather, out_pos in scratch.
  (a+) the same with out_pos in an array of the caller's: the call allocates nothing.
  (m)  hipMemcpyAsync, device to device, of as many bytes as (a) writes: the ceiling of a pass that reads and writes every byte.
  (g)  pire_hip_gather_spans over the same span list, no tail byte: the sibling pass (it moves the matches, not the rest).
  (b)  pire_hip_search_lines_splice on the raw buffer, end to end: split, search, splice; host wall clock, one synchronise.
  (s)  pire_hip_search_all_lines_gather on the same input (spans and `grep -o`'s bytes): the nearest call before this one.
  (h)  the host route that (b) replaces: the spans fetched, bytes.join in Python, the result uploaded.  Timed once; for `num`
       (50 matches a line) on the first --host-lines lines only, scaled by bytes, and labelled so.
(a), (a+), (m), (g): device events around `--inner` back-to-back enqueue-only calls; (b), (s): host wall clock around one call and a
synchronise; median (min, max) of `--reps` warmed repetitions, the sides alternating repetition by repetition, one run.  All
sides are compared before anything is timed: (a) and (b) byte for byte with each other and with re.sub on the host (for `num`
re.sub runs on the lines of (h) only), (g)'s byte count with the matches' own, (h) with (a).

    python tools/splice_case.py [--reps 7] [--inner 3] [--out profiles/splice_case.txt] [--small] [--host-lines 65536]
"""
import argparse
import ctypes as C
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
HEAD, TAIL = b"\x1b[31m", b"\x1b[0m"
PIECES = (("1-byte replacement", b"#", b"", 0, b"#"), ("deletion", b"", b"", 0, b""),
          ("wrap 5 + 4 bytes", HEAD, TAIL, pb.SPLICE_KEEP, HEAD.replace(b"\\", b"\\\\") + rb"\g<0>" + TAIL))
D2D = 3   # hipMemcpyDeviceToDevice


def host_route(host, spans, head, tail, keep):
    """the spans are on the host already: the join, and the upload of its result"""
    t0 = time.perf_counter()
    parts, at = [], 0
    for b, e in spans.tolist():
        parts.append(host[at:b])
        parts.append(head + host[b:e] + tail if keep else head)
        at = e
    parts.append(host[at:])
    joined = b"".join(parts)
    up = torch.as_tensor(np.frombuffer(joined, dtype=np.uint8), device="cuda")
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, joined, up


def measure(name, raw, n, a, hip):
    stream = torch.cuda.current_stream().cuda_stream
    size = raw.numel()
    i64 = dict(dtype=torch.int64, device="cuda")
    rev, fwd = pire_amd.Table(blob(name + ".nr.blob")), pire_amd.Table(blob(name + ".n.blob"))
    words = torch.zeros(8, **i64)
    pb.search_all_lines_gather_device(rev, fwd, raw.data_ptr(), size, words.data_ptr(), words[1:].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    count = int(words.cpu()[1])
    cap = count + 1
    spans = torch.zeros((cap, 2), **i64)
    pb.search_all_lines_gather_device(rev, fwd, raw.data_ptr(), size, words.data_ptr(), words[1:].data_ptr(), out_spans_ptr=spans.data_ptr(),
                                      match_cap=cap, stream=stream)
    torch.cuda.synchronize()
    matched = int((spans[:count, 1] - spans[:count, 0]).sum().cpu())
    room = size + cap * (len(HEAD) + len(TAIL))
    out_a = torch.empty(room, dtype=torch.uint8, device="cuda")
    out_b = torch.empty(room, dtype=torch.uint8, device="cuda")
    out_m = torch.empty(room, dtype=torch.uint8, device="cuda")
    pos = torch.zeros(cap, **i64)
    g_text, g_offs = torch.empty(matched + cap + 16, dtype=torch.uint8, device="cuda"), torch.zeros(cap + 1, **i64)
    host = raw.cpu().numpy().tobytes()
    t0 = time.perf_counter()
    h_spans = spans[:count].cpu().numpy()                                       # (h)'s first step: the spans fetched
    fetch_ms = (time.perf_counter() - t0) * 1e3
    lines_host = n if name == "ipv4" else min(a.host_lines, n)
    cut = size if lines_host == n else int(torch.nonzero(raw == 10).reshape(-1)[lines_host - 1].cpu()) + 1

    def gather():
        rc = pb.lib().pire_hip_gather_spans(raw.data_ptr(), size, spans.data_ptr(), words[1:].data_ptr(), cap, pb.NO_TAIL, pb.FLAG_ON_DEVICE,
                                            g_text.data_ptr(), g_text.numel(), g_offs.data_ptr(), words[4:].data_ptr(), stream)
        assert rc == 0, pb.lib().pire_hip_last_error()

    def nearest():
        pb.search_all_lines_gather_device(rev, fwd, raw.data_ptr(), size, words.data_ptr(), words[1:].data_ptr(), out_bytes_ptr=words[5:].data_ptr(),
                                          tail_byte=None, out_spans_ptr=spans.data_ptr(), match_cap=cap, out_text_ptr=g_text.data_ptr(),
                                          text_cap=g_text.numel(), out_offsets_ptr=g_offs.data_ptr(), stream=stream)

    gather()
    torch.cuda.synchronize()
    same = int(words.cpu()[4]) == matched
    out = ["pair `%s`: %d matches of %d bytes in %d lines, %.1f MB of raw text" % (name, count, matched, n, size / 1e6)]
    for what, head, tail, mode, repl in PIECES:
        def alone():
            pb.splice_device(raw.data_ptr(), size, spans.data_ptr(), cap, words[2:].data_ptr(), head=head, tail=tail, mode=mode,
                             span_count_ptr=words[1:].data_ptr(), out_text_ptr=out_a.data_ptr(), text_cap=room, stream=stream)

        def alone_pos():
            pb.splice_device(raw.data_ptr(), size, spans.data_ptr(), cap, words[2:].data_ptr(), head=head, tail=tail, mode=mode,
                             span_count_ptr=words[1:].data_ptr(), out_text_ptr=out_a.data_ptr(), text_cap=room, out_pos_ptr=pos.data_ptr(),
                             stream=stream)

        def fused():
            pb.search_lines_splice_device(rev, fwd, raw.data_ptr(), size, words.data_ptr(), words[6:].data_ptr(), words[3:].data_ptr(), head=head,
                                          tail=tail, mode=mode, match_cap=cap, out_text_ptr=out_b.data_ptr(), text_cap=room, stream=stream)

        alone(), fused()
        torch.cuda.synchronize()
        w = words.cpu().tolist()
        nbytes = w[2]
        want = re.sub(PATTERNS[name], repl, host[:cut])                         # (whole lines: no match straddles the cut)
        ok = nbytes == w[3] and (len(want) == nbytes or cut < size) and w[6] == count and w[0] == n
        ok = ok and bool((out_a[:nbytes] == out_b[:nbytes]).all().item()) and out_a[:len(want)].cpu().numpy().tobytes() == want
        h_ms, joined, up = host_route(host[:cut], h_spans[h_spans[:, 1] <= cut], head, tail, bool(mode))
        ok = ok and joined == want[:len(joined)] and bool((up == out_a[:len(joined)]).all().item())
        del want, joined, up
        same = same and ok

        def memcpy():
            assert hip.hipMemcpyAsync(C.c_void_p(out_m.data_ptr()), C.c_void_p(out_a.data_ptr()), C.c_size_t(nbytes), D2D, C.c_void_p(stream)) == 0

        ev = alternate({"a": alone, "a+": alone_pos, "m": memcpy, "g": gather}, a.reps, lambda fn: event_ms(fn, a.inner))
        wl = alternate({"b": fused, "s": nearest}, max(a.reps // 2, 3), wall_ms)
        moved = size + nbytes                                                   # bytes read + bytes written, the lists aside
        fmt = lambda m, by: "%.4f ms (min %.4f, max %.4f) = %.1f GB/s" % (m + (by / (m[0] * 1e-3) / 1e9,))   # noqa: E731
        scale = size / cut
        out += ["  %s: %d bytes out   same answer: %s" % (what, nbytes, ok),
                "  (a)  pire_hip_splice alone, out_pos in scratch:               %s read + written" % fmt(ev["a"], moved),
                "  (a+) ... out_pos in the caller's array:                        %s read + written" % fmt(ev["a+"], moved),
                "  (m)  hipMemcpyAsync device to device of the output's bytes:   %s read + written" % fmt(ev["m"], 2 * nbytes),
                "  (g)  pire_hip_gather_spans over the same spans, no tail:      %s read + written" % fmt(ev["g"], 2 * matched),
                "  (a) / (m) = %.2f   (a) / (g) = %.2f   rate of (a) / rate of (g) = %.2f" % (
                    ev["a"][0] / ev["m"][0], ev["a"][0] / ev["g"][0], (moved / ev["a"][0]) / (2 * matched / ev["g"][0])),
                "  (b)  pire_hip_search_lines_splice, raw in, rewritten text out: %s of raw text" % fmt(wl["b"], size),
                "  (s)  pire_hip_search_all_lines_gather, spans + matched bytes:  %s of raw text" % fmt(wl["s"], size),
                "  (h)  host route%s: spans fetched %.1f ms + join and upload %.0f ms%s   (b) / (s) = %.2f   (h) / (b) = %.0f" % (
                    "" if lines_host == n else ", first %d lines" % lines_host, fetch_ms, h_ms,
                    "" if lines_host == n else " (x %.1f by bytes = %.0f ms)" % (scale, h_ms * scale), wl["b"][0] / wl["s"][0],
                    (fetch_ms + h_ms * scale) / wl["b"][0])]
    return same, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    ap.add_argument("--host-lines", type=int, default=1 << 16, help="the lines the host route of `num` is timed on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/splice_case.py measures on the GPU: no HIP device here")
    hip = C.CDLL("libamdhip64.so")
    n = 1 << 16 if a.small else 1 << 20
    raw = lines_with_addresses(n)
    out = ["# tools/splice_case.py: %d log lines, %.1f MB, resident; %s in every third line" % (n, raw.numel() / 1e6, ADDRESS.decode()),
           "# (a), (a+), (m), (g) device events around %d back-to-back enqueue-only calls; (b), (s) host wall clock around one call and a synchronise;" % a.inner,
           "# median (min, max) of %d (%d) warmed repetitions, the sides alternating, one run; (h) timed once" % (a.reps, max(a.reps // 2, 3))]
    same = True
    for name in ("ipv4", "num"):
        ok, lines = measure(name, raw, n, a, hip)
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
