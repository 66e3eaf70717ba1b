#!/usr/bin/env python3
"""What cutting raw text into lines on the device costs, and what it replaces.

Two workloads, resident on the device: log lines (the synthetic corpus of set_a cut into lines of 64..1023 bytes) and URLs
for the dict_1k blacklist scanner, a newline behind every line.  Per workload, medians of warmed repetitions:
  (a) pire_hip_split, device pointers, in raw bytes per second (device events around `--inner` back-to-back calls), next
      to a device-to-device copy of the same byte count (torch's copy_ of a contiguous tensor: hipMemcpyAsync) timed in the
      same run -- the floor of any pass that reads and writes every byte once; the split reads every byte twice;
  (b) pire_hip_run_lines_select on the resident raw buffer with the hits and their spans fetched to the host, against the
      path it replaces for the same bytes: a host split (NumPy: flatnonzero + a masked copy -- the work of the sample's old
      ReadLines, vectorised), text and offsets uploaded, pire_hip_run_select, the hits fetched.  Host wall clock around
      call + synchronise; the raw buffer is on the host already for the old path and on the device already for the new one.

    python tools/split_case.py [--reps 7] [--inner 10] [--out profiles/split_case.txt] [--small] [--only-split]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pire_amd  # noqa: E402
from pire_amd import binding as pb  # noqa: E402
from pire_amd import workloads as W  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def log_lines(n, seed=1234):
    """(table, raw u8 on the device): n lines of 64..1023 bytes over the set_a corpus."""
    big = W.pattern_set("set_a")
    lens = np.random.RandomState(seed).randint(64, 1024, size=n)
    total = int(lens.sum()) + n
    rec = 1024
    buf = torch.empty(((total + rec - 1) // rec, rec), dtype=torch.uint8, device="cuda")
    pire_amd.corpus_fill_device(buf.data_ptr(), seed, 0, buf.shape[0], rec, rec, W.plants_for(big),
                                torch.cuda.current_stream().cuda_stream)
    raw = buf.reshape(-1)[:total]
    raw[raw == 10] = 32
    raw[torch.as_tensor(np.cumsum(lens + 1) - 1, device="cuda")] = 10
    return pire_amd.Table(W.load_blob(big["blob"])), raw.contiguous()


def urls(n, seed=0x5EED5EED):
    entry = W.wide_set("dict_1k")
    text, offs = W.wide_urls(entry, seed, n)
    lens = np.diff(offs.astype(np.int64))
    raw = np.full(len(text) + n, 10, dtype=np.uint8)
    keep = np.ones(len(raw), dtype=bool)
    keep[np.cumsum(lens + 1) - 1] = False
    raw[keep] = text
    return pire_amd.Table(W.load_blob(entry["blob"])), torch.as_tensor(raw, device="cuda")


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def event_ms(fn, reps, inner, warm=3):
    """Median over reps of (device time of `inner` back-to-back calls) / inner."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return float(np.median(out))


def case(title, table, raw, a, out):
    size = raw.numel()
    stream = torch.cuda.current_stream().cuda_stream
    host_raw = raw.cpu().numpy()
    n = int((host_raw == 10).sum()) + (1 if host_raw[-1] != 10 else 0)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(raw)

    def split():
        pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)

    def split_keep():
        pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, 0, offs.data_ptr(), n, stream)

    split_ms = event_ms(split, a.reps, a.inner)
    copy_ms = event_ms(lambda: dst.copy_(raw), a.reps, a.inner)
    keep_ms = event_ms(split_keep, a.reps, a.inner)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == n
    d = n - (1 if host_raw[-1] != 10 else 0)
    assert (text[:size - d].cpu().numpy() == host_raw[host_raw != 10]).all(), "split text differs from the host's"
    out.append(title)
    out.append("  raw %.1f MB, %d lines, %.1f B a line" % (size / 1e6, n, size / n))
    out.append("  (a) pire_hip_split %.4f ms = %.0f GB/s of raw   device-to-device copy %.4f ms = %.0f GB/s   split / copy rate %.2f"
               % (split_ms, size / split_ms / 1e6, copy_ms, size / copy_ms / 1e6, copy_ms / split_ms))
    out.append("      offsets only (out_text == NULL) %.4f ms = %.0f GB/s" % (keep_ms, size / keep_ms / 1e6))
    if a.only_split:
        return
    # (b) end to end
    cap = n
    hits = torch.empty(cap, dtype=torch.int64, device="cuda")
    spans = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = {}

    def new_path():
        table.run_lines_select_device(raw.data_ptr(), size, BE, counts.data_ptr(), counts.data_ptr() + 8, out_hits_ptr=hits.data_ptr(),
                                      out_hit_spans_ptr=spans.data_ptr(), hit_cap=cap, stream=stream)
        k = int(counts.cpu()[1])
        got["new"] = (hits[:k].cpu().numpy(), spans[:2 * k].cpu().numpy())

    def old_path():
        p = np.flatnonzero(host_raw == 10)
        htext = host_raw[host_raw != 10]
        lines = len(p) + (1 if host_raw[-1] != 10 else 0)
        hoffs = np.zeros(lines + 1, dtype=np.int64)
        hoffs[1:len(p) + 1] = p - np.arange(len(p))
        hoffs[lines] = len(htext)
        dt, do = torch.as_tensor(htext, device="cuda"), torch.as_tensor(hoffs, device="cuda")
        table.run_select_device(dt.data_ptr(), do.data_ptr(), lines, BE, counts.data_ptr() + 8, out_hits_ptr=hits.data_ptr(), hit_cap=cap,
                                stream=stream)
        k = int(counts.cpu()[1])
        got["old"] = hits[:k].cpu().numpy()

    new_ms = median_ms(new_path, a.reps)
    kernel = pb.last_kernel()
    old_ms = median_ms(old_path, a.reps)
    same = len(got["new"][0]) == len(got["old"]) and bool((got["new"][0] == got["old"]).all())
    out.append("  (b) run_lines_select, hits + spans fetched %.3f ms (scan kernel %s)   host split + upload + run_select, hits fetched %.3f ms"
               % (new_ms, kernel, old_ms))
    out.append("      hits %d of %d lines, same hit list %s, old / new = %.1f" % (len(got["old"]), n, same, old_ms / new_ms))
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines per workload (a quick check of the tool)")
    ap.add_argument("--only-split", action="store_true", help="(a) alone: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/split_case.py measures on the GPU: no HIP device here")
    out = ["# tools/split_case.py: medians of %d warmed repetitions; (a) device events around %d back-to-back calls, (b) host wall clock"
           % (a.reps, a.inner),
           "# around call + synchronise.  The split reads every byte of raw twice (count, scatter) and writes it once."]
    for title, make, n in (("log lines 64..1023 B (set_a)", log_lines, 1 << 20), ("URLs (dict_1k)", urls, 1 << 19)):
        table, raw = make(1 << 14 if a.small else n)
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
