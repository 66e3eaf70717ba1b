#!/usr/bin/env python3
"""What finding one column of every line on the device costs, and what it replaces.

The two workloads of tools/split_case.py, resident on the device -- log lines (the synthetic corpus of set_a cut into lines of
64..1023 bytes) and URLs for the dict_1k blacklist scanner, a newline behind every line --, with a TAB planted at one third
and at two thirds of every line of three bytes or more: three columns, the middle one is scanned.  Per workload, medians of
warmed repetitions:
  (a) pire_hip_fields on the split text (device pointers, field 1), in text bytes per second (device events around `--inner`
      back-to-back calls), next to a device-to-device copy of the same bytes and to pire_hip_split on the raw buffer, timed
      in the same run; the spans are held against the planted positions;
  (b) pire_hip_run_lines_field_select on the resident raw buffer with the hits and their spans fetched to the host, against
      pire_hip_run_lines_select on the same buffer (whole lines: other answers, the cost of the steps in between is the
      difference) and against the path it replaces: a host cut of the column (NumPy, vectorised), the column's text and offsets
      uploaded, pire_hip_run_select, the hits fetched.  Host wall clock around call + synchronise.

    python tools/fields_case.py [--reps 7] [--inner 10] [--out profiles/fields_case.txt] [--small] [--only-fields]
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
from split_case import event_ms, log_lines, median_ms, urls  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END
FIELD = 1


def plant_columns(raw):
    """raw with its TABs blanked and two of them planted in every line of three bytes or more; returns (raw on the device,
    the host copy, line starts, line ends, the two planted positions per line -- all in raw -- and which lines have them)."""
    host = raw.cpu().numpy().copy()
    host[host == 9] = 32
    ends = np.flatnonzero(host == 10).astype(np.int64)
    assert host[-1] == 10
    starts = np.concatenate([[0], ends[:-1] + 1])
    lens = ends - starts
    has = lens >= 3
    p1, p2 = starts + lens // 3, starts + 2 * lens // 3
    host[p1[has]] = 9
    host[p2[has]] = 9
    return torch.as_tensor(host, device="cuda"), host, starts, ends, p1, p2, has


def case(title, table, raw, a, out):
    stream = torch.cuda.current_stream().cuda_stream
    raw, host_raw, starts, ends, p1, p2, has = plant_columns(raw)
    size, n = raw.numel(), len(ends)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")

    def split():
        pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)

    def fields():
        pb.fields_device(text.data_ptr(), offs.data_ptr(), n, FIELD, spans.data_ptr(), stream=stream)

    split()
    bytes_ = size - n
    src, dst = text[:bytes_], torch.empty(bytes_, dtype=torch.uint8, device="cuda")
    fields_ms = event_ms(fields, a.reps, a.inner)
    copy_ms = event_ms(lambda: dst.copy_(src), a.reps, a.inner)
    split_ms = event_ms(split, a.reps, a.inner)
    torch.cuda.synchronize()
    # line i of the split text lies i bytes in front of where it lies in raw
    i = np.arange(n, dtype=np.int64)
    want = np.stack([np.where(has, p1 + 1, ends) - i, np.where(has, p2, ends) - i], axis=1)
    assert (spans.cpu().numpy().reshape(n, 2) == want).all(), "the spans differ from the planted columns"
    out.append(title)
    out.append("  text %.1f MB, %d lines, %.1f B a line, 2 separators a line" % (bytes_ / 1e6, n, bytes_ / n))
    out.append("  (a) pire_hip_fields %.4f ms = %.0f GB/s of text   device-to-device copy %.4f ms = %.0f GB/s   pire_hip_split (raw) %.4f ms = %.0f GB/s"
               % (fields_ms, bytes_ / fields_ms / 1e6, copy_ms, bytes_ / copy_ms / 1e6, split_ms, size / split_ms / 1e6))
    out.append("      fields / copy rate %.2f   fields / split rate %.2f" % (copy_ms / fields_ms, split_ms / fields_ms * bytes_ / size))
    if a.only_fields:
        return
    # (b) end to end
    cap = n
    hits = torch.empty(cap, dtype=torch.int64, device="cuda")
    hspans = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = {}

    def field_path():
        table.run_lines_field_select_device(raw.data_ptr(), size, FIELD, BE, counts.data_ptr(), counts.data_ptr() + 8,
                                            out_hits_ptr=hits.data_ptr(), out_hit_spans_ptr=hspans.data_ptr(), hit_cap=cap, stream=stream)
        k = int(counts.cpu()[1])
        got["field"] = (hits[:k].cpu().numpy(), hspans[:2 * k].cpu().numpy())

    def lines_path():
        table.run_lines_select_device(raw.data_ptr(), size, BE, counts.data_ptr(), counts.data_ptr() + 8, out_hits_ptr=hits.data_ptr(),
                                      out_hit_spans_ptr=hspans.data_ptr(), hit_cap=cap, stream=stream)
        k = int(counts.cpu()[1])
        got["lines"] = hits[:k].cpu().numpy()

    def host_path():
        nl = np.flatnonzero(host_raw == 10)
        tab = host_raw == 9
        st = np.concatenate([[0], nl[:-1] + 1])
        tabs_before = np.concatenate([[0], np.cumsum(tab)])          # separators in front of every byte
        rank = tabs_before[:-1] - np.repeat(tabs_before[st], nl - st + 1)   # ... since the line's start
        keep = (rank == FIELD) & ~tab & (host_raw != 10)
        htext = host_raw[keep]
        kept_before = np.concatenate([[0], np.cumsum(keep)])
        hoffs = np.concatenate([kept_before[st], [len(htext)]]).astype(np.int64)
        dt, do = torch.as_tensor(htext, device="cuda"), torch.as_tensor(hoffs, device="cuda")
        table.run_select_device(dt.data_ptr(), do.data_ptr(), len(nl), BE, counts.data_ptr() + 8, out_hits_ptr=hits.data_ptr(), hit_cap=cap,
                                stream=stream)
        k = int(counts.cpu()[1])
        got["host"] = hits[:k].cpu().numpy()

    field_ms = median_ms(field_path, a.reps)
    kernel = pb.last_kernel()
    lines_ms = median_ms(lines_path, a.reps)
    host_ms = median_ms(host_path, a.reps)
    same = len(got["field"][0]) == len(got["host"]) and bool((got["field"][0] == got["host"]).all())
    k = len(got["host"])
    whole = bool((got["field"][1].reshape(k, 2) == np.stack([starts[got["host"]], ends[got["host"]]], axis=1)).all()) if same else False
    out.append("  (b) run_lines_field_select, hits + spans fetched %.3f ms (scan kernel %s)   run_lines_select (whole lines) %.3f ms"
               % (field_ms, kernel, lines_ms))
    out.append("      host cut + upload + run_select, hits fetched %.3f ms   host / device = %.1f" % (host_ms, host_ms / field_ms))
    out.append("      hits %d of %d lines in column %d (%d on whole lines), same hit list %s, spans are the whole lines %s"
               % (k, n, FIELD, len(got["lines"]), same, whole))
    assert same and whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines per workload (a quick check of the tool)")
    ap.add_argument("--only-fields", action="store_true", help="(a) alone: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fields_case.py measures on the GPU: no HIP device here")
    out = ["# tools/fields_case.py: medians of %d warmed repetitions; (a) device events around %d back-to-back calls, (b) host wall clock"
           % (a.reps, a.inner),
           "# around call + synchronise.  The fields pass reads every byte of the text twice (count, resolve) and writes 16 bytes a string."]
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
