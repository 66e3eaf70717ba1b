#!/usr/bin/env python3
"""What turning capture positions into byte ranges on the device costs, and what it replaces.

2^20 log lines resident on the device -- the corpus of tools/gather_case.py (the synthetic corpus of set_a cut into lines of
64..1023 bytes) with a witness of the capture_kv fixture (`user_id: "alice"` and its kin) written into about a quarter of
the lines --, scanned by the capture_kv scanner.  Medians (and the spread, min..max) of warmed repetitions:
  (a) pire_hip_capture_select alone, device pointers, on the positions pire_hip_capture_run left on the device: device
      events around `--inner` back-to-back calls, in bytes read + written per second (17 B in per string, 24 B out per
      selected string); next to it pire_hip_select on the same n (the end states of the set_a scanner on the same lines,
      hits only) and a device-to-device copy of the same number of bytes, timed in the same run;
  (b) pire_hip_capture_run alone against pire_hip_capture_run_select on the split lines (what the pass adds to a scan);
  (c) pire_hip_capture_lines_gather on the resident raw buffer, the captured fields and their offsets left on the device,
      against the route it replaces: the split and pire_hip_capture_run on the device, out_begin / out_end fetched, the
      spans computed and compacted on the host (numpy), uploaded, pire_hip_gather_spans.  Host wall clock around call +
      synchronise.

    python tools/capture_select_case.py [--reps 7] [--inner 10] [--out profiles/capture_select_case.txt] [--small]
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
from pire_amd import workloads as W  # noqa: E402
from split_case import log_lines  # noqa: E402

BE = pb.FLAG_BEGIN | pb.FLAG_END


def spread_ms(fn, reps, inner, warm=3):
    """(median, min, max) over reps of (device time of `inner` back-to-back calls) / inner"""
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
    return float(np.median(out)), float(min(out)), float(max(out))


def wall_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def fmt(t):
    return "%.4f ms (%.4f..%.4f)" % t


def capture_fixture(name="capture_kv"):
    import json

    with open(os.path.join(W.GOLDEN, "cases.json")) as f:
        return [c for c in json.load(f)["capturing"] if c["name"] == name][0]


def planted_lines(n, rate=0.25, seed=1234):
    """(set_a table, raw u8 on the device): log_lines with a capture_kv witness inside about `rate` of the lines"""
    table, raw = log_lines(n, seed)
    host = raw.cpu().numpy()
    wit = [np.frombuffer(bytes.fromhex(h), dtype=np.uint8) for h in capture_fixture()["witnesses_hex"]]
    wit = [w for w in wit if len(w) <= 48 and 10 not in w]
    nl = np.flatnonzero(host == 10)
    starts = np.concatenate([[0], nl[:-1] + 1])
    rng = np.random.RandomState(seed + 1)
    for i in np.flatnonzero(rng.rand(len(starts)) < rate).tolist():
        w = wit[i % len(wit)]
        room = int(nl[i] - starts[i]) - len(w)                 # lines have 64 bytes or more
        at = int(starts[i]) + int(rng.randint(0, room + 1))
        host[at:at + len(w)] = w
    return table, torch.as_tensor(host, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capture_select_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^14 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/capture_select_case.py measures on the GPU: no HIP device here")
    stream = torch.cuda.current_stream().cuda_stream
    plain, raw = planted_lines(1 << 14 if a.small else 1 << 20)
    plain.upload()
    cap = pb.CountingTable(W.load_blob(capture_fixture()["blob"]), 0)
    size = raw.numel()
    host_raw = raw.cpu().numpy()
    n = int((host_raw == 10).sum()) + (1 if host_raw[-1] != 10 else 0)
    text = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    fin = torch.empty(n, dtype=torch.uint8, device="cuda")
    begin, end = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    hits = torch.empty(n, dtype=torch.int64, device="cuda")
    spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")

    def capture_run():
        cap.capture_device(text.data_ptr(), offs.data_ptr(), n, BE, idx.data_ptr(), fin.data_ptr(), begin.data_ptr(), end.data_ptr(), stream)

    capture_run()
    torch.cuda.synchronize()
    kernel = pb.last_kernel()
    b, e = begin.cpu().numpy(), end.cpu().numpy()
    captured = (b >= 0) & (e >= 0)
    k = int(captured.sum())
    out = ["# tools/capture_select_case.py: median (min..max) of %d warmed repetitions; (a), (b) device events around %d back-to-back"
           % (a.reps, a.inner),
           "# calls, (c) host wall clock around call + synchronise",
           "2^20 log lines 64..1023 B (set_a corpus), capture_kv witnesses planted" if not a.small else "2^14 log lines (--small)",
           "  raw %.1f MB, %d lines, %d captured (%.1f %%), capture kernel %s" % (size / 1e6, n, k, 100.0 * k / n, kernel)]

    # (a) the pass alone, pire_hip_select on the same n, a copy of the same bytes
    def the_pass():
        pb.capture_select_device(offs.data_ptr(), n, BE, begin.data_ptr(), end.data_ptr(), cnt.data_ptr() + 8, final_ptr=fin.data_ptr(),
                                 need_final=True, out_hits_ptr=hits.data_ptr(), out_spans_ptr=spans.data_ptr(), hit_cap=n, stream=stream)

    the_pass()
    torch.cuda.synchronize()
    got = int(cnt.cpu()[1])
    host_fin = fin.cpu().numpy()
    want = np.flatnonzero(captured & (host_fin != 0))
    assert got == len(want) and (hits[:got].cpu().numpy() == want).all(), "the pass's list differs from the host's"
    host_offs = offs.cpu().numpy()
    sp = spans[:2 * got].cpu().numpy().reshape(-1, 2)
    lens = host_offs[want + 1] - host_offs[want]
    cb = np.clip(b[want] - 1, 0, lens)
    assert (sp[:, 0] == host_offs[want] + cb).all() and (sp[:, 1] == host_offs[want] + np.clip(e[want] - 1, cb, lens)).all()
    moved = 17 * n + 8 * 2 * got + 24 * got        # begin, end, final; offsets[i], offsets[i + 1] of the selected; hits + spans
    pass_t = spread_ms(the_pass, a.reps, a.inner)
    sidx = torch.empty(n, dtype=torch.int32, device="cuda")
    plain.run_device(text.data_ptr(), offs.data_ptr(), n, BE, out_idx_ptr=sidx.data_ptr(), stream=stream)
    torch.cuda.synchronize()

    def select():
        plain.select_device(sidx.data_ptr(), n, cnt.data_ptr() + 16, out_hits_ptr=hits.data_ptr(), hit_cap=n, stream=stream)

    select_t = spread_ms(select, a.reps, a.inner)
    select_hits = int(cnt.cpu()[2])
    src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
    copy_t = spread_ms(lambda: dst.copy_(src), a.reps, a.inner)
    out.append("  (a) pire_hip_capture_select (need_final, hits + spans), %d selected, %.1f MB read + written: %s = %.0f GB/s"
               % (got, moved / 1e6, fmt(pass_t), moved / pass_t[0] / 1e6))
    out.append("      pire_hip_select, same n, %d hits (hits only): %s   pass / select %.2f" % (select_hits, fmt(select_t), pass_t[0] / select_t[0]))
    out.append("      device-to-device copy of %.1f MB: %s = %.0f GB/s   pass / copy %.2f"
               % (moved / 1e6, fmt(copy_t), moved / copy_t[0] / 1e6, pass_t[0] / copy_t[0]))

    # (b) what the pass adds to a scan
    def run_select():
        cap.capture_select_device(text.data_ptr(), offs.data_ptr(), n, BE, cnt.data_ptr() + 8, out_hits_ptr=hits.data_ptr(),
                                  out_spans_ptr=spans.data_ptr(), hit_cap=n, stream=stream)

    run_t = spread_ms(capture_run, a.reps, a.inner)
    both_t = spread_ms(run_select, a.reps, a.inner)
    text_bytes = int(host_offs[n])
    out.append("  (b) pire_hip_capture_run %s = %.0f GB/s of text   pire_hip_capture_run_select (positions in scratch) %s   + %.1f %%"
               % (fmt(run_t), text_bytes / run_t[0] / 1e6, fmt(both_t), 100.0 * (both_t[0] / run_t[0] - 1)))

    # (c) raw bytes in, captured fields out: one call against the host detour
    g_text = torch.empty(size + n + 16, dtype=torch.uint8, device="cuda")
    g_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")

    def fused():
        cap.capture_lines_gather_device(raw.data_ptr(), size, BE, cnt.data_ptr(), cnt.data_ptr() + 8, out_bytes_ptr=cnt.data_ptr() + 24,
                                        tail=-1, out_spans_ptr=spans.data_ptr(), hit_cap=n, out_text_ptr=g_text.data_ptr(),
                                        text_cap=size + n, out_offsets_ptr=g_offs.data_ptr(), stream=stream)

    fused()
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert int(c[0]) == n and int(c[1]) == k
    fused_bytes = int(c[3])
    fused_text = g_text[:fused_bytes].cpu().numpy().copy()
    up_spans = torch.empty(2 * n, dtype=torch.int64, device="cuda")

    def detour():
        pb.split_device(raw.data_ptr(), size, cnt.data_ptr(), 10, text.data_ptr(), offs.data_ptr(), n, stream)
        capture_run()
        hb, he, ho = begin.cpu().numpy(), end.cpu().numpy(), offs.cpu().numpy()      # (synchronises)
        sel = np.flatnonzero((hb >= 0) & (he >= 0))
        base = ho[sel] + sel                                                         # line i lies i bytes further into raw
        hs = np.stack([base + hb[sel] - 1, base + he[sel] - 1], axis=1)
        up_spans[:2 * len(sel)].copy_(torch.as_tensor(hs.reshape(-1)), non_blocking=False)
        pb.gather_spans_device(raw.data_ptr(), size, up_spans.data_ptr(), cnt.data_ptr() + 24, span_cap=len(sel), tail=10,
                               out_text_ptr=g_text.data_ptr(), text_cap=size + n, out_offsets_ptr=g_offs.data_ptr(), stream=stream)

    detour()
    torch.cuda.synchronize()
    assert int(cnt.cpu()[3]) == fused_bytes and (g_text[:fused_bytes].cpu().numpy() == fused_text).all(), "the two routes differ"
    fused_t = wall_ms(fused, a.reps)
    detour_t = wall_ms(detour, a.reps)
    out.append("  (c) pire_hip_capture_lines_gather, %d fields, %.1f MB gathered, left on the device: %s" % (k, fused_bytes / 1e6, fmt(fused_t)))
    out.append("      split + capture_run on the device, positions fetched, spans on the host (numpy), upload, gather_spans: %s   old / new %.1f"
               % (fmt(detour_t), detour_t[0] / fused_t[0]))
    result = "\n".join(out) + "\n"
    print(result, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(result)
    return 0


if __name__ == "__main__":
    sys.exit(main())
