#!/usr/bin/env python3
"""What the labels of pire_hip_lex cost beside pire_hip_search_all, and tokens beside matches.

Input: tools/search_all_case.py's -- 2^20 log lines of 64..1023 bytes, resident on the device, split once.  The set is
`lexer3` of tests/golden/lex: `[a-z]+`, `[0-9]+`, `[ \\t]+` glued (5 states) and the reversed union (3 states).
  (a)  pire_hip_lex, search mode: rows, owners, spans, masks and label counts.
  (a-) the same without label counts: what the tallies cost.
  (b)  pire_hip_search_all on the same two tables and text: rows, owners, spans.  (a) / (b) is the cost of the labels.
  (c)  pire_hip_lex, token mode, all five outputs: no marks, and the gaps as entries of their own.
  (d)  the host route to (a): (b)'s spans fetched, every span labelled by its first byte (for this set that decides the regexp)
       and counted with numpy.  Host wall clock, it includes the copy of the spans.
(a), (a-), (b), (c): device events around `--inner` back-to-back enqueue-only calls; median (min, max) of `--reps` warmed
repetitions, the sides alternating repetition by repetition, one run.  (d): host wall clock, median of 3.  Before anything is
timed: (a)'s spans, owners and rows are (b)'s bit for bit, its masks are (d)'s labels, its label counts their histogram, and
(c) without its gaps is (a).

    python tools/lex_case.py [--reps 7] [--inner 3] [--out profiles/lex_case.txt] [--small]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pire_amd  # noqa: E402
from pire_amd import binding as pb  # noqa: E402
from search_case import alternate, event_ms, lines_with_addresses, wall_ms  # noqa: E402
from tests import helpers as H  # noqa: E402

SET = "lexer3"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lex_case.txt"))
    ap.add_argument("--small", action="store_true", help="2^16 lines (a quick check of the tool)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lex_case.py measures on the GPU: no HIP device here")
    n = 1 << 16 if a.small else 1 << 20
    stream = torch.cuda.current_stream().cuda_stream
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
    rev = pire_amd.Table(H.load_blob(os.path.join("lex", SET + ".nr.blob")))
    fwd = pire_amd.Table(H.load_blob(os.path.join("lex", SET + ".n.blob")))
    R = fwd.info.regexps
    tp, op = text.data_ptr(), offs.data_ptr()
    # how many there are: the calls with no room say so
    pb.lex_device(rev, fwd, tp, text_bytes, op, n, words.data_ptr(), stream=stream)
    pb.lex_device(None, fwd, tp, text_bytes, op, n, words[1:].data_ptr(), opts=pb.LEX_TOKENS, stream=stream)
    torch.cuda.synchronize()
    matches, entries = (int(x) for x in words.cpu()[:2])
    cap, tcap = matches + 1, entries + 1

    def lists(k):
        return torch.zeros(n + 1, **i64), torch.zeros(k, **i64), torch.zeros((k, 2), **i64), torch.zeros(k, **i64), torch.zeros(R + 1, **i64)

    a_rows, a_owners, a_spans, a_masks, a_labels = lists(cap)
    b_rows, b_owners, b_spans, _, _ = lists(cap)
    c_rows, c_owners, c_spans, c_masks, c_labels = lists(tcap)

    def labelled(labels=True):
        pb.lex_device(rev, fwd, tp, text_bytes, op, n, words[2:].data_ptr(), out_rows_ptr=a_rows.data_ptr(), out_owners_ptr=a_owners.data_ptr(),
                      out_spans_ptr=a_spans.data_ptr(), out_masks_ptr=a_masks.data_ptr(), match_cap=cap,
                      out_label_counts_ptr=a_labels.data_ptr() if labels else 0, stream=stream)

    def plain():
        pb.search_all_device(rev, fwd, tp, text_bytes, op, n, words[3:].data_ptr(), out_rows_ptr=b_rows.data_ptr(),
                             out_owners_ptr=b_owners.data_ptr(), out_spans_ptr=b_spans.data_ptr(), match_cap=cap, stream=stream)

    def tokens():
        pb.lex_device(None, fwd, tp, text_bytes, op, n, words[4:].data_ptr(), opts=pb.LEX_TOKENS, out_rows_ptr=c_rows.data_ptr(),
                      out_owners_ptr=c_owners.data_ptr(), out_spans_ptr=c_spans.data_ptr(), out_masks_ptr=c_masks.data_ptr(), match_cap=tcap,
                      out_label_counts_ptr=c_labels.data_ptr(), stream=stream)

    klass = np.full(256, R, dtype=np.int64)                       # the regexp a span of this set belongs to, by its first byte
    klass[np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)] = 0
    klass[np.frombuffer(b"0123456789", np.uint8)] = 1
    klass[np.frombuffer(b" \t", np.uint8)] = 2
    host_text = text.cpu().numpy()
    host = {}

    def on_host():
        spans = b_spans[:matches].cpu().numpy()
        host["labels"] = klass[host_text[spans[:, 0]]]
        host["counts"] = np.bincount(host["labels"], minlength=R + 1)

    labelled(), plain(), tokens()
    torch.cuda.synchronize()
    on_host()
    w = words.cpu().tolist()
    ok_spans = w[2] == w[3] == matches and bool((a_rows == b_rows).all().item()) and bool((a_owners == b_owners).all().item()) and \
        bool((a_spans == b_spans).all().item())
    masks = a_masks[:matches].cpu().numpy()
    ok_masks = bool((masks == (1 << host["labels"])).all()) and bool((a_labels.cpu().numpy() == host["counts"]).all())
    keep = c_masks[:entries] != 0
    ok_tokens = w[4] == entries and int(keep.sum().cpu()) == matches and bool((c_spans[:entries][keep] == a_spans[:matches]).all().item()) and \
        bool((c_masks[:entries][keep] == a_masks[:matches]).all().item()) and \
        int(c_labels[R].cpu()) == entries - matches and bool((c_labels[:R] == a_labels[:R]).all().item())
    same = ok_spans and ok_masks and ok_tokens

    ev = alternate({"a": labelled, "a-": lambda: labelled(False), "b": plain, "c": tokens}, a.reps, lambda fn: event_ms(fn, a.inner))
    wl = alternate({"d": on_host}, 3, wall_ms)
    gbs = lambda m: text_bytes / (m[0] * 1e-3) / 1e9   # noqa: E731
    fmt = lambda m: "%.4f ms (min %.4f, max %.4f) = %.1f GB/s of text" % (m + (gbs(m),))   # noqa: E731
    out = ["# tools/lex_case.py: %d log lines, %.1f MB of text, resident; set `%s` (%d regexps)" % (n, text_bytes / 1e6, SET, R),
           "# (a), (a-), (b), (c) device events around %d back-to-back enqueue-only calls; median (min, max) of %d warmed repetitions," % (
               a.inner, a.reps),
           "# the sides alternating, one run; (d) host wall clock, median of 3",
           "%d matches (%.1f a line), %d entries in token mode (%d gaps)   same answer: spans %s, masks and label counts %s, tokens %s" % (
               matches, matches / n, entries, entries - matches, ok_spans, ok_masks, ok_tokens),
           "label counts, search mode: %s   token mode: %s" % (a_labels.cpu().tolist(), c_labels.cpu().tolist()),
           "(a)  pire_hip_lex, search mode, rows + owners + spans + masks + label counts: %s" % fmt(ev["a"]),
           "(a-) the same without label counts:                                           %s" % fmt(ev["a-"]),
           "(b)  pire_hip_search_all, rows + owners + spans:                              %s" % fmt(ev["b"]),
           "(c)  pire_hip_lex, token mode, all five outputs:                              %s" % fmt(ev["c"]),
           "(a) / (b) = %.3f   (a-) / (b) = %.3f   (c) / (a) = %.3f" % (ev["a"][0] / ev["b"][0], ev["a-"][0] / ev["b"][0], ev["c"][0] / ev["a"][0]),
           "(d)  (b)'s spans fetched, labelled and counted on the host:                   %.1f ms (min %.1f, max %.1f)   ((b) + (d)) / (a) = %.1f" % (
               wl["d"] + ((ev["b"][0] + wl["d"][0]) / ev["a"][0],))]
    text_out = "\n".join(out) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
