#!/usr/bin/env python3
"""Generate tests/golden/search_all/cases.json from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): every
leftmost-longest match of every probe (pire_hip_search_all), for the scanner pairs of tests/golden/search.  It reads those
pairs and their blobs and adds none.

Run where the reference tree exists:   python tests/golden/make_search_all_inputs.py
The fixture travels with the repo; tests/test_search_all.py reads it wherever it runs.

  cases.json   the probes -- those of tests/golden/search/cases.json and, behind them, strings with many matches -- and per
               pair, for the pair's own option bits ("matches") and with S added ("matches_shortest"), the answer of the loop of
               include/pire_hip.h for every probe: a list of [begin, end).  The loop is computed through the reference's own
               LongestSuffix and LongestPrefix / ShortestPrefix (oracle.binding.RefScanner.suffix / .prefix), one call per
               round over all the strings that are still walking.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import RefScanner, pack_strings  # noqa: E402
from tests import helpers as H  # noqa: E402

SEARCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search_all")
S, B, E = 1, 2, 4   # PIRE_HIP_SEARCH_SHORTEST / _THROUGH_BEGIN / _THROUGH_END


def many_match_probes(words):
    w = [x.encode() for x in words[:8]]
    return [b"a1b22c333", b" ".join(b"%d" % i for i in range(1, 41)), b"abcabcabc bb abc", b"x  y \t", b"-->-->x-->",
            b"from 2024-01-02 to 2024-02-03, not 2025-11-30x", b"10.0.0.1 10.0.0.2, 192.168.1.254", b" ".join(w), b"".join(w)]


def search_all_loop(R, F, strings, opts):
    """include/pire_hip.h, line by line, for all strings at once: [[(begin, end), ...] per string]"""
    n = len(strings)
    p = [0] * n
    out = [[] for _ in range(n)]
    live = [i for i in range(n) if len(strings[i]) > 0]
    while live:                                                                 # while p < len
        text, offs = pack_strings([strings[i][p[i]:] for i in live])
        plain = R.suffix(text, offs, True, bool(opts & E), False)
        marked = R.suffix(text, offs, True, bool(opts & E), True) if opts & B else plain
        t = [int(marked[k] if p[i] == 0 else plain[k]) for k, i in enumerate(live)]
        b = [len(strings[i]) - tk for i, tk in zip(live, t) if tk > 0]
        live = [i for i, tk in zip(live, t) if tk > 0]                          # t <= 0: stop
        if not live:
            break
        text, offs = pack_strings([strings[i][bi:] for i, bi in zip(live, b)])
        plain = F.prefix(text, offs, not (opts & S), False, bool(opts & E))
        marked = F.prefix(text, offs, not (opts & S), True, bool(opts & E)) if opts & B else plain
        nxt = []
        for k, (i, bi) in enumerate(zip(live, b)):
            h = int(marked[k] if bi == 0 else plain[k])
            if h < 0:                                                           # h < 0: stop
                continue
            if h > 0:
                out[i].append((bi, bi + h))
            p[i] = bi + max(h, 1)
            if p[i] < len(strings[i]):
                nxt.append(i)
        live = nxt
    return out


def generate():
    with open(os.path.join(SEARCH, "cases.json")) as f:
        base = json.load(f)
    words = next(c for c in base["pairs"] if c["name"] == "words")["words"]
    probes = [bytes.fromhex(h) for h in base["probes_hex"]] + many_match_probes(words)
    pairs = []
    for c in base["pairs"]:
        R = RefScanner.load(H.load_blob(os.path.join("search", c["rev"])))
        F = RefScanner.load(H.load_blob(os.path.join("search", c["fwd"])))
        entry = {"name": c["name"], "opts": c["opts"]}
        for key, opts in (("matches", c["opts"]), ("matches_shortest", c["opts"] | S)):
            entry[key] = [[list(m) for m in ms] for ms in search_all_loop(R, F, probes, opts)]
        pairs.append(entry)
    doc = {"generator": "tests/golden/make_search_all_inputs.py", "base_probes": len(base["probes_hex"]),
           "probes_hex": [p.hex() for p in probes], "pairs": pairs}
    return (json.dumps(doc) + "\n").encode()


def main():
    os.makedirs(OUT, exist_ok=True)
    data = generate()
    assert len(data) < (1 << 19)
    with open(os.path.join(OUT, "cases.json"), "wb") as f:
        f.write(data)
    print("%8d  cases.json" % len(data))


if __name__ == "__main__":
    main()
