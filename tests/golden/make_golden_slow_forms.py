#!/usr/bin/env python3
"""Golden fixtures that reach every launch form of the SlowScanner kernels (slow.hip PlanSlow), generated
with the unmodified reference (oracle/_ref).  Beside make_golden_slow_wide.py, and separate for the same reason: the
other fixtures stay byte-identical.

    python tests/golden/make_golden_slow_forms.py      (needs the reference library: runs in the build container only)

Writes tests/golden/slow_forms.json and the files it names under tests/golden/blobs/.  Per case: the blob, the strings
(hex in the JSON for the automata of up to 256 states, one gzipped file of the concatenated text plus the lengths for
the large ones), `final`, and a SHA-256 of every string's state bits.  Then four blobs without strings ("slow_lanes").

Strings of a case: the empty string, one byte, the pattern's head followed by gap - 1, gap and gap + 1 bytes (only the
middle one matches), and random strings over the pattern's letters and a few others in which the head is planted at a
density drawn per string: from a couple of live threads to dozens, so that the 16-slot list and the 4-slot lane list both
hold some strings and give up on others."""
import gzip
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.binding import RefSlowScanner  # noqa: E402

A20 = "abcdefghijklmnopqrst"
A36 = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJ"
A64 = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-"

# name, head (the literal in front of the gap), gap, large (more than 256 states: few, long strings)
CASES = [
    ("forms_masks_in_memory", A20, 110, False),
    ("forms_tables_in_memory", A36, 100, False),
    ("forms_tables_in_memory_no_list", A64, 90, False),
    ("forms_x124", "x", 124, False),
    ("forms_x125", "x", 125, True),
    ("forms_x1020", "x", 1020, True),
    ("forms_x1021", "x", 1021, True),
    ("forms_x3000", "x", 3000, True),
    ("forms_x21000", "x", 21000, True),
]

# blobs only, for the tests that build their own records: one automaton per width of the bitset kernel's lane (K = 1, 2, 4, 8 words)
LANES = [("forms_x10", "x.{10}$"), ("forms_x20", "x.{20}$"), ("forms_x50", "x.{50}$"), ("forms_x120", "x.{120}$")]

MAX_COMMITTED = 1 << 20


def strings_for(head, gap, large, rng):
    head = head.encode()
    others = np.frombuffer(b"yz Q.,\n" + (b"" if len(head) == 1 else head[:3] + head[-2:]), dtype=np.uint8)
    out = [b"", head[:1]] + [b"z" + head + b"y" * k for k in (gap - 1, gap, gap + 1)]
    count, top = (20, gap + 100) if large else (200, 2 * gap)
    for i in range(count):
        k = int(rng.randint(0, top + 1)) if i % 4 else top        # every fourth at full length: the longest-lived sets
        body = bytearray(others[rng.randint(0, len(others), size=k)].tobytes())
        alive = (1, 3, 8, 14, 15, 16, 17, 24, 40)[i % 9]          # heads wanted inside one gap
        step = max(len(head), gap // alive)
        at = int(rng.randint(0, step))
        while at + len(head) <= k:
            body[at:at + len(head)] = head
            at += int(rng.randint(len(head), 2 * step - len(head) + 2))
        out.append(bytes(body))
    return out


def write_gz(rel, data):
    os.makedirs(os.path.join(HERE, "blobs"), exist_ok=True)
    packed = gzip.compress(data, 9, mtime=0)
    with open(os.path.join(HERE, rel), "wb") as f:
        f.write(packed)
    return len(packed)


def main():
    cases = []
    for name, head, gap, large in CASES:
        pat = "%s.{%d}$" % (head, gap)
        sc = RefSlowScanner.compile(pat, "")
        assert (sc.size > 256) == large, (name, sc.size)
        blob = sc.save()
        rng = np.random.RandomState(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
        strings = strings_for(head, gap, large, rng)
        fin, bits = sc.run_strings(strings, threads=8)
        assert [int(x) for x in fin[:5]] == [0, 0, 0, 1, 0], (name, fin[:5])
        case = {"name": name, "pattern": pat, "options": "", "head": head, "gap": gap,
                "geometry": {"states": sc.size, "letters": sc.letters, "words": sc.words},
                "blob_sha256": hashlib.sha256(blob).hexdigest(), "blob_bytes": len(blob)}
        rel = os.path.join("blobs", name + ".slow.blob.gz")
        packed = len(gzip.compress(blob, 9, mtime=0))
        assert packed <= MAX_COMMITTED, (name, packed)     # x.{21000}$: 1.7 MB raw, 0.18 MB gzipped
        write_gz(rel, blob)
        case["blob"] = rel
        if large:
            case["strings_gz"] = os.path.join("blobs", name + ".strings.gz")
            case["lengths"] = [len(s) for s in strings]
            write_gz(case["strings_gz"], b"".join(strings))
        else:
            case["strings_hex"] = [s.hex() for s in strings]
        case["final"] = [int(x) for x in fin]
        case["bits_sha256"] = [hashlib.sha256(bytes(np.ascontiguousarray(b))).hexdigest() for b in bits]
        cases.append(case)
        print(name, "states", sc.size, "letters", sc.letters, "words", sc.words, "blob", len(blob), "gz", packed,
              "strings", len(strings), "finals", int(sum(fin)))
    lanes = []
    for name, pat in LANES:
        sc = RefSlowScanner.compile(pat, "")
        blob = sc.save()
        rel = os.path.join("blobs", name + ".slow.blob.gz")
        write_gz(rel, blob)
        lanes.append({"name": name, "pattern": pat, "options": "", "gap": int(pat[3:-2]),
                      "geometry": {"states": sc.size, "letters": sc.letters, "words": sc.words},
                      "blob": rel, "blob_sha256": hashlib.sha256(blob).hexdigest()})
        print(name, "states", sc.size, "letters", sc.letters, "words", sc.words, "blob", len(blob))
    with open(os.path.join(HERE, "slow_forms.json"), "w") as f:
        json.dump({"slow_forms": cases, "slow_lanes": lanes}, f, indent=1)


if __name__ == "__main__":
    main()
