#!/usr/bin/env python3
"""Generate tests/golden/glue/* from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): the operands of the Glue
products that tests/test_glue_edges.py builds, and what the reference's own Scanner::Glue makes of them.

  <operand>.blob[.gz]   Scanner::Save() of ONE pattern (gzipped where large)
  abc_left.blob         Scanner::Save() of the reference's glue(glue(a, b), c) of `tiny`'s operands and `x+y`
  cases.json            per operand: pattern (hex of the bytes handed to the lexer), options, file, Size, LettersCount;
                        per pair: lhs, rhs and, read off the table that the reference's left-to-right Scanner::Glue
                        (RefScanner.compile([lhs, rhs], glue_max=m)) built: N, LC, the boundaries h_0 = 1 < h_1 < ... < h_K = N of
                        the breadth-first levels (h_{k+1} = 1 + the largest target of the states below h_k: the numbering is
                        the order of discovery), distinct_k = the number of distinct targets of the states of level k, and, for
                        every max_size of the tests' sweep, whether the reference glued (true) or failed (false).

Run where the reference tree exists:   python tests/golden/make_glue_inputs.py
The fixtures travel with the repo; tests/test_glue_edges.py reads them wherever it runs.
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import OracleScanner, RefScanner  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "glue")

TRIE_FIRST = "pqrstuvwxy"
TRIE_SECOND = [c for c in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz" if c not in "pqrstuvwxyabz"] + list("_,;:!@#%=<>/' ")


def trie_pattern():
    """(w_0|...|w_629)z, w = f + s + the ten bits of 63 j + i in a/b, low bit first: ten first letters that each lead to 63
    second ones, and behind every one of the 630 a tail of its own, so the product's second level is 650 pairs wide."""
    assert len(TRIE_SECOND) == 63 and len(set(TRIE_SECOND)) == 63
    words = []
    for j, f in enumerate(TRIE_FIRST):
        for i, s in enumerate(TRIE_SECOND):
            words.append(f + s + "".join("ab"[((63 * j + i) >> k) & 1] for k in range(10)))
    return "(" + "|".join(words) + ")z"


def classes_pattern():
    """128 symbols with pairwise different behaviour (64 Cyrillic letters = 64 different UTF-8 continuation bytes, 64 ASCII
    bytes), each followed by its own 7-bit code in a/b, then z: the construction of
    tests/test_random_scanners.py::test_many_letter_classes_disable_the_compact_tier, cut to what passes 127 classes."""
    symbols = [chr(0x410 + k) for k in range(64)] + list("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYcdefghijklmnopqrstuvwxy_,;:!@")
    assert len(symbols) == 128 and len(set(symbols)) == 128
    return "(" + "|".join(s + "".join("ab"[(i >> k) & 1] for k in range(7)) for i, s in enumerate(symbols)) + ")z"


# name -> (pattern, options)
OPERANDS = {
    "hello": ("hello\\s+w.+d$", ""),
    "acd": ("[a-c]+d.{2,4}", ""),
    "ab": ("a+b", ""),
    "xy": ("x+y", ""),
    "chain": ("".join("abcdefghijklmnopqrstuvwxyz"[(7 * i) % 26] for i in range(300)), ""),
    "trie": (trie_pattern(), ""),
    "q": ("q", ""),
    "cyr": (classes_pattern(), "u"),
    "cyr_i": ("[а-д]+я", "iu"),
}
# name -> (lhs, rhs, further max_size values to record beside the sweep)
PAIRS = {
    "tiny": ("hello", "acd", []),
    "self": ("ab", "ab", []),
    "chain": ("chain", "xy", []),
    "trie": ("trie", "q", [10, 11, 12]),
    "classes": ("cyr", "cyr_i", []),
}
SWEPT = ("tiny", "trie")


def raw(name):
    pattern, options = OPERANDS[name]
    return pattern.encode("utf-8" if "u" in options else "latin-1"), options


def levels(o):
    """(boundaries, distinct_k) of a table numbered in breadth-first order of discovery, from its own Next"""
    reps, seen = [], set()
    for c in range(264):
        if c != 257 and o.letter_class(c) not in seen:
            seen.add(o.letter_class(c))
            reps.append(c)
    assert o.initial == 0 and len(reps) == o.letters
    bounds, distinct, lo, hi = [1], [], 0, 1
    while lo < hi:
        targets = {o.next(s, c) for s in range(lo, hi) for c in reps}
        distinct.append(len(targets))
        lo, hi = hi, max(hi, max(targets) + 1)
        if hi > lo:
            bounds.append(hi)
    assert bounds[-1] == o.size
    assert len(distinct) == len(bounds)   # the last level is walked too and finds nothing new
    return bounds, distinct


def sweep_values(bounds, extra=()):
    n = bounds[-1]
    vals = {1, 2, n - 2, n - 1, n} | set(extra)
    for h in bounds:
        vals |= {h - 2, h - 1, h}
    return sorted(v for v in vals if v > 0)


def glued(pats, opts, m):
    try:
        return not RefScanner.compile(pats, opts, glue_max=m).empty
    except ValueError as e:
        assert "gluing failed" in str(e), e
        return False


def generate():
    files, doc = {}, {"generator": "tests/golden/make_glue_inputs.py", "operands": {}, "pairs": []}
    for name in OPERANDS:
        pat, opt = raw(name)
        sc = RefScanner.compile([pat], [opt])
        assert sc.regexps == 1 and not sc.empty, name
        blob, fname = sc.save(), name + ".blob"
        if len(blob) >= 16384:
            fname, blob = fname + ".gz", gzip.compress(blob, 9, mtime=0)
        assert len(blob) < (1 << 17), (fname, len(blob))
        files[fname] = blob
        doc["operands"][name] = {"pattern_hex": pat.hex(), "options": opt, "blob": fname, "states": int(sc.size), "letters": int(sc.letters)}
    for name, (lhs, rhs, extra) in PAIRS.items():
        pats, opts = [raw(lhs)[0], raw(rhs)[0]], [raw(lhs)[1], raw(rhs)[1]]
        o = OracleScanner(RefScanner.compile(pats, opts).save())
        bounds, distinct = levels(o)
        entry = {"name": name, "lhs": lhs, "rhs": rhs, "N": int(o.size), "LC": int(o.letters), "boundaries": bounds, "distinct": distinct}
        if name in SWEPT:
            entry["glued_at"] = {str(m): glued(pats, opts, m) for m in sweep_values(bounds, extra)}
        doc["pairs"].append(entry)
        print("%-8s N %5d  LC %3d  levels %3d  widest %d positions" % (name, o.size, o.letters, len(distinct),
              max(b - a for a, b in zip([0] + bounds, bounds)) * o.letters))
    names = ["hello", "acd", "xy"]
    left = RefScanner.compile([raw(n)[0] for n in names], [raw(n)[1] for n in names])
    files["abc_left.blob"] = left.save()
    assert len(files["abc_left.blob"]) < (1 << 16)
    doc["abc_left"] = {"operands": names, "blob": "abc_left.blob", "N": int(left.size), "LC": int(left.letters)}
    files["cases.json"] = (json.dumps(doc, indent=1) + "\n").encode()
    return files


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, data in sorted(generate().items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        print("%8d  %s" % (len(data), name))


if __name__ == "__main__":
    main()
