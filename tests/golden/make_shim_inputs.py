#!/usr/bin/env python3
"""Generate tests/golden/shim_inputs/* from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): the scanners and
the string lists of tests/cpp/select_shim_test.cpp and tests/cpp/route_shim_test.cpp, and what the reference answers on them.

Run where the reference tree exists:   python tests/golden/make_shim_inputs.py
The fixtures travel with the repo; tests/test_hit_pass_shim_inputs.py reads them wherever it runs.

  <scanner>.blob           Scanner::Save() of the patterns compiled and glued left to right, the order the shim tests glue in
  <scanner>__<list>.json   per string of the list: Runner(sc).Begin().Run(s).End() -> StateIndex, Final, AcceptedRegexps (a hex
                           mask, bit r <=> regexp r accepted).  The strings themselves are NOT stored: LISTS below restates the
                           formulas of main() of the two programs, and the file carries the SHA-256 of the packed list.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import RefScanner, pack_strings  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim_inputs")
LONG = b"x" * 3000 + b"abc" + b"y" * 70   # the one string that takes the scan's long-string paths
LETTERS = "abcdefghij"


def select_text():
    """select_shim_test.cpp main(): `text`"""
    out = [b"def abc ghi", b"abc", b"def abd ghi", b"abc ghi", b"def abc", b"xaez", b"xadddddddddddez", b"xx", b"xxx", b"", b"hello world",
           b"aaa", b"bbb", b"aaabbb", b"ccc", b"aaacccbbb", b"HeadInnerInnerTail", LONG]
    for i in range(700):
        out.append(b"..aaa.." if i % 7 == 0 else b"bbbccc" if i % 11 == 0 else b"abc" if i % 13 == 0 else b"nothing here")
    return out


def route_text():
    """route_shim_test.cpp main(): `text`"""
    out = [b"def abc ghi", b"abc", b"aaa", b"bbb", b"aaabbb", b"ccc", b"aaacccbbb", b"", b"xx", LONG]
    for i in range(2300):
        out.append(b"..aaa.." if i % 7 == 0 else b"bbbccc" if i % 11 == 0 else b"abc aaa bbb ccc" if i % 13 == 0 else b"nothing here")
    return out


def dense():
    """route_shim_test.cpp main(): `dense`"""
    return [b"aaa"] * 3000


def pairs():
    """select_shim_test.cpp main(): `pairs`"""
    return [b"zz" if i % 5 == 0 else (LETTERS[(i * 7) % 10] + LETTERS[(i * 3) % 10]).encode() for i in range(1500)]


LISTS = {"select_text": select_text, "route_text": route_text, "dense": dense, "pairs": pairs}

# name -> (patterns in gluing order, options, RegexpsCount the shim tests check)
SCANNERS = {
    "abc": (["abc"], [""], 1),
    "aaa_bbb_ccc": (["aaa", "bbb", "ccc"], [""] * 3, 3),
    "aaa_bbb_ccc_abc": (["aaa", "bbb", "ccc", "abc"], [""] * 4, 4),
    "two_letters_70": ([LETTERS[a] + LETTERS[b] for a in range(10) for b in range(7)], ["n"] * 70, 70),
}

BE = 3   # PIRE_HIP_RUN_BEGIN | PIRE_HIP_RUN_END: Runner(sc).Begin().Run(s).End(), what the two programs do

# every (scanner, list, run flags) the two programs Compare() -- and the 70 patterns once more WITHOUT the begin and end marks:
# they are compiled as they stand (not Surround()ed: the product of 70 surrounded patterns does not fit the reference's glue
# limit), so Begin() takes every string to the dead state and the reference accepts nothing on that list.  The programs'
# comparison of two mask words is therefore one of empty lists; the unmarked run of the same list is what has hits in both words.
PAIRS = [("abc", "select_text", BE), ("aaa_bbb_ccc", "select_text", BE), ("two_letters_70", "pairs", BE), ("two_letters_70", "pairs", 0),
         ("abc", "route_text", BE), ("aaa_bbb_ccc_abc", "route_text", BE), ("aaa_bbb_ccc_abc", "dense", BE)]
ALL_EMPTY = [("two_letters_70", "pairs", BE)]   # the reference's own answer, asserted below: no row has a member


def pair_name(scanner, which, flags):
    return "%s__%s%s" % (scanner, which, "" if flags == BE else "__unmarked")


def list_sha256(strings):
    """SHA-256 of the packed list: its offsets (uint64, little endian) followed by its text"""
    text, offs = pack_strings(strings)
    return hashlib.sha256(offs.astype("<u8").tobytes() + text.tobytes()).hexdigest()


def answer(sc, regexps, scanner, which, flags):
    """The JSON record of one (scanner, list, flags), from the reference alone"""
    strings = LISTS[which]()
    text, offs = pack_strings(strings)
    idx, fin = sc.run(text, offs, flags=flags)
    mask_of = {}
    for s in np.unique(idx).tolist():
        acc = sc.accepted(int(s))
        assert all(r < regexps for r in acc), (scanner, s, acc)
        mask_of[s] = sum(1 << r for r in acc)
    masks = [mask_of[int(s)] for s in idx]
    rows = [sum((m >> r) & 1 for m in masks) for r in range(regexps)]
    if (scanner, which, flags) in ALL_EMPTY:
        assert not any(rows) and not fin.any(), (scanner, which, rows)
    else:
        assert any(rows), (scanner, which, "every row is empty: the pair pins nothing")
    if scanner == "two_letters_70" and flags == 0:
        assert any(rows[:64]) and any(rows[64:]), (rows, "hits in both mask words")
    if (scanner, which) == ("aaa_bbb_ccc_abc", "route_text"):
        assert all(rows), (rows, "the isolation cases of the test want all four rows")
    return {"generator": "tests/golden/make_shim_inputs.py", "scanner": scanner, "list": which, "flags": flags, "n": len(strings), "regexps": regexps,
            "sha256": list_sha256(strings), "row_counts": rows, "idx": [int(x) for x in idx], "final": [int(x) for x in fin],
            "masks": ["%x" % m for m in masks]}


def generate():
    """{file name: bytes} of everything under tests/golden/shim_inputs"""
    files, compiled = {}, {}
    for name, (patterns, options, regexps) in SCANNERS.items():
        sc = RefScanner.compile(patterns, options)
        assert sc.regexps == regexps and not sc.empty, (name, sc.regexps, sc.empty)
        compiled[name] = sc
        files[name + ".blob"] = sc.save()
    for scanner, which, flags in PAIRS:
        rec = answer(compiled[scanner], SCANNERS[scanner][2], scanner, which, flags)
        files[pair_name(scanner, which, flags) + ".json"] = (json.dumps(rec, separators=(",", ":")) + "\n").encode()
    return files


def main():
    os.makedirs(OUT, exist_ok=True)
    files = generate()
    for name, data in sorted(files.items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        print("%8d  %s" % (len(data), name))


if __name__ == "__main__":
    main()
