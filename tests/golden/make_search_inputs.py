#!/usr/bin/env python3
"""Generate tests/golden/search/* from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): the scanner pairs of the
leftmost-longest search (pire_hip_search), neither of them Surround()ed.  Per pair:

  <name>.n.blob     Scanner::Save() of `re`, option `n`                    (F: the forward leg, LongestPrefix / ShortestPrefix)
  <name>.nr.blob    Scanner::Save() of `(re).*`, options `nr`: compiled from Fsm::Reverse()   (R: the backward leg, LongestSuffix)
  (gzipped where a blob is large, as tests/golden does)

Run where the reference tree exists:   python tests/golden/make_search_inputs.py
The fixtures travel with the repo; tests/test_search.py reads them wherever it runs.

  ipv4.slow.blob   SlowCapturingScanner::Save() of the Surround()ed `.*?(re)` of the pair `ipv4`: the one-call route to the same
               answer without the search, the yardstick of tools/search_case.py (written by oracle/_ref/bin/slow_capture_golden,
               `make -C tests/cpp slow_capture_golden`, as tests/golden/make_slow_capture_inputs.py has its blobs written)
  cases.json   per pair: name, pattern, the pair's option bits (B = 2: throughBeginMark, E = 4: throughEndMark), files, the
               reference's Size() of both -- and, for every probe string, what the reference's LongestSuffix(R) answers ("tail")
               and then what its LongestPrefix(F) / ShortestPrefix(F) answer on the strings cut at len - tail ("longest",
               "shortest"; -1 where tail is -1): the recorded truth of the composition in include/pire_hip.h.
"""
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import RefScanner, pack_strings  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "search")
B, E = 2, 4   # PIRE_HIP_SEARCH_THROUGH_BEGIN / _THROUGH_END


def draw_words(count=320, seed=20240613):
    """`count` distinct words of 4-9 letters over ten letters: an alternation whose scanners have more than 255 states in BOTH
    forms, so both legs of the search leave the dense rows (64 words gave 198 / 293 states)."""
    rng = random.Random(seed)
    words = set()
    while len(words) < count:
        words.add("".join(rng.choice("abcdefghij") for _ in range(rng.randint(4, 9))))
    return sorted(words)


WORDS = draw_words()

# name -> (pattern, option bits of the pair)
PAIRS = {
    "num": ("[0-9]+", 0),
    "stamp": ("[0-9]{4}-[0-9]{2}-[0-9]{2}", 0),
    "alt": ("abc|abcabc|b+", 0),                 # leftmost-LONGEST: [0, 6) on abcabc, where leftmost-first engines say [0, 3)
    "blanks_star": ("[ \\t]*", 0),               # accepts the empty string: every string is found
    "arrow": ("-->", 0),
    "gap": ("a.*b", 0),                          # the forward leg never dies: it walks to the string's end
    "eol": ("[a-z]+$", E),
    "bol": ("^[ \\t]+", B),
    "words": ("|".join(WORDS), 0),
    "ipv4": ("[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}\\.[0-9]{1,3}", 0),   # tools/search_case.py's pattern
}
SLOW_BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "slow_capture_golden")

# the empty string, a lone byte, a match at 0, at the end, over the whole string, two matches, none -- for every pair
PROBES = [b"", b"7", b"a", b"b", b" ", b"-", b"x",
          b"12", b"12ab", b"ab12", b"a1b22c", b"no digits",
          b"2024-01-02", b"2024-01-02 x", b"x 2024-01-02", b"on 2024-01-02 and 2025-11-30.", b"2024-01-0",
          b"abcabc", b"xabcabcx", b"zabcz bbb", b"bbb", b"abcab", b"ac",
          b"-->", b"-->a-->", b"x-->", b"-->x", b"a--b->",
          b" \t x \t", b"\t", b"x  ", b"  x", b"  ",
          b"ab", b"axxb", b"a b a b", b"xaxbx", b"ba", b"aaa",
          b"hello", b"hello world", b"9 lives", b"trail9 end", b"END", b"a1",
          b"  lead", b"\tlead and  more", b"x \t",
          b"10.0.0.1", b"from 192.168.1.254:80", b"1.2.3", b"1234.5.6.7.8 9.9.9.9",
          WORDS[0].encode(), b"x" + WORDS[1].encode(), WORDS[2].encode() + b"x", WORDS[3].encode() + b" " + WORDS[4].encode(),
          b"xy" + WORDS[5].encode()[:-1] + b"z" + WORDS[6].encode() + b"q", WORDS[7].encode()[:-1], b"klmnop"]


def cut(strings, tails):
    """the strings from len - tail on (empty where tail is -1), and where each starts"""
    starts = [len(s) - int(t) if t >= 0 else len(s) for s, t in zip(strings, tails)]
    return [s[b:] for s, b in zip(strings, starts)], starts


def forward(sc, strings, tails, longest, opts):
    """LongestPrefix / ShortestPrefix of the reference on the cut strings; throughBeginMark only where the cut is at 0"""
    tails_cut, starts = cut(strings, tails)
    text, offs = pack_strings(tails_cut)
    plain = sc.prefix(text, offs, longest, False, bool(opts & E))
    marked = sc.prefix(text, offs, longest, True, bool(opts & E)) if opts & B else plain
    return [-1 if t < 0 else int(m if b == 0 else p) for t, b, p, m in zip(tails, starts, plain, marked)]


def slow_capture_blob(pattern):
    """SlowCapturingScanner::Save() of the Surround()ed `.*?(pattern)`, capture 1"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "slow_capture_golden"], check=True, stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as tmp:
        req = os.path.join(tmp, "request.txt")
        with open(req, "w") as f:
            f.write("case slow 1 %s\ns %s\nend\n" % ((".*?(%s)" % pattern).encode().hex(), b"at 10.0.0.1".hex()))
        out = subprocess.run([SLOW_BIN, "gen", req, tmp], check=True, stdout=subprocess.PIPE, text=True).stdout
        assert "r 1 3 11 1" in out, out                      # captured [3, 11) of the one string
        with open(os.path.join(tmp, "slow.blob"), "rb") as f:
            return f.read()


def generate():
    """{file name: bytes} of everything under tests/golden/search"""
    files, cases = {}, []
    files["ipv4.slow.blob"] = slow_capture_blob(PAIRS["ipv4"][0])
    assert len(files["ipv4.slow.blob"]) < (1 << 16)
    text, offs = pack_strings(PROBES)
    for name, (pattern, opts) in PAIRS.items():
        fwd = RefScanner.compile([pattern], ["n"])
        rev = RefScanner.compile(["(%s).*" % pattern], ["nr"])
        assert fwd.regexps == 1 and rev.regexps == 1 and not fwd.empty and not rev.empty, name
        if name == "words":
            assert fwd.size > 255 and rev.size > 255, (fwd.size, rev.size)
        entry = {"name": name, "pattern": pattern if name != "words" else None, "words": WORDS if name == "words" else None, "opts": opts,
                 "fwd_states": int(fwd.size), "rev_states": int(rev.size)}
        for form, sc in (("n", fwd), ("nr", rev)):
            blob = sc.save()
            fname = "%s.%s.blob" % (name, form)
            if len(blob) >= 8192:
                fname, blob = fname + ".gz", gzip.compress(blob, 9, mtime=0)
            assert len(blob) < (1 << 19), (fname, len(blob))
            files[fname] = blob
            entry["fwd" if form == "n" else "rev"] = fname
        tails = [int(x) for x in rev.suffix(text, offs, True, bool(opts & E), bool(opts & B))]
        entry["tail"] = tails
        entry["longest"] = forward(fwd, PROBES, tails, True, opts)
        entry["shortest"] = forward(fwd, PROBES, tails, False, opts)
        cases.append(entry)
    doc = {"generator": "tests/golden/make_search_inputs.py", "probes_hex": [p.hex() for p in PROBES], "pairs": cases}
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
