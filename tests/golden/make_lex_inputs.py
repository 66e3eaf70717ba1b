#!/usr/bin/env python3
"""Generate tests/golden/lex/* from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): the scanner pairs of the
labelled search and of the tokenizer (pire_hip_lex), neither of them Surround()ed.  Per set of R regexps:

  <set>.n.blob     Scanner::Save() of Scanner::Glue over the R regexps in order, option `n`   (F: the forward leg and the labels)
  <set>.nr.blob    Scanner::Save() of `((re_0)|(re_1)|...).*`, options `nr`: compiled from Fsm::Reverse()   (R: the backward leg)
  (gzipped where a blob is large, as tests/golden does; `r65` has the forward blob only: it is there to be refused)

Run where the reference tree exists:   python tests/golden/make_lex_inputs.py
The fixtures travel with the repo; tests/test_lex.py reads them wherever it runs.

  cases.json   the probes (those of tests/golden/make_search_inputs.py and, behind them, the examples of include/pire_hip.h) and
               per set: name, patterns, option bits (B = 2, E = 4), files, the reference's Size() of both tables, and for every
               probe the entries [begin, end, [accepted regexp ids]] of the loops of include/pire_hip.h -- "search" and "tokens"
               with the set's own bits, "search_shortest" and "tokens_shortest" with S added.  A gap has no ids.  The loops are
               computed through the reference's own LongestSuffix, LongestPrefix / ShortestPrefix, Next, Final and
               AcceptedRegexps (oracle.binding.RefScanner).
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import BEGIN_MARK, END_MARK, RefScanner, pack_strings  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_search_inputs as MS  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lex")
S, B, E = 1, 2, 4   # PIRE_HIP_LEX_SHORTEST / _THROUGH_BEGIN / _THROUGH_END

WORDS = MS.draw_words()
IPV4 = MS.PAIRS["ipv4"][0]

# name -> (patterns, option bits of the set)
SETS = {
    "lexer3": (["[a-z]+", "[0-9]+", "[ \\t]+"], 0),
    "kw": (["if|else|while", "[a-z]+"], 0),                    # masks with two bits
    "alt3": (["abc", "abcabc", "b+"], 0),                      # the longest match wins over the order of the regexps
    "ipnum": ([IPV4, "[0-9]+"], 0),
    "eol": (["[a-z]+$", "[0-9]+"], E),
    "ends": (["[a-z]+", "[a-z]+$"], E),                        # the OR of both states
    "bol": (["^#", "[a-z]+"], B),
    "words2": (["|".join(WORDS[:len(WORDS) // 2]), "|".join(WORDS[len(WORDS) // 2:])], 0),   # both legs outside the dense rows
    "r64": (["k%02d" % i for i in range(64)], 0),              # bit 63
    "r65": (["k%02d" % i for i in range(65)], 0),              # one regexp too many: the forward blob only
}

EXAMPLES = [b"if iffy 10 else x9", b"abcabc bb abc", b"from 10.0.0.1:80 x 10.0.0", b"  ?? a1!", b"ab 12 cd", b"ab cd", b"12 ab",
            b"#ab #c", b"x#", b"k00 k63k01 k6", b"k63", b"while(x) else9 elsewhere",
            WORDS[200].encode(), WORDS[3].encode() + b" " + WORDS[300].encode() + WORDS[301].encode()[:-1]]
PROBES = MS.PROBES + EXAMPLES


def accepted_after(F, s, b, h, opts):
    """the ids of the entry [b, b + h) of s: AcceptedRegexps of F's state after its bytes, and of the state behind the EndMark
    where the entry ends the string"""
    st = F.initial
    if opts & B and b == 0:
        st = F.next(st, BEGIN_MARK)
    for c in s[b:b + h]:
        st = F.next(st, c)
    ids = set(F.accepted(st)) if F.final(st) else set()
    if opts & E and b + h == len(s):
        end = F.next(st, END_MARK)
        if F.final(end):
            ids |= set(F.accepted(end))
    assert ids, (s, b, h)
    return sorted(ids)


def prefix_at(F, s, b, opts):
    text, offs = pack_strings([s[b:]])
    return int(F.prefix(text, offs, not (opts & S), bool(opts & B) and b == 0, bool(opts & E))[0])


def search_loop(R, F, s, opts):
    """include/pire_hip.h, search mode, line by line"""
    out, p = [], 0
    while p < len(s):
        text, offs = pack_strings([s[p:]])
        t = int(R.suffix(text, offs, True, bool(opts & E), bool(opts & B) and p == 0)[0])
        if t <= 0:
            break
        b = len(s) - t
        h = prefix_at(F, s, b, opts)
        if h < 0:
            break
        if h > 0:
            out.append([b, b + h, accepted_after(F, s, b, h, opts)])
        p = b + max(h, 1)
    return out


def token_loop(F, s, opts):
    """include/pire_hip.h, token mode, line by line: a maximal run of gap bytes is one entry without ids"""
    out, p, gap = [], 0, None
    while p < len(s):
        h = prefix_at(F, s, p, opts)
        if h > 0:
            if gap is not None:
                out.append([gap, p, []])
                gap = None
            out.append([p, p + h, accepted_after(F, s, p, h, opts)])
            p += h
        else:
            gap = p if gap is None else gap
            p += 1
    if gap is not None:
        out.append([gap, len(s), []])
    return out


def generate():
    """{file name: bytes} of everything under tests/golden/lex"""
    files, cases = {}, []
    for name, (patterns, opts) in SETS.items():
        fwd = RefScanner.compile(patterns, ["n"] * len(patterns))
        assert fwd.regexps == len(patterns) and not fwd.empty, name
        entry = {"name": name, "patterns": patterns if name != "words2" else None, "opts": opts, "regexps": len(patterns),
                 "fwd_states": int(fwd.size)}
        forms = [("n", fwd)]
        rev = None
        if name != "r65":
            rev = RefScanner.compile(["(%s).*" % "|".join("(%s)" % p for p in patterns)], ["nr"])
            assert rev.regexps == 1 and not rev.empty, name
            entry["rev_states"] = int(rev.size)
            forms.append(("nr", rev))
        if name == "words2":
            assert fwd.size > 255 and rev.size > 255, (fwd.size, rev.size)
        for form, sc in forms:
            blob = sc.save()
            fname = "%s.%s.blob" % (name, form)
            if len(blob) >= 8192:
                fname, blob = fname + ".gz", gzip.compress(blob, 9, mtime=0)
            assert len(blob) < (1 << 19), (fname, len(blob))
            files[fname] = blob
            entry["fwd" if form == "n" else "rev"] = fname
        if rev is not None:
            for key, o in (("", opts), ("_shortest", opts | S)):
                entry["search" + key] = [search_loop(rev, fwd, p, o) for p in PROBES]
                entry["tokens" + key] = [token_loop(fwd, p, o) for p in PROBES]
        cases.append(entry)
    doc = {"generator": "tests/golden/make_lex_inputs.py", "base_probes": len(MS.PROBES), "words": WORDS,
           "probes_hex": [p.hex() for p in PROBES], "sets": cases}
    files["cases.json"] = (json.dumps(doc) + "\n").encode()
    assert len(files["cases.json"]) < (1 << 19)
    return files


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, data in sorted(generate().items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        print("%8d  %s" % (len(data), name))


if __name__ == "__main__":
    main()
