#!/usr/bin/env python3
"""Generate tests/golden/slow_capture/* from the UNMODIFIED reference: what Pire::SlowCapturingScanner (pire/extra/capture.h)
answers, as data.  The scanners are compiled and run by tests/cpp/slow_capture_golden.cpp (`make -C tests/cpp
slow_capture_golden` -> oracle/_ref/bin/slow_capture_golden), as the reference's own capture test compiles and runs them.

Run where the reference tree exists:   python tests/golden/make_slow_capture_inputs.py
The fixtures travel with the repo; tests/test_slow_capture.py reads them wherever it runs.

  <name>.blob    SlowCapturingScanner::Save() of the case's pattern (with the action area)
  cases.json     per case: name, pattern, capture index, `always`, blob, the reference's Size() / GetLettersCount() / GetStart(),
                 `gap` (the wide cases), the number of its strings, the SHA-1 of their concatenation with lengths, and `first`: where
                 its rows start in expected.i16
  expected.i16   int16[strings][5], little endian: per string captured, begin, end, matched, live -- GetCapture()'s return,
                 final.GetBegin() / GetEnd() (-1 for npos and where nothing was assigned), whether `final` was assigned, and the
                 longest state list the walk held on that string
The strings themselves are not stored: `case_strings(name, gap)` below makes them, from the table CASES and a generator written
out here (`Lcg`), and the test calls the same function and holds the SHA-1.

A case in which no string captures is refused, and so is one in which every string captures unless it is marked `always`.
The one exception is marked `never`: under A|(A) the reference matches every string that holds an A and captures in none --
the uncaptured branch has the priority --, which is what the pair (A)|A, A|(A) is there to show; that case is refused unless some
string matches without capturing.
"""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slow_capture")
BIN = os.path.join(ROOT, "oracle", "_ref", "bin", "slow_capture_golden")
SEED = 20261020

PREF_TEXT = b"pref ala bla pref cla suff dla"
UTF8_RE = ("\u0417\u0434\u0440\u0430\u0432\u0441\u0442\u0432\u0443\u0439\u0442\u0435, ((\\s|\\w|[()]|-)+)!").encode("utf-8")
UTF8_TEXT = ("    \u0417\u0434\u0440\u0430\u0432\u0441\u0442\u0432\u0443\u0439\u0442\u0435, "
             "\u0423\u0432\u0430\u0436\u0430\u0435\u043c\u044b\u0439 (-\u0430\u044f)!   ").encode("utf-8")

# name, pattern, capture index, alphabet of the random strings, the reference's own texts, always (or "never")
CASES = [
    ("lazy_pref", b".*?(pref.*suff)", 1, b"prefsu ", [PREF_TEXT], False),
    ("greedy_pref", b".*(pref.*suff)", 1, b"prefsu ", [PREF_TEXT], False),
    ("or_first", b"(A)|A", 1, b"AB", [b"A"], False),
    ("or_second", b"A|(A)", 1, b"AB", [b"A"], "never"),
    ("vk", b"^http://vk(ontakte[.]ru|[.]com)/id(\\d+)([^0-9]|$)", 2, b"htp:/vk.comid0159",
     [b"http://vkontakte.ru/id100500", b"http://vk.com/id7", b"http://vk.com/id77x", b"xhttp://vk.com/id7"], False),
    ("google_id", b"google_id\\s*=\\s*['\"]([a-z0-9]+)['\"]\\s*;", 1, b"google_id ='\"a0;",
     [b"google_id = 'abcde';", b"var google_id = 'abcde'; eval(google_id);", b"google_id != 'abcde';", b"google_id=\"a0\";"], False),
    ("utf8", UTF8_RE, 1, b" ()-!,ab", [UTF8_TEXT, UTF8_TEXT[4:-3], UTF8_TEXT.replace(b"!", b"?")], False),
    ("lazy_ab_1", b".*?(a+?)(b*)c", 1, b"abc", [], False),
    ("lazy_ab_2", b".*?(a+?)(b*)c", 2, b"abc", [], False),
    ("alt_cd", b"(a|ab)(c|bcd)(d*)", 2, b"abcd", [b"abcd"], False),
    ("greedy_alt", b".*(ab|a)(b?)c+?", 1, b"abc", [], False),
    ("rep_group", b"x*?(a.{3}b)+", 1, b"xab", [], False),
    ("lazy_class", b"[ab]*?((ab)+|b)a", 1, b"abc", [], False),
    ("id", b".*?id=(\\d+?)\\d*&", 1, b"id=12&", [b"GET /x?id=12345&y=2", b"id=&", b"id=7&id=8&"], False),
    ("star", b"(a*)", 1, b"ab", [b"", b"aaa"], True),
    ("anchored_lazy", b"^(a*?)b", 1, b"ab", [], False),
]
WIDE = {"wide": 70, "wide64": None, "wide65": None}            # name -> gap of .*?(a.{gap}b); None: found by asking (generate)
NAMES = tuple(c[0] for c in CASES) + tuple(WIDE)


class Lcg:
    """Knuth's 64-bit linear congruential generator, its upper bits: the same strings under every Python"""

    def __init__(self, seed):
        self.x = seed & (2 ** 64 - 1)

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n

    def string(self, alphabet, length):
        return bytes(alphabet[self.below(len(alphabet))] for _ in range(length))

    def strings(self, alphabet, count, longest):
        return [self.string(alphabet, self.below(longest + 1)) for _ in range(count)]


def wide_pattern(gap):
    return b".*?(a.{%d}b)" % gap


def case_strings(name, gap=None):
    """The strings of a case: the reference's own texts, then 256 random strings of 0..48 bytes over the case's alphabet (an
    empty one among them).  wide: the string that fills the state list (a^(2 * gap + 10) b), every length 0..200 over {a, b, c},
    24 planted matches.  wide64 / wide65: the filling string, a^n b around the gap, 32 random strings over {a, b}."""
    rng = Lcg(SEED + NAMES.index(name))
    if name == "wide":
        out = [b"a" * (2 * gap + 10) + b"b"] + [rng.string(b"abc", n) for n in range(201)]
        for _ in range(24):
            head = rng.string(b"abc", rng.below(41))
            out.append(head + b"a" + rng.string(b"abc", gap) + b"b" + head[:7])
        return out
    if name in WIDE:
        return [b"a" * (2 * gap + 10) + b"b"] + [b"a" * n + b"b" for n in range(gap - 2, gap + 8)] + rng.strings(b"ab", 32, 160)
    _, _, _, alphabet, own, _ = CASES[NAMES.index(name)]
    while True:
        out = rng.strings(alphabet, 256, 48)
        if b"" in out:
            return list(own) + out


def digest(strings):
    return hashlib.sha1(b"".join(struct.pack("<I", len(s)) + s for s in strings)).hexdigest()


def ask(cases):
    """[(name, pattern, index, strings)] -> [{states, letters, start, results}], blobs left in a directory that is returned"""
    tmp = tempfile.mkdtemp(prefix="slow_capture_")
    req = os.path.join(tmp, "request.txt")
    with open(req, "w") as f:
        for name, pattern, index, strings in cases:
            f.write("case %s %d %s\n" % (name, index, pattern.hex()))
            for s in strings:
                f.write("s %s\n" % s.hex())
            f.write("end\n")
    r = subprocess.run([BIN, "gen", req, tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    out, cur = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = {"name": w[1], "states": int(w[2]), "letters": int(w[3]), "start": int(w[4]), "results": []}
        elif w[0] == "r":
            cur["results"].append([int(x) for x in w[1:]])
        elif w[0] == "end":
            out.append(cur)
    assert [c["name"] for c in out] == [c[0] for c in cases]
    return out, tmp


def generate():
    """{file name: bytes} of everything under tests/golden/slow_capture"""
    # the gaps at which the longest state list is exactly 64 and 65 entries long: found by asking
    probes = [("probe%d" % g, wide_pattern(g), 1, [b"a" * (2 * g + 10) + b"b"]) for g in range(48, 64)]
    answers, probe_tmp = ask(probes)
    shutil.rmtree(probe_tmp)
    live = {int(p[0][5:]): a["results"][0][4] for p, a in zip(probes, answers)}
    gaps = dict(WIDE, wide64=min(g for g, v in live.items() if v == 64), wide65=min(g for g, v in live.items() if v == 65))
    requests = [(name, pattern, index, case_strings(name)) for name, pattern, index, _, _, _ in CASES]
    requests += [(name, wide_pattern(gaps[name]), 1, case_strings(name, gaps[name])) for name in WIDE]
    always = {c[0]: c[5] for c in CASES}
    answers, tmp = ask(requests)
    files, cases, rows = {}, [], []
    for (name, pattern, index, strings), a in zip(requests, answers):
        captured = sum(r[0] for r in a["results"])
        if always.get(name) == "never":
            assert captured == 0 and any(r[3] and not r[0] for r in a["results"]), "%s: nothing matches without capturing" % name
        else:
            assert captured > 0, "%s: no string captures" % name
            assert always.get(name) or captured < len(strings), "%s: every string captures" % name
        with open(os.path.join(tmp, name + ".blob"), "rb") as f:
            files[name + ".blob"] = f.read()
        cases.append({"name": name, "pattern_hex": pattern.hex(), "index": index, "always": always.get(name, False), "blob": name + ".blob",
                      "states": a["states"], "letters": a["letters"], "start": a["start"], "gap": gaps.get(name), "first": len(rows),
                      "strings": len(strings), "sha1": digest(strings)})
        rows += a["results"]
    shutil.rmtree(tmp)
    flat = [v for r in rows for v in r]
    assert all(-1 <= v < 2 ** 15 for v in flat)
    files["expected.i16"] = struct.pack("<%dh" % len(flat), *flat)
    doc = {"generator": "tests/golden/make_slow_capture_inputs.py", "seed": SEED, "expected": "expected.i16",
           "row": ["captured", "begin", "end", "matched", "live"]}
    body = ",\n".join(json.dumps(c) for c in cases)
    files["cases.json"] = (json.dumps(doc)[:-1] + ', "cases": [\n' + body + "\n]}\n").encode()
    return files


def main():
    if not os.path.exists(BIN):
        sys.exit("build %s first: make -C tests/cpp slow_capture_golden" % BIN)
    os.makedirs(OUT, exist_ok=True)
    for name, data in sorted(generate().items()):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        print("%8d  %s" % (len(data), name))


if __name__ == "__main__":
    main()
