#!/usr/bin/env python3
"""Generate tests/golden/affix/* from the UNMODIFIED reference library (oracle/_ref/libpire_ref.so): small unsurrounded
scanners for the prefix and suffix searches, each in a forward form (option `n`: not Surround()ed) and in a form compiled from
Fsm::Reverse() (`nr`, what LongestSuffix / ShortestSuffix walk: pire_ut.cpp:283).

Run where the reference tree exists:   python tests/golden/make_affix_inputs.py
The fixtures travel with the repo; tests/test_affix.py reads them wherever it runs.

  <name>.<form>.blob   Scanner::Save() of the one pattern compiled with the form's options
  cases.json           per blob: name, form, pattern, options, file, the reference's Size() -- and what the reference's
                       LongestPrefix / ShortestPrefix (form n) or LongestSuffix / ShortestSuffix (form nr) answer on PROBES
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.binding import RefScanner, pack_strings  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "affix")

# name -> (pattern of the forward form, pattern of the reversed form)
SCANNERS = {
    "blanks": ("[ \\t]+", "[ \\t]+"),
    "blanks_star": ("[ \\t]*", "[ \\t]*"),                    # accepts the empty string: every length is >= 0
    "stamp": ("[0-9]{4}-[0-9]{2}-[0-9]{2} ", "[0-9]{4}-[0-9]{2}-[0-9]{2} "),
    "arrow": ("-->", "-->"),                                  # pire_ut.cpp:278-306
    "ext": ("\\.(gz|log|txt)", "\\.(gz|log|txt)"),
    "alt": ("abc|abcabc|b+", "abc|abcabc|b+"),                # a dead state after one byte of anything else
    "marked_blanks": ("^[ \\t]+", "[ \\t]+$"),                # match only through the begin mark (n) / the end mark (nr)
}
FORMS = ("n", "nr")
PROBES = [b"", b" ", b"  \t x \t", b"2024-01-02 x.gz", b"-->a-->", b"abcabc", b"bbb", b".log", b"xyz"]


def generate():
    """{file name: bytes} of everything under tests/golden/affix"""
    files, cases = {}, []
    text, offs = pack_strings(PROBES)
    for name, patterns in SCANNERS.items():
        for form, pattern in zip(FORMS, patterns):
            sc = RefScanner.compile([pattern], [form])
            assert sc.regexps == 1 and not sc.empty, (name, form)
            blob = sc.save()
            assert len(blob) < 8192, (name, form, len(blob))
            fname = "%s.%s.blob" % (name, form)
            files[fname] = blob
            walk = sc.prefix if form == "n" else sc.suffix
            marks = name == "marked_blanks"
            cases.append({"name": name, "form": form, "pattern": pattern, "options": form, "blob": fname, "states": int(sc.size),
                          "marks": marks,
                          "longest": [int(x) for x in walk(text, offs, True, marks, False)],
                          "shortest": [int(x) for x in walk(text, offs, False, marks, False)]})
    doc = {"generator": "tests/golden/make_affix_inputs.py", "probes_hex": [p.hex() for p in PROBES], "scanners": cases}
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
