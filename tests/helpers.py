"""Shared test helpers: golden fixtures, string packing."""
import gzip
import json
import os
import subprocess

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_cache = None


def golden():
    global _cache
    if _cache is None:
        with open(os.path.join(GOLDEN, "cases.json")) as f:
            _cache = json.load(f)
    return _cache


def load_blob(rel: str) -> bytes:
    path = os.path.join(GOLDEN, rel)
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if rel.endswith(".gz") else data


def case_strings(case):
    return [bytes.fromhex(h) for h in case["strings_hex"]]


def all_cases():
    return golden()["cases"]


def big_sets():
    return golden()["big"]


def pack(strings):
    offs = np.zeros(len(strings) + 1, dtype=np.uint64)
    if strings:
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    text = np.frombuffer(b"".join(strings), dtype=np.uint8) if strings else np.zeros(0, np.uint8)
    return text, offs


def make_shim_program(name, *args):
    """`make -C tests/cpp NAME`: tests/cpp/NAME.cpp against the reference headers into oracle/_ref/bin/NAME, with the flags every
    program that includes the shim gets (tests/cpp/shim.mk); oracle/_ref/libpire_ref.so is there before.  The finished process."""
    return subprocess.run(["make", "-C", os.path.join(os.path.dirname(GOLDEN), "cpp"), name] + list(args), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=900)


def plants_for(big):
    from oracle.binding import make_plants

    return make_plants([(bytes.fromhex(h), t) for h, t in zip(big["witnesses_hex"], big["witness_at_tail"])])


def random_strings(rng, n, max_len, alphabet=None):
    out = []
    for _ in range(n):
        k = int(rng.randint(0, max_len + 1))
        if alphabet is None:
            out.append(bytes(rng.randint(0, 256, size=k, dtype=np.uint8)))
        else:
            out.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=k)))
    return out


# ---- batches laid across byte offset 2^32 of a device buffer (tests/test_past_4gib.py) -----------------------------------
FOUR_GIB = 1 << 32
ACROSS_WHERE = ("between", "chunk", "line", "empty")
ACROSS_LEAD_MODS = (0, 1, 77, 112)


def across_4gib(strings, where, lead_mod, pad):
    """(strings', lead, k, d): the batch with `pad[:r]`, r < 128, appended to its first string, and the byte offset `lead` of its
    first byte, chosen so that byte 2^32 of the buffer is byte d of string k (k near the middle of the batch) and
    lead % 128 == lead_mod.  where:
      "between"  d = 0, strings k - 1 and k not empty: 2^32 exactly between two strings;
      "chunk"    d % 16 == 8, 0 < d < len(k): inside string k, in the middle of a 16-byte chunk counted from its first byte;
      "line"     d % 128 == 0 (d % 16 == 0 where the batch has no string of more than 128 bytes), 0 < d < len(k): inside
                 string k, a whole number of 128-byte lines (16-byte chunks) behind its first byte;
      "empty"    string k is made empty and starts at 2^32 (as does the string behind it)."""
    s = [bytes(x) for x in strings]
    n, k = len(s), len(s) // 2
    assert n >= 4 and len(pad) >= 127

    def first(pred):
        for i in list(range(k, n - 1)) + list(range(k - 1, 0, -1)):
            if pred(i):
                return i
        raise AssertionError("no string for %r" % where)

    if where == "between":
        k, d = first(lambda i: len(s[i - 1]) > 0 and len(s[i]) > 0), 0
    elif where == "chunk":
        k = first(lambda i: len(s[i]) >= 10)
        d = 8 + 16 * ((len(s[k]) // 2) // 16)
        d = d if d < len(s[k]) else 8
    elif where == "line":
        step = 128 if max(len(x) for x in s[1:n - 1]) > 128 else 16
        k = first(lambda i: len(s[i]) > step)
        d = step * max(1, (len(s[k]) // 2) // step)
    elif where == "empty":
        s[k], d = b"", 0
    else:
        raise KeyError(where)
    w = sum(len(x) for x in s[:k]) + d
    r = (-lead_mod - w) % 128
    s[0] = s[0] + bytes(pad[:r])
    lead = FOUR_GIB - w - r
    assert lead % 128 == lead_mod and (d == 0 or 0 < d < len(s[k])) and 0 < k < n - 1
    return s, lead, k, d


def sides_of_4gib(strings, lead):
    """(below, above, inside): masks of the strings that start below 2^32 / at or above it, and of those that have byte 2^32
    behind their first byte (start < 2^32 < end)."""
    _, offs = pack(strings)
    b, e = offs[:-1].astype(np.int64) + lead, offs[1:].astype(np.int64) + lead
    return b < FOUR_GIB, b >= FOUR_GIB, (b < FOUR_GIB) & (e > FOUR_GIB)


def period_of_lines(plants, nbytes, seed, sep=9):
    """u8[nbytes]: lines of 1 .. 4 KiB cut from the tails of the synthetic corpus' records (where the plants put the witnesses),
    each ended by a newline, the last one too; a newline or `sep` inside a record becomes a blank, and every line gets one
    `sep` a third of the way in (two columns: the second one ends with the record's tail).  (raw, lengths)."""
    from oracle.binding import corpus_fill

    rng = np.random.RandomState(seed)
    lens, left = [], nbytes
    while left > 2 * 4097:
        lens.append(int(rng.randint(1024, 4097)))
        left -= lens[-1] + 1
    half = (left - 2) // 2
    lens += [half, left - 2 - half]
    assert sum(lens) + len(lens) == nbytes and min(lens) >= 1024 and max(lens) <= 4096
    rec = corpus_fill(seed, 0, len(lens), 4096, plants, threads=4)
    rec[(rec == 10) | (rec == sep)] = 32
    raw = np.empty(nbytes, dtype=np.uint8)
    at = 0
    for i, k in enumerate(lens):
        raw[at:at + k] = rec[i, 4096 - k:]
        raw[at + k // 3] = sep
        raw[at + k] = 10
        at += k + 1
    return raw, np.asarray(lens, dtype=np.int64)
