"""The batch and the plain reference of test_find_cpu.py and test_find_gpu.py.  The reference is Python's re on bytes:
re.finditer per row, and a Counter of the matched bytes ordered by (-count, first position).  The one row that holds
matches longer than max_len = 64 (SPACES under \\s+) has its expected spans written out."""
import collections
import functools
import re

import numpy as np

import tokengeex_amd as tgx

# (the first two: leftmost-first and leftmost-longest differ)
PATTERNS = [r"\+|\+\+|\+=", r"a|ab|abc+", r" ?[A-Za-z]+", r"[0-9]{1,3}(\.[0-9])?", r"'(re|ve|s|d|ll|t|m)", r"\n[ ]+|\n[\t]+", r"std::\w+", r"\s+"]
MINE_RS_SAMPLES = [b"std::string", b"std::vector", b"std::vector<std::string>", b"std::map<int, std::string>"]

CHUNK, SEG = 64, 4096
MIXED = b"std::vector<int> v; a++ += it's we'll 12.5 192.168.0.1 abccc ab a\n    x+=1\n\t\tstd::string s = \"they've\";\n"


def _build():
    """-> (rows, the index of SPACES).  `#` matches no pattern and pads a row's start to where an edge must fall."""
    rows, at = [], 0

    def add(row):
        nonlocal at
        rows.append(row)
        at += len(row)

    def pad_to(pos):  # a filler row that ends at global byte `pos`
        add(b"#" * (pos - at))

    add(b"")                                    # rows of length 0 and 1
    add(b"a")
    for k in range(40):                         # forty rows inside chunk 0
        add([b"a", b"+", b"ab", b"7", b"", b"'s"][k % 6])
    assert at < CHUNK
    pad_to(3 * CHUNK - 7)
    add(b"# hello world+=")                     # " hello" ends on the last byte of chunk 2, " world" begins chunk 3
    pad_to(SEG - 13)
    add(b"# std::vector<int>")                  # "std::vector" ends on the last byte of segment 0
    pad_to(SEG + 5 * CHUNK + 62)
    add(b"#" + b"Q" * 64)                       # a 64-byte match from byte 63 of a chunk to its row's end: skip 63 into the next chunk
    pad_to(2 * SEG - 40)
    add(b"+" * 20 + b"a" * 40 + b"+=" * 10)     # matches back to back across the boundary of segments 1 and 2
    pad_to(3 * SEG - 31)
    add(b"+=" * 30 + b" 1.5")
    add((MIXED * 700)[:70_001])                 # longer than the 64 KiB of a block's four waves
    spaces = len(rows)
    add(b" " * 5000)                            # one long match source: under \s+ it is cut into 78 matches of 64 and one of 8
    k = 0
    while at < 280_000:                         # ordinary rows at odd cuts
        add((MIXED * 40)[k % 101:k % 101 + 37 + (k * 131) % 3001])
        k += 1
    add(b"it's std::map")                       # the last row ends mid-chunk
    assert at % CHUNK
    return rows, spaces


ROWS, SPACES = _build()
FLAT, OFFS = tgx.pack(ROWS)


@functools.lru_cache(maxsize=None)
def pattern(src):
    return tgx.compile_pattern(src, find=True)


def spans_of(src, rows, spaces=None):
    out = [[m.span() for m in re.finditer(src.encode(), row)] for row in rows]
    if spaces is not None and src == r"\s+":
        out[spaces] = [(64 * k, 64 * k + 64) for k in range(78)] + [(4992, 5000)]
    return out


@functools.lru_cache(maxsize=None)
def want(src):
    """of the batch under `src` -> (count int64[S], lens uint8[N], truncated int64[S], [(bytes, count)] in the mine's order)"""
    spans = spans_of(src, ROWS, SPACES)
    count, lens, truncated = np.array([len(s) for s in spans], np.int64), np.zeros(FLAT.size, np.uint8), np.zeros(len(ROWS), np.int64)
    if src == r"\s+":
        truncated[SPACES] = 78
    return count, lens_of(spans, OFFS, lens), truncated, ranked(spans, ROWS)


def lens_of(spans, offs, lens):
    for i, row in enumerate(spans):
        for a, b in row:
            lens[int(offs[i]) + a] = b - a
    return lens


def ranked(spans, rows):
    seen = collections.Counter(row[a:b] for row, s in zip(rows, spans) for a, b in s)  # (a Counter keeps first-seen order)
    first = {m: k for k, m in enumerate(seen)}
    return sorted(seen.items(), key=lambda mc: (-mc[1], first[mc[0]]))


def mined(flat, res):
    """what _lib.mine_host / NativeCorpus.mine return -> ([(bytes, count)], n_distinct, n_matches)"""
    pos, length, count, n_distinct, n_matches = res
    return [(flat[int(p):int(p) + int(n)].tobytes(), int(c)) for p, n, c in zip(pos, length, count)], n_distinct, n_matches
