"""Texts, part geometries and the brute-force reference for the raw interface of the document-frequency pass
(tgx_substring_df[_top], csrc/generate.hip): tests/test_generate_cases_cpu.py shows that each case sits on the edge it is
named for and pins the brute force, tests/test_generate_parts_gpu.py runs the same cases on the device.  Nothing here
calls a kernel; the keep rule's draw is the host function that include/tgx.h specifies (tgx_generate_u01).

A case: name, text (bytes), parts [(begin, end, sample)] sorted and disjoint with ascending sample ids, origin (per part:
where its sample begins in the text; None: the part is its own sample).  The device works in blocks of 256 positions and
finds a block's first part through a table made on the host, which is what the geometries are about."""
from __future__ import annotations

import functools

import numpy as np

from tokengeex_amd import _lib

BLOCK = 256
MTLS = (1, 4, 5, 7, 32)
MAX_SAMPLE = (1 << 27) - 1
E2, E3, E4 = "é".encode(), "中".encode(), "𝒳".encode()
assert (len(E2), len(E3), len(E4)) == (2, 3, 4)


def is_start(text: bytes, p: int) -> bool:
    return (text[p] & 0xC0) != 0x80


def brute_force(text: bytes, parts, origin, mtl: int, prob: float = 1.0, seed: int = 0):
    """-> ({substring: number of samples whose set holds it}, number of kept windows).  For every part (b, e, s): every
    character start p in [b, e), every length up to mtl with p + length <= e that ends on a character boundary or at e;
    with prob < 1 the window is kept iff tgx_generate_u01(seed, s, (p - origin) << 8 | length) < prob."""
    sets: dict = {}
    n_windows = 0
    for k, (b, e, s) in enumerate(parts):
        o = b if origin is None else origin[k]
        mine = sets.setdefault(s, set())
        for p in range(b, e):
            if not is_start(text, p):
                continue
            for ln in range(1, mtl + 1):
                if p + ln > e:
                    break
                if p + ln < e and not is_start(text, p + ln):
                    continue
                if prob < 1.0 and not _lib.generate_u01(seed, s, ((p - o) << 8) | ln) < prob:
                    continue
                mine.add(text[p:p + ln])
                n_windows += 1
    df: dict = {}
    for held in sets.values():
        for sub in held:
            df[sub] = df.get(sub, 0) + 1
    return df, n_windows


def make_text(n: int, seed: int) -> bytes:
    """n bytes over a small alphabet (substrings repeat) with 2-, 3- and 4-byte characters; cut at n, maybe inside one."""
    rng = np.random.default_rng(seed)
    chars = ["a", "b", "c", " ", "é", "中", "𝒳"]
    draw = rng.choice(len(chars), size=n, p=[0.3, 0.25, 0.15, 0.12, 0.08, 0.06, 0.04])
    return "".join(chars[i] for i in draw).encode()[:n]


def ascii_text(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"abcd ", np.uint8)[rng.integers(0, 5, size=n)])


def _utf8_case():
    """2-, 3- and 4-byte characters straddling the block boundaries at 256, 512 and 768; characters that end exactly at
    mtl = 4, 5, 7 and 32 bytes from a window's start; parts that end inside a character of every width."""
    t = bytearray(ascii_text(1024, 3))
    t[255:257] = E2          # bytes 255, 256
    t[510:513] = E3          # 510 .. 512
    t[766:770] = E4          # 766 .. 769
    t[20:24] = b"ab" + E2                                   # "abé": 4 bytes
    t[30:35] = b"ab" + E3                                   # "ab中": 5
    t[40:47] = b"abc" + E4                                  # "abc𝒳": 7
    t[100:132] = b"abcdabcdabcdabcdabcdabcdabcd" + E4       # 28 + 4 = 32
    t[140:172] = b"abcdabcdabcdabcdabcdabcdabcdab" + E2     # 30 + 2
    t[180:212] = b"abcdabcdabcdabcdabcdabcdabcda" + E3      # 29 + 3
    t[600:602], t[610:613], t[620:624] = E2, E3, E4         # cut by the ends of the parts below
    text = bytes(t)
    parts = [(0, 300, 0), (400, 560, 1), (590, 601, 2), (604, 611, 3), (614, 622, 4), (700, 800, 5)]
    return dict(name="utf8", text=text, parts=parts, origin=None)


@functools.lru_cache(maxsize=None)
def geometry_cases():
    cases = []
    t = make_text(1024, 1)
    cases.append(dict(name="on_block_boundaries", text=t, parts=[(0, 256, 0), (256, 512, 1), (512, 768, 1), (768, 1024, 5)], origin=None))
    cases.append(dict(name="one_part_over_three_blocks", text=t, parts=[(100, 700, 0)], origin=None))
    t = ascii_text(600, 2)
    cases.append(dict(name="300_one_byte_parts", text=t, parts=[(40 + i, 41 + i, i // 3) for i in range(300)], origin=None))
    t = make_text(2048, 4)
    cases.append(dict(name="gaps", text=t, parts=[(10, 60, 0), (650, 650, 0), (700, 760, 1), (1500, 1530, 5), (2040, 2048, 6)],
                      origin=None))  # (with an empty part between two others)
    for n in (512, 513, 511):
        t = make_text(n, 5 + n)
        cases.append(dict(name=f"last_part_ends_at_{n}", text=t, parts=[(0, 100, 0), (n - 70, n, 1)], origin=None))
    t = bytearray(ascii_text(700, 6))
    t[300:304] = E4
    t[10:13] = E3
    cases.append(dict(name="no_position_inside_a_part", text=bytes(t), parts=[(5, 5, 0), (11, 13, 1), (256, 256, 1), (301, 304, 2), (699, 699, 3)],
                      origin=None))
    text = b"abcabc----abcabc----abcabc----" + b"x" * 300 + b"abcabc"
    cases.append(dict(name="once_per_sample", text=text, parts=[(0, 6, 3), (10, 16, 3), (20, 26, 4), (330, 336, 4)], origin=None))
    t = make_text(900, 7)
    cases.append(dict(name="sample_ids", text=t, parts=[(0, 200, 0), (250, 500, 5), (500, 520, 5), (600, 900, MAX_SAMPLE)], origin=None))
    cases.append(_utf8_case())
    return tuple(cases)


def case(name: str):
    return next(c for c in geometry_cases() if c["name"] == name)


GEOMETRY_NAMES = ("on_block_boundaries", "one_part_over_three_blocks", "300_one_byte_parts", "gaps", "last_part_ends_at_512",
                  "last_part_ends_at_513", "last_part_ends_at_511", "no_position_inside_a_part", "once_per_sample", "sample_ids", "utf8")


# ---- placement: the same samples at other offsets of the buffer, and in two calls -----------------------------------------
PLACE_PROB, PLACE_SEED, PLACE_MTL = 0.3, 5, 8
PLACE_IDS = (7, 8, 11, 12, 40, 41)


@functools.lru_cache(maxsize=None)
def placement_samples():
    """Six samples of 150 .. 700 bytes, each with the parts a split pattern would give: the runs between spaces."""
    out = []
    for i, n in enumerate((150, 256, 257, 700, 333, 512)):
        text = make_text(n, 20 + i)
        parts, b = [], None
        for p in range(n + 1):
            inside = p < n and text[p] != 0x20
            if inside and b is None:
                b = p
            if not inside and b is not None:
                parts.append((b, p))
                b = None
        out.append((text, tuple(parts)))
    return tuple(out)


def place(which, lead: int, gap: int, filler: bytes = b"#"):
    """The samples `which` (indices into placement_samples) packed with `lead` filler bytes before the first and `gap`
    between two -> a case with origins; sample ids PLACE_IDS[i]."""
    buf, parts, origin = bytearray(filler * lead), [], []
    for i in which:
        text, rel = placement_samples()[i]
        at = len(buf)
        buf += text
        parts += [(at + b, at + e, PLACE_IDS[i]) for b, e in rel]
        origin += [at] * len(rel)
        buf += filler * gap
    return dict(name=f"placed+{lead}/{gap}", text=bytes(buf), parts=parts, origin=origin)


def arrays(c):
    """-> (flat, part_begin, part_end, part_sample, part_origin or None) for _lib.substring_df"""
    flat = np.frombuffer(c["text"], np.uint8)
    pb = np.array([p[0] for p in c["parts"]], np.uint64)
    pe = np.array([p[1] for p in c["parts"]], np.uint64)
    ps = np.array([p[2] for p in c["parts"]], np.uint32)
    po = None if c["origin"] is None else np.array(c["origin"], np.uint64)
    return flat, pb, pe, ps, po


def top_expectation(df: dict, k: int):
    """-> (the k largest frequencies in descending order, cutoff_df: the (k + 1)-th largest, or 0 when nothing is cut)"""
    d = sorted(df.values(), reverse=True)
    return d[:k], (d[k] if k < len(d) else 0)


def top_ks(df: dict) -> dict:
    """kind -> k: 1, a k with equal frequencies on both sides of the cut, n_distinct - 1, n_distinct, n_distinct + 1"""
    d = sorted(df.values(), reverse=True)
    n = len(d)
    tied = [k for k in range(2, n) if d[k - 1] == d[k] and d[k - 1] > d[-1]] or [k for k in range(1, n) if d[k - 1] == d[k]]
    ks = {"1": 1, "n-1": n - 1, "n": n, "n+1": n + 1}
    if tied:
        ks["tie"] = tied[0]
    return {kind: k for kind, k in ks.items() if k >= 1}
