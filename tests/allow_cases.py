"""The two allow automata and the reference of the allow filter inside the document-frequency pass (include/tgx_allow.h):
tests/test_allow_cpu.py holds the host twin to it, tests/test_allow_gpu.py the device.  The texts, geometries and the brute
force are those of tests/generate_cases.py; the filter is a plain walk of the automaton's next / tag arrays."""
from __future__ import annotations

import functools
import os

import numpy as np

import generate_cases as gc
from tokengeex_amd import _lib, compile_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (A) at most 16 states: 16-wide tables; runs that stay live to 32 bytes, arms that die on the first byte, multi-byte arms
SMALL = "[ab]+|c[a-d]*| ?(?:é)+|中|𝒳[a-d]"  # (the group: a repeat binds to one BYTE of the compiler's syntax)
# (B) the reference's allow regex (tests/golden/exact.regex) in byte syntax, arm by arm; the operators' arm is the file's own
ARMS = [
    rb"[\x00-\x09\x0b-\x7f]|[\xc2-\xdf][\x80-\xbf]|[\xe0-\xef][\x80-\xbf][\x80-\xbf]|[\xf0-\xf4][\x80-\xbf][\x80-\xbf][\x80-\xbf]",
    rb"[a-z]+|[A-Z]+|[A-Z][a-z]+",
    rb"'(?:re|ve|s|d|ll|t|m)",
    rb"(?:\xe3[\x90-\xbf][\x80-\xbf]|\xe4[\x80-\xb6][\x80-\xbf]|\xe4[\xb8-\xbf][\x80-\xbf]|[\xe5-\xe9][\x80-\xbf][\x80-\xbf])+",
    rb"[ ]+|[\t]+",
    None,
    rb" ?[!-/:-@\[-`{-~] ?",
]


@functools.lru_cache(maxsize=None)
def exact_source() -> bytes:
    with open(os.path.join(ROOT, "tests", "golden", "exact.regex"), "rb") as f:
        operators = f.read().strip().split(b"$|^")[7]  # "(?: ?(?:(?:\+)|...) ?)"
    return b"|".join(b"(?:" + (operators if arm is None else arm) + b")" for arm in ARMS)


@functools.lru_cache(maxsize=None)
def automaton(which: str):
    return compile_pattern([SMALL if which == "A" else exact_source()], search=False, max_states=64)


@functools.lru_cache(maxsize=None)
def chunk_cases():
    """What the 256-position geometries do not pin of the kernels' chunks of 64: a 200-byte part of long [a-d] runs at
    offsets 33 and 63, so that 32-byte windows cross one and two chunk edges, with a two-byte character on bytes 63 / 64;
    and texts of 65 and 127 bytes, whose last chunk has nothing behind it."""
    run = (b"c" + b"abdc" * 10)[:40]
    cases = []
    for lead in (33, 63):
        t = bytearray(b"#" * lead + run * 5 + b"#" * 40)
        t[63:65] = gc.E2
        cases.append(dict(name=f"part_at_{lead}", text=bytes(t), parts=[(lead, lead + 200, 2)], origin=None))
    for n in (65, 127):
        cases.append(dict(name=f"text_of_{n}", text=(run * 4)[:n], parts=[(0, n, 0)], origin=None))
    return tuple(cases)


def allows(pat, data: bytes) -> bool:
    q = pat.start
    for b in data:
        q = int(pat.next[b][q])
    return bool(pat.tag[q])


@functools.lru_cache(maxsize=None)
def _reference(text: bytes, parts, origin, which: str, mtl: int, prob: float, seed: int):
    pat = automaton(which)
    mask = np.zeros(len(text), np.uint32)
    for k, (b, e, s) in enumerate(parts):
        o = b if origin is None else origin[k]
        for p in range(b, e):
            if not gc.is_start(text, p):
                continue
            q = pat.start
            for ln in range(1, min(mtl, e - p) + 1):
                q = int(pat.next[text[p + ln - 1]][q])
                if pat.tag[q] and (p + ln == e or gc.is_start(text, p + ln)) and (prob >= 1.0 or _lib.generate_u01(seed, s, ((p - o) << 8) | ln) < prob):
                    mask[p] |= np.uint32(1 << (ln - 1))
    df, _ = gc.brute_force(text, list(parts), origin, mtl, prob, seed)
    return mask, {sub: d for sub, d in df.items() if allows(pat, sub)}, sum(bin(int(m)).count("1") for m in mask)


def reference(c, which: str, mtl: int, prob: float = 1.0, seed: int = 0):
    """-> (mask uint32[N]: bit l - 1 of mask[p] set iff window (p, l) is kept, {allowed substring: samples}, kept windows)"""
    return _reference(c["text"], tuple(c["parts"]), None if c["origin"] is None else tuple(c["origin"]), which, mtl, prob, seed)
