"""Byte patterns without a device: the host twin (tgx_dfa_hits_host: the kernels' maps, chunks, doubling steps, records,
carry and store / add rule through csrc/dfa.h) against the header's definition restated in ten lines, the pattern
compiler (tokengeex_amd/patterns.py) against Python's re on the small cases, and the refusals.  The case table below is
the GPU test's too (tests/test_patterns_gpu.py).  Everything is integer work and compared exactly."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EMAIL = r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}"
# name -> (patterns, the states the minimal search automaton must have)
PATTERNS = {
    "never": ([r"[^\x00-\xff]"], 1), "ab": (["ab"], 3), "a+b": (["a+b"], 3), "email": ([EMAIL], 7), "dotted": ([r"\d+\.\d+\.\d+\.\d+"], 8),
    "abcdefgh": (["abcdefgh"], 9), "a{15}": (["a{15}"], 16), "ab|b": (["ab", "b"], 4), "high_low": ([r"[\x80-\xff][\x00-\x1f]"], 3),
}
PHONE_17 = r"\+\d{2} \d{3} \d{3} \d{4}"


def _place(n, at, fill=b"x"):
    """n filler bytes with the strings of `at` written at their positions"""
    out = bytearray(fill * n)
    for pos, s in at.items():
        out[pos:pos + len(s)] = s
    return bytes(out)


def _cut(text, lengths):
    cuts = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert cuts[-1] == len(text)
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


def _mixed(n, seed):
    """n bytes in which every pattern of the table occurs, in rows of 0 to 90 bytes around one of 300"""
    rng = np.random.default_rng(seed)
    words = [b"bob@mail.example.org", b"10.0.12.255", b"abcdefgh", b"a" * 17, b"ab", b"aab", b" ", b"\n", b"x.y@", b"1.2.3", b"@a.bc", b"abcdefg"]
    text = b"".join(words[int(k)] for k in rng.integers(0, len(words), n))[:n]
    lengths = rng.integers(0, 91, n).tolist()
    lengths.insert(5, 300)
    keep = int(np.searchsorted(np.cumsum(lengths), n))
    lengths = lengths[:keep] + [n - sum(lengths[:keep])]
    return _cut(text, lengths)


EDGES = _place(600, {62: b"ab", 63 + 64: b"ab", 255: b"ab", 598: b"ab"})  # ends on lane 63; lane 63 -> lane 0; tile edge; the last byte of a short chunk
TWO_TILES = 2048 * 256 + 2 * 256 + 70  # past the grid's cap of 2048 blocks of one 256-byte tile: a block takes two tiles
# name -> the rows
TEXTS = {
    "edges": lambda: _cut(EDGES, [1, 190, 409]),                     # rows that begin on lanes 0, 1 and 63
    "row_cut": lambda: [b"a", b"b", b"ab", b"", b"a", b"ab", b"b"],  # "a" then "b" is no match
    "empties": lambda: [b"", b"", b"ab", b"", b"", b"", b"b", b"a", b"xab", b""],
    "no_rows": lambda: [],
    "no_bytes": lambda: [b"", b"", b""],
    "long_row": lambda: [b"a" * 66_000 + b"b"],
    "all_bytes": lambda: [bytes([0, 10, 255]) + bytes(range(256)) + bytes([0, 10, 255])],
    "both_tags": lambda: [b"xabb", b"b", b"ab"],
    "mixed": lambda: _mixed(1500, 1),
    "two_tiles": lambda: [b""] + _mixed(200_000, 2) + [(b"a" * 40 + b"b") * 1707] + _mixed(TWO_TILES - 200_000 - 41 * 1707, 3) + [b""],
}
# (pattern, text): the whole table
CASES = [("ab", "edges"), ("ab", "row_cut"), ("ab", "empties"), ("ab", "no_rows"), ("email", "no_bytes"), ("a+b", "long_row"), ("a{15}", "long_row"),
         ("high_low", "all_bytes"), ("email", "all_bytes"), ("ab|b", "both_tags"), ("never", "mixed"), ("email", "mixed"), ("dotted", "mixed"),
         ("abcdefgh", "mixed"), ("a{15}", "mixed"), ("a+b", "mixed"), ("email", "two_tiles"), ("a{15}", "two_tiles")]
SMALL = [c for c in CASES if c[1] in ("edges", "row_cut", "empties", "both_tags", "all_bytes")]  # rows the quadratic check of re can take
CASE_IDS = [f"{p}-{t}" for p, t in CASES]


@functools.lru_cache(maxsize=None)
def pattern(name):
    pat = tgx.compile_pattern(PATTERNS[name][0])
    assert pat.n_states == PATTERNS[name][1], (name, pat.n_states)
    return pat


@functools.lru_cache(maxsize=None)
def text(name):
    flat, offs = tgx.pack(TEXTS[name]())
    for a in (flat, offs):
        a.setflags(write=False)
    return flat, offs


def reference(pat, flat, offs):
    """include/tgx_patterns.h's definition: per row q = start, then q = next[b][q] byte by byte"""
    nxt, tag, data = pat.next.tolist(), pat.tag.tolist(), flat.tolist()
    count, ends = np.zeros(len(offs) - 1, np.int64), np.zeros(len(data), np.uint8)
    for i in range(len(offs) - 1):
        q = pat.start
        for p in range(int(offs[i]), int(offs[i + 1])):
            q = nxt[data[p]][q]
            ends[p] = tag[q]
            count[i] += tag[q] != 0
    return count, ends


@functools.lru_cache(maxsize=None)
def want(case):
    """a case's answers by the reference: computed once, never changed"""
    out = reference(pattern(case[0]), *text(case[1]))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_twin_equals_the_reference(case):
    flat, offs = text(case[1])
    count, ends = _lib.dfa_hits_host(flat, offs, pattern(case[0]))
    assert np.array_equal(count, want(case)[0]) and np.array_equal(ends, want(case)[1])


def test_the_table_holds_what_it_is_for():
    assert text("two_tiles")[0].size == TWO_TILES and want(("a{15}", "long_row"))[0].tolist() == [66_000 - 14]
    assert want(("ab", "edges"))[0].tolist() == [0, 2, 2] and want(("ab", "row_cut"))[0].tolist() == [0, 0, 1, 0, 0, 1, 0]
    assert want(("ab|b", "both_tags"))[1].tolist() == [0, 0, 3, 2, 2, 0, 3] and want(("high_low", "all_bytes"))[0].tolist() == [2]
    assert all(want((p, "mixed"))[0].any() for p in ("email", "dotted", "abcdefgh", "a{15}", "a+b")) and not want(("never", "mixed"))[0].any()
    assert pattern("a{15}").next.max() == 15, "state and nibble 15 are in use"


@pytest.mark.parametrize("case", SMALL, ids=[f"{p}-{t}" for p, t in SMALL])
def test_compiler_against_re(case):
    """bit k at end j iff some s <= j has re.fullmatch(pattern k, row[s : j + 1])"""
    flat, offs = text(case[1])
    regs = [re.compile(p.encode()) for p in PATTERNS[case[0]][0]]
    for i in range(len(offs) - 1):
        row = bytes(flat[int(offs[i]):int(offs[i + 1])])
        got = want(case)[1][int(offs[i]):int(offs[i + 1])].tolist()
        for j in range(len(row)):
            bits = sum(1 << k for k, r in enumerate(regs) if any(r.fullmatch(row, s, j + 1) for s in range(j + 1)))
            assert got[j] == bits, (case, i, j)


def test_compiler_folds_refuses_and_counts():
    folded = tgx.compile_pattern("ab[c-d]", fold_case=True)
    assert reference(folded, *tgx.pack([b"xAbD", b"aBc", b"abe"]))[0].tolist() == [1, 1, 0]
    whole = tgx.compile_pattern("ab", search=False)  # the pattern itself from a row's first byte, with a dead state
    assert reference(whole, *tgx.pack([b"ab", b"xab", b"abab"]))[0].tolist() == [1, 0, 1]
    for bad, name in (("^a", "anchor"), ("a$", "anchor"), (r"a\b", "anchor"), (r"(a)\1", "backreference"), ("(?=a)b", "look-around"), ("(?<!a)b", "look-around"),
                      ("a+?", "lazy"), (r"\p{L}", "Unicode"), ("[é]", "non-ASCII"), ("a*", "empty string")):
        with pytest.raises(ValueError, match=name):
            tgx.compile_pattern(bad)
    with pytest.raises(ValueError, match="17 states"):
        tgx.compile_pattern(PHONE_17)
    for over in (r"[0-9a-f]{32}", r"AKIA[0-9A-Z]{16}"):
        with pytest.raises(ValueError, match="states"):
            tgx.compile_pattern(over)


def test_bad_automata_are_refused_with_nothing_written():
    flat, offs = text("row_cut")
    good = pattern("ab")
    count, ends = np.full(len(offs) - 1, -7, np.int64), np.full(flat.size, 7, np.uint8)

    def call(d, c=count, e=ends):
        return _lib.lib.tgx_dfa_hits_host(_lib.ptr(flat), _lib.ptr(offs), len(offs) - 1, ctypes.byref(d) if d else None, _lib.ptr(c) if c is not None else None,
                                          _lib.ptr(e) if e is not None else None)

    def broken(**fields):
        d = _lib.dfa_struct(good)
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    bad_next, bad_tag = broken(), broken()
    bad_next.next[200][2] = 3
    bad_tag.tag[good.start] = 1
    for d in (broken(n_states=0), broken(n_states=17), broken(start=3), bad_next, bad_tag, None):
        assert call(d) == _lib.ERR_INVALID and "tgx_dfa_hits_host" in _lib.lib.tgx_last_error().decode()
    assert call(broken(), None, None) == _lib.ERR_INVALID
    assert (count == -7).all() and (ends == 7).all()
    spare = broken()
    spare.next[200][5] = 99  # an entry at or above n_states is ignored
    assert call(spare) == _lib.OK and np.array_equal(count, want(("ab", "row_cut"))[0])


def test_header_and_symbol_table_agree():
    """every function the header declares is in PATTERN_SYMBOLS and exported, and none of them is in tgx.h's table"""
    with open(os.path.join(ROOT, "include", "tgx_patterns.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    assert declared == set(_lib.PATTERN_SYMBOLS) and not declared & set(_lib.SYMBOLS)
    assert ctypes.sizeof(_lib.TgxDfa) == 8 + 256 * 16 + 16
    import tokengeex
    assert all(getattr(tokengeex, n) is getattr(tgx, n) for n in ("compile_pattern", "BytePattern", "pattern_hits", "pattern_rows"))
