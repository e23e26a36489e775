"""Cover and redaction without a device (include/tgx_redact.h): the host twins (tgx_dfa_cover_host, tgx_redact_host: the
kernels' arithmetic through csrc/cover.h, csrc/dfa.h and csrc/redact.h) against the header's definitions restated in
plain Python, compile_pattern(cover=True) against re.fullmatch of every substring on the small cases, and the refusals.
The case tables below are the GPU test's too (tests/test_cover_gpu.py).  Everything is integer work and compared exactly."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from test_patterns_cpu import EMAIL, ROOT, TEXTS, TWO_TILES, _cut

SSN = r"\d{3}-\d{2}-\d{4}"
# name -> (patterns, the forward / backward states: all four pairs of map widths, 8 or 16 nibbles a side)
PATTERNS = {"ab": (["ab"], (3, 2)), "a+b": (["a+b"], (3, 2)), "ab+c|c": (["ab+c|c"], (4, 3)), "email": ([EMAIL], (7, 10)),
            "abcdefgh": (["abcdefgh"], (9, 8)), "ssn+digits": ([SSN, r"\d{5,}"], (14, 11)), "a{15}": (["a{15}"], (16, 15))}
COVER_TEXTS = dict(TEXTS)
COVER_TEXTS.update({
    "row_ends": lambda: _cut(b"ab" * 150, [1, 62, 1, 65, 171]),   # rows whose last byte sits on lanes 0, 62, 63 and 0 again
    "xbbc": lambda: [b"xbbc", b"abbc", b"c"],                       # only the c of xbbc: a backward pass alone would take the b's
    "overlap": lambda: [b"id 123-45-67890 and 1234, 99999-"],       # "6789" lies inside an SSN and inside a digit run
    "long_row_no_b": lambda: [b"a" * 66_000],
})
CASES = [("ab", "edges"), ("email", "edges"), ("ab", "row_ends"), ("ab", "row_cut"), ("ab+c|c", "xbbc"), ("ssn+digits", "overlap"), ("ab", "empties"),
         ("ab", "no_rows"), ("email", "no_bytes"), ("a+b", "long_row"), ("a+b", "long_row_no_b"), ("a{15}", "long_row"), ("ab+c|c", "mixed"),
         ("email", "mixed"), ("abcdefgh", "mixed"), ("ssn+digits", "mixed"), ("email", "two_tiles"), ("a{15}", "two_tiles")]
SMALL = [c for c in CASES if c[1] in ("edges", "row_ends", "row_cut", "xbbc", "overlap", "empties")]
CASE_IDS = [f"{p}-{t}" for p, t in CASES]


@functools.lru_cache(maxsize=None)
def pattern(name):
    pat = tgx.compile_pattern(PATTERNS[name][0], cover=True)
    assert (pat.n_states, pat.back.n_states) == PATTERNS[name][1], (name, pat.n_states, pat.back.n_states)
    return pat


@functools.lru_cache(maxsize=None)
def text(name):
    flat, offs = tgx.pack(COVER_TEXTS[name]())
    for a in (flat, offs):
        a.setflags(write=False)
    return flat, offs


def reference(pat, flat, offs):
    """include/tgx_redact.h's definition: f left to right, g right to left, mask = cover[f_j][g_j]"""
    nxt, back, pair, data = pat.next.tolist(), pat.back.next.tolist(), pat.cover.tolist(), flat.tolist()
    covered, mask = np.zeros(len(offs) - 1, np.int64), np.zeros(len(data), np.uint8)
    for i in range(len(offs) - 1):
        lo, hi = int(offs[i]), int(offs[i + 1])
        f, q = [0] * (hi - lo), pat.start
        for p in range(lo, hi):
            f[p - lo] = q = nxt[data[p]][q]
        g = pat.back.start
        for p in range(hi - 1, lo - 1, -1):
            mask[p] = pair[f[p - lo]][g]
            g = back[data[p]][g]
        covered[i] = np.count_nonzero(mask[lo:hi])
    return covered, mask


@functools.lru_cache(maxsize=None)
def want(case):
    """a case's answers by the reference: computed once, never changed"""
    out = reference(pattern(case[0]), *text(case[1]))
    for a in out:
        a.setflags(write=False)
    return out


def _runs(n, runs):
    """a mask of n zero bytes with value v over [a, b) for every (a, b, v)"""
    m = np.zeros(n, np.uint8)
    for a, b, v in runs:
        m[a:b] = v
    return m


# name -> (rows, mask, replacements)
REDACT_CASES = {
    # a run at a row's first and last byte, adjacent runs of two classes, a deleted run, 64 bytes, a class with no
    # replacement (copied), a row that becomes empty, and a run that ends a row before one of its class begins the next
    "small": lambda: ([b"abcdefgh", b"", b"hi", b"qq", b""], np.array([1, 1, 0, 2, 2, 4, 8, 1, 1, 3, 2, 2], np.uint8), [b"<0>", b"", b"Z" * 64]),
    # runs across the chunk edges 63/64 (lane 0 is no head), 127/128 (lane 0 heads another class) and the tile edge
    "edges": lambda: (_cut(bytes(range(256)) * 2 + b"tail", [100, 200, 216]), _runs(516, [(60, 70, 1), (126, 128, 1), (128, 130, 2), (250, 260, 4), (515, 516, 1)]),
                      [b"<A>", b"B", b"<<C>>"]),
    "none_covered": lambda: ([b"plain", b"", b"text"], np.zeros(9, np.uint8), [b"x"]),
    "all_covered": lambda: ([b"plain", b"", b"text"], np.full(9, 1, np.uint8), [b"x"]),
    "no_bytes": lambda: ([b"", b"", b""], np.zeros(0, np.uint8), [b"x"]),
    "no_rows": lambda: ([], np.zeros(0, np.uint8), [b"x"]),
    # every byte heads a run: the output outgrows the input, and the offsets cross thousands of summed chunks
    "two_tiles": lambda: (TEXTS["two_tiles"](), (1 << (np.arange(TWO_TILES) % 3)).astype(np.uint8), [b"<one>", b"", b"<three>"]),
}


@functools.lru_cache(maxsize=None)
def redact_case(name):
    """-> (flat, offs, mask, replacements, the new text and the new offsets by a loop that joins bytes)"""
    rows, mask, repl = REDACT_CASES[name]()
    flat, offs = tgx.pack(rows)
    out, done, new_offs, m = [], 0, [0], mask.tolist()
    for i, row in enumerate(rows):
        base, before = int(offs[i]), None
        for j in range(len(row)):
            low = m[base + j] & -m[base + j]
            cls = low.bit_length() - 1 if low and low.bit_length() - 1 < len(repl) else None
            if cls is None:
                out.append(row[j:j + 1])
            elif cls != before:
                out.append(repl[cls])
            before = cls
        new_offs.append(new_offs[-1] + sum(map(len, out[done:])))
        done = len(out)
    return flat, offs, mask, repl, np.frombuffer(b"".join(out), np.uint8), np.array(new_offs, np.uint64)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cover_twin_equals_the_reference(case):
    covered, mask = _lib.dfa_cover_host(*text(case[1]), pattern(case[0]))
    assert np.array_equal(covered, want(case)[0]) and np.array_equal(mask, want(case)[1])


def test_the_table_holds_what_it_is_for():
    assert want(("ab+c|c", "xbbc"))[1].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1] and want(("ab", "row_cut"))[0].tolist() == [0, 0, 2, 0, 0, 2, 0]
    assert bytes(want(("ssn+digits", "overlap"))[1]) == bytes([0] * 3 + [1] * 7 + [3] * 4 + [2] + [0] * 11 + [2] * 5 + [0])
    assert want(("a+b", "long_row"))[0].tolist() == [66_001] and not want(("a+b", "long_row_no_b"))[0].any()
    assert want(("ab", "edges"))[0].tolist() == [0, 4, 4] and want(("email", "two_tiles"))[0].sum() > 1000
    assert redact_case("two_tiles")[4].size > TWO_TILES and redact_case("small")[5].tolist() == [0, 72, 72, 75, 75, 75]


@pytest.mark.parametrize("case", SMALL, ids=[f"{p}-{t}" for p, t in SMALL])
def test_compiler_against_re(case):
    """bit k at byte j iff some s <= j < e has re.fullmatch(pattern k, row[s:e]); the forward tags are the match ends"""
    flat, offs = text(case[1])
    regs = [re.compile(p.encode()) for p in PATTERNS[case[0]][0]]
    ends = _lib.dfa_hits_host(flat, offs, pattern(case[0]))[1]
    assert np.array_equal(ends, _lib.dfa_hits_host(flat, offs, tgx.compile_pattern(PATTERNS[case[0]][0]))[1])
    for i in range(len(offs) - 1):
        row = bytes(flat[int(offs[i]):int(offs[i + 1])])
        bits = [0] * len(row)
        for k, r in enumerate(regs):
            for s in range(len(row)):
                for e in range(s + 1, len(row) + 1):
                    if r.fullmatch(row, s, e):
                        bits[s:e] = [b | 1 << k for b in bits[s:e]]
        assert want(case)[1][int(offs[i]):int(offs[i + 1])].tolist() == bits, (case, i)


@pytest.mark.parametrize("name", list(REDACT_CASES))
def test_redact_twin_equals_the_reference(name):
    flat, offs, mask, repl, want_text, want_offs = redact_case(name)
    got_text, got_offs = _lib.redact_host(flat, offs, mask, repl)
    assert np.array_equal(got_offs, want_offs) and np.array_equal(got_text, want_text)


def test_compiler_names_the_side_that_is_too_large():
    for bad, side in ((r"\+\d{2} \d{3} \d{3} \d{4}", "forward automaton of the cover has 17"), (r".{8}x", "backward automaton of the cover has 256")):
        with pytest.raises(ValueError, match=side):
            tgx.compile_pattern(bad, cover=True)
    plain = tgx.compile_pattern("ab+c|c")
    assert plain.n_states == 2 and not hasattr(plain, "cover"), "without cover nothing changes"


def test_bad_arguments_are_refused_with_nothing_written():
    flat, offs = text("row_cut")
    S, N = len(offs) - 1, flat.size
    covered, mask = np.full(S, -7, np.int64), np.full(N, 7, np.uint8)

    def cover(d, c=covered, m=mask):
        return _lib.lib.tgx_dfa_cover_host(_lib.ptr(flat), _lib.ptr(offs), S, ctypes.byref(d) if d else None, _lib.ptr(c) if c is not None else None,
                                           _lib.ptr(m) if m is not None else None)

    broken = [_lib.dfa_cover_struct(pattern("ab")) for _ in range(5)]
    broken[0].fwd.n_states, broken[1].bwd.n_states, broken[2].bwd.start = 17, 0, 2
    broken[3].bwd.next[200][1] = 2
    broken[4].fwd.tag[0] = 1
    for d in broken + [None]:
        assert cover(d) == _lib.ERR_INVALID and "tgx_dfa_cover_host" in _lib.lib.tgx_last_error().decode()
    assert cover(_lib.dfa_cover_struct(pattern("ab")), None, None) == _lib.ERR_INVALID
    assert (covered == -7).all() and (mask == 7).all()
    tagged = _lib.dfa_cover_struct(pattern("ab"))
    tagged.bwd.tag[0] = 1  # the backward automaton's tag is not looked at
    assert cover(tagged) == _lib.OK and np.array_equal(covered, want(("ab", "row_cut"))[0])

    out, new_offs, n = np.full(64, 7, np.uint8), np.full(S + 1, 7, np.uint64), ctypes.c_uint64(7)
    for rflat, roffs, n_repl in ((b"x", [0, 1], 0), (b"x" * 9, list(range(10)), 9), (b"x" * 65, [0, 65], 1), (b"xx", [0, 2, 1], 2), (b"xx", [1, 2], 1)):
        rflat, roffs = np.frombuffer(rflat, np.uint8), np.array(roffs, np.uint64)
        st = _lib.lib.tgx_redact_host(_lib.ptr(flat), _lib.ptr(offs), S, _lib.ptr(mask), _lib.ptr(rflat), _lib.ptr(roffs), n_repl, _lib.ptr(out), 64,
                                      _lib.ptr(new_offs), ctypes.byref(n))
        assert st == _lib.ERR_INVALID and n.value == 0 and (out == 7).all() and (new_offs == 7).all(), (n_repl, roffs)


def test_header_and_symbol_table_agree():
    """every function the header declares is in REDACT_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_redact.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    assert declared == set(_lib.REDACT_SYMBOLS) and not declared & (set(_lib.SYMBOLS) | set(_lib.PATTERN_SYMBOLS))
    assert ctypes.sizeof(_lib.TgxDfaCover) == 2 * ctypes.sizeof(_lib.TgxDfa) + 256
    import tokengeex
    assert all(getattr(tokengeex, n) is getattr(tgx, n) for n in ("pattern_cover", "redact", "redact_patterns"))
