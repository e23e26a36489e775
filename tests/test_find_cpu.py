"""Leftmost-first matches and the mine without a device: the compiler's find=True and the host twins (tgx_find_host,
tgx_mine_host: the kernels' walks, doubling rounds, maps, fold, scan and order rule through csrc/find.h) against Python's
re on the batch of tests/find_cases.py, the truncation contract, the refusals and the header's table.  Everything is
integer work and compared exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from find_cases import CHUNK, FLAT, MINE_RS_SAMPLES, OFFS, PATTERNS, ROWS, SEG, SPACES, mined, pattern, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_batch_holds_what_it_is_for():
    words, std, plus = want(r" ?[A-Za-z]+")[1], want(r"std::\w+")[1], want(r"\+|\+\+|\+=")
    assert words[3 * CHUNK - 6] == 6 and words[3 * CHUNK] == 6 and std[SEG - 11] == 11 and words[SEG + 5 * CHUNK + 63] == 64
    assert want(r"a|ab|abc+")[1][2 * SEG - 20:2 * SEG + 20].tolist() == [1] * 40 and plus[1][3 * SEG - 31:3 * SEG + 29].tolist() == [1, 0] * 30, "first beats longest"
    assert want(r"\s+")[0][SPACES] == 79 and len(ROWS[0]) == 0 and len(ROWS[1]) == 1 and int(OFFS[42]) < CHUNK and FLAT.size % CHUNK and FLAT.size <= 300 << 10


@pytest.mark.parametrize("src", PATTERNS)
def test_twins_equal_re(src):
    want_count, want_lens, want_truncated, want_top = want(src)
    count, lens, truncated = _lib.find_host(FLAT, OFFS, pattern(src))
    assert np.array_equal(truncated, want_truncated) and np.array_equal(count, want_count) and np.array_equal(lens, want_lens)
    for top in (1, 3, len(want_top) + 5):
        got, n_distinct, n_matches = mined(FLAT, _lib.mine_host(FLAT, OFFS, pattern(src), top))
        assert got == want_top[:top] and n_distinct == len(want_top) and n_matches == want_count.sum(), top


def test_the_reference_miners_own_example():
    flat, offs = tgx.pack(MINE_RS_SAMPLES)
    assert mined(flat, _lib.mine_host(flat, offs, pattern(r"std::\w+"), 2))[0] == [(b"std::string", 3), (b"std::vector", 2)]
    assert pattern(r"(?:std|abc)::\w+").n_states == pattern(r"(std|abc)::\w+").n_states


@pytest.mark.parametrize("row,max_len,want_lens,want_truncated", [(b"a" * 150, 64, [64, 64, 22], 2), (b"aaaaaaab", 5, [5, 2], 1)])
def test_truncation_contract(row, max_len, want_lens, want_truncated):
    flat, offs = tgx.pack([b"b", row])
    count, lens, truncated = _lib.find_host(flat, offs, pattern("a+"), max_len)
    assert lens[lens != 0].tolist() == want_lens and count.tolist() == [0, len(want_lens)] and truncated.tolist() == [0, want_truncated]


def test_refusals():
    flat, offs = tgx.pack([b"ab+", b""])
    count, lens, truncated = np.full(2, -7, np.int64), np.full(3, 7, np.uint8), np.full(2, -7, np.int64)
    good, empty = _lib.dfa64_struct(pattern("a+")), _lib.dfa64_struct(pattern("a+"))
    empty.tag[empty.start] = 1

    def find(d, max_len, outs=(count, lens, truncated)):
        return _lib.lib.tgx_find_host(_lib.ptr(flat), _lib.ptr(offs), 2, ctypes.byref(d), max_len, *(None if o is None else _lib.ptr(o) for o in outs))

    assert find(good, 0) == find(good, 65) == find(empty, 64) == find(good, 64, (None, None, None)) == _lib.ERR_INVALID
    assert (count == -7).all() and (lens == 7).all() and (truncated == -7).all() and find(good, 64) == _lib.OK
    with pytest.raises(tgx.TokenGeeXError, match="top is 0"):
        _lib.mine_host(flat, offs, pattern("a+"), 0)
    with pytest.raises(ValueError, match="empty string"):
        tgx.compile_pattern("a*", find=True)
    with pytest.raises(ValueError, match="72 states"):
        tgx.compile_pattern("a{70}", find=True)
    for mixed in (dict(cover=True), dict(search=True), dict(search=False)):
        with pytest.raises(ValueError, match="find=True"):
            tgx.compile_pattern("ab", find=True, **mixed)


def test_header_and_symbol_table_agree():
    """every function the header declares is in FIND_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_find.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS") and name != "FIND_SYMBOLS"]
    assert declared == set(_lib.FIND_SYMBOLS) and not any(declared & set(t) for t in others) and all(hasattr(_lib.lib, name) for name in declared)
