"""Word ids (include/tgx_word_ids.h; csrc/words.h) without a device: the host twin tgx_words_host, which walks the kernels'
chunks, doubling steps, records, carry, emit rule and offsets, against the definition written out below (bytes.split(),
the polynomial in Python integers, the two mixes) on the case table that tests/test_words_gpu.py shares; tgx_word_key;
and the argument errors, with nothing written."""
import ctypes
import functools
import os

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, MASK = 0x9E3779B97F4A7C15, 2**64 - 1
FOLD = bytes(b + 32 if 65 <= b <= 90 else b for b in range(256))
SEED = 0x0123456789ABCDEF


def mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK
    return x ^ x >> 31


def ref_key(word, fold, seed):
    p = 0
    for b in word.translate(FOLD) if fold else word:
        p = (p * M + b + 1) & MASK
    return mix(p ^ mix((mix((seed + M) & MASK) + len(word)) & MASK))


def reference(rows, fold, seed):
    ids = [[ref_key(w, fold, seed) >> 33 for w in row.split()] for row in rows]
    return np.asarray([i for r in ids for i in r], np.uint32), np.cumsum([0] + [len(r) for r in ids]).astype(np.uint64)


def _word(n, salt=0):
    """n non-space bytes, every one of them different from its neighbours"""
    return bytes(33 + (7 * j + salt) % 94 for j in range(n))


with open(os.path.join(ROOT, "tests", "golden", "words_text.txt"), "rb") as f:
    TEXT = f.read()  # a fixed text: 57 611 bytes of prose and code with 2 140 distinct words
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 129, 200)
NON_SPACE = [b for b in range(256) if bytes([b]) not in b" \t\n\r\x0b\x0c"]
CASES = {  # name -> the rows
    "lengths": [b" ".join(_word(n, n) for n in LENGTHS), b"\t".join(_word(n) for n in reversed(LENGTHS))],
    # the same 70-byte word behind 0, 1, 63 and 64 bytes of another row, with no space between the two
    **{f"at{k}": [b"q" * k, _word(70), b"tail"] for k in (0, 1, 63, 64)},
    # words that end at lane 63 (the byte after them: a row's first, a space, the word's next) and begin at lane 0
    "edges": [b"x" * 60 + b" abc", b"def ghi", b"y" * 53 + b" ab", b" cd" + b"z" * 58 + b" " + _word(3) + _word(64) + b" e"],
    "rows": [b"", b"ab cd", b"ef", b"", b"", b" \t\n\r\x0b\x0c ", b"gh  ij ", b"", b"k", b""],
    "no_rows": [],
    "no_bytes": [b"", b"", b""],
    "one_byte": [b"", b"a"],
    "bytes": [b" ".join(bytes([b]) for b in NON_SPACE), b"\x00a a \x00\x00a \x00 \x00\x00", bytes(NON_SPACE), bytes(reversed(NON_SPACE)) + b"\n"],
    "fold": [b"Word word WORD wOrD @[`{ @[`{ \xc3\x89t\xc3\xa9 \xc3\xa9T\xc3\x89 AZaz az", b"Zebra" * 30 + b" zebra" * 3],
    # one word of 66 000 bytes between ordinary text: many chunks without a reset, and a scan of more than one block
    "long": [TEXT[:2000], TEXT[2000:2100] + _word(66000) + TEXT[2100:3000], TEXT[3000:4003]],
    "text": [TEXT],
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name, fold):
    """(text, offs, want_ids, want_offs): computed once, never changed"""
    text, offs = _lib.pack(CASES[name])
    out = (text, offs) + reference(CASES[name], fold, SEED)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("fold", (False, True))
@pytest.mark.parametrize("name", NAMES)
def test_twin_matches_the_definition(name, fold):
    text, offs, want_ids, want_offs = case(name, fold)
    ids, out_offs = _lib.words_host(text, offs, fold, SEED)
    assert ids.dtype == np.uint32 and np.array_equal(out_offs, want_offs) and np.array_equal(ids, want_ids)
    assert ids.size == 0 or int(ids.max()) < 2**31


def test_what_the_table_is_there_to_show():
    """the reference itself: the placements agree, 0x00 counts, the fold is A-Z's alone, the seed matters, and the 2 000
    distinct words of a fixed text have 2 000 ids"""
    at = [reference(CASES[f"at{k}"], False, SEED)[0][-2] for k in (0, 1, 63, 64)]
    assert len(set(at)) == 1 and sum(len(r) for r in CASES["long"]) > 69000
    assert len({ref_key(w, True, 0) for w in (b"\x00a", b"a", b"\x00\x00a", b"\x00", b"\x00\x00")}) == 5
    assert ref_key(b"WORD", True, 0) == ref_key(b"word", True, 0) != ref_key(b"WORD", False, 0)
    assert ref_key(b"@[\xc9", True, 0) == ref_key(b"@[\xc9", False, 0) != ref_key(b"`{\xe9", True, 0)
    distinct = set(TEXT.split())
    assert len(distinct) > 2000 and len({ref_key(w, False, SEED) >> 33 for w in distinct}) == len(distinct)
    text, offs, want_ids, _ = case("text", True)
    assert not np.array_equal(_lib.words_host(text, offs, True, SEED + 1)[0], want_ids)


def test_word_key_and_word_id():
    for word in (b"", b"a", b"\x00a", b"Hello,", _word(200), bytes(range(256))):
        for fold in (False, True):
            assert _lib.word_key(word, fold, SEED) == ref_key(word, fold, SEED) and tgx.word_id(word, fold, SEED) == ref_key(word, fold, SEED) >> 33
    assert tgx.word_id("Été") == ref_key("Été".encode(), True, 0) >> 33 and tgx.word_id("The") == tgx.word_id(b"the")
    import tokengeex
    assert tokengeex.word_id is tgx.word_id and tokengeex.word_rows is tgx.word_rows


def test_argument_errors_write_nothing():
    text, offs, want_ids, want_offs = case("rows", False)
    p, call = _lib.ptr, _lib.lib.tgx_words_host
    ids, out_offs, nw = np.full(want_ids.size, 7, np.uint32), np.full(want_offs.size, 7, np.uint64), ctypes.c_uint64(99)
    S, bad = offs.size - 1, np.asarray([0, 3, 2], np.uint64)
    for args in ((p(text), p(offs), S, 2, 0, p(ids), ids.size, p(out_offs), ctypes.byref(nw)),         # a flag that is none
                 (p(text), p(bad), 2, 0, 0, p(ids), ids.size, p(out_offs), ctypes.byref(nw)),          # offsets that descend
                 (p(text), None, S, 0, 0, p(ids), ids.size, p(out_offs), ctypes.byref(nw)),
                 (None, p(offs), S, 0, 0, p(ids), ids.size, p(out_offs), ctypes.byref(nw)),
                 (p(text), p(offs), S, 0, 0, p(ids), ids.size, None, ctypes.byref(nw)),
                 (p(text), p(offs), S, 0, 0, p(ids), ids.size, p(out_offs), None)):
        assert call(*args) == _lib.ERR_INVALID and nw.value in (0, 99), args
        nw.value = 99
    assert call(p(text), p(offs), S, 0, 0, p(ids), ids.size - 1, p(out_offs), ctypes.byref(nw)) == _lib.ERR_INVALID and nw.value == want_ids.size
    assert call(p(text), p(offs), S, 0, 0, None, ids.size, p(out_offs), ctypes.byref(nw)) == _lib.ERR_INVALID
    assert (ids == 7).all() and (out_offs == 7).all()
    assert call(p(text), p(offs), S, 0, SEED, p(ids), ids.size, p(out_offs), ctypes.byref(nw)) == 0 and np.array_equal(ids, want_ids)

