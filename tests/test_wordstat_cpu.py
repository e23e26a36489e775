"""The word statistics without a device: the host twin (tgx_word_stats_host; it walks the kernels' chunks, masks, summaries,
carry and store / add rule through csrc/wordstat.h) against the independent checker (tests/wordstat_checker.py) on the
batches of tests/wordstat_cases.py, the batches against the geometry they claim, the keep rule of the Gopher filters on
hand-made tables, the refusals, and who declares the new calls.  Everything is compared exactly: this is integer work."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dirty_runs
import wordstat_cases
import wordstat_checker as ck
from wordstat_cases import CAP, CHUNK, COMBOS, RUN, TILE, table_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = wordstat_cases.NAMES + ("past_cap",)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = wordstat_cases.past_cap_case() if name == "past_cap" else wordstat_cases.case(name)
    for a in (c["text"], c["offs"]):
        a.setflags(write=False)
    return c


@pytest.mark.parametrize("name", ALL)
def test_twin_matches_checker(name):
    c = _case(name)
    for limit, unit, fold, with_table in COMBOS:
        stops = table_for(fold, with_table)
        want, want_marks = ck.stats_of(c["text"], c["offs"], limit, stops, unit, fold)
        stats, marks = _lib.word_stats_host(c["text"], c["offs"], limit, stops, unit, fold)
        for k, stat in enumerate(ck.NAMES):
            assert np.array_equal(stats[k], want[k]), (stat, limit, unit, fold, with_table)
        assert np.array_equal(marks, want_marks), (limit, unit, fold, with_table)


def test_no_rows_and_no_bytes():
    none, empty = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    stats, marks = _lib.word_stats_host(none, empty)
    assert stats.shape == (ck.N, 0) and marks.size == 0
    stats, marks = _lib.word_stats_host(none, np.zeros(4, np.uint64), 5, (), "byte", False)
    assert stats.shape == (ck.N, 3) and not stats.any(), "a corpus of empty rows: every statistic is written, as 0"


# ---- the batches hold the geometry they claim -----------------------------------------------------------------------------

def _marks(name, fold=True, with_table=True):
    c = _case(name)
    return ck.stats_of(c["text"], c["offs"], 5, table_for(fold, with_table), "char", fold)[1]


def _stat(name, stat, limit=5, unit="char", fold=True, with_table=True):
    c = _case(name)
    return ck.stats_of(c["text"], c["offs"], limit, table_for(fold, with_table), unit, fold)[0][ck.NAMES.index(stat)]


def test_cases_hold_their_geometry():
    rows = _case("short_rows")["rows"]
    assert {b"", b" ", b"a", b"a a", b"\n\n", b" a "} <= set(rows) and {len(r) for r in rows} >= {0, 1, 2, 3}
    assert any(len(r) > CHUNK and not r.split() for r in rows), "a row of spaces only, longer than a chunk"
    assert sum(rows[i] == rows[i + 1] == b"" for i in range(len(rows) - 1)) >= 4
    assert any(sorted(r) == list(range(256)) for r in _case("byte_classes")["rows"])
    m, c = _marks("word_at_chunk_edges"), _case("word_at_chunk_edges")
    ends, starts = set(np.flatnonzero(m & ck.MARK_END).tolist()), set(np.flatnonzero(m & ck.MARK_START).tolist())
    edges = range(CHUNK, c["text"].size, CHUNK)
    assert any(e - 1 in ends and e not in starts for e in edges), "an end on a chunk's last lane alone"
    assert any(e in starts and e - 1 not in ends for e in edges), "a start on a chunk's first lane alone"
    assert any(e - 1 in ends and e in starts for e in edges), "both: a row ends there"
    rows = _case("long_words")["rows"]
    assert sum(max(len(w) for w in r.split()) == 5 * TILE for r in rows) == 3
    assert _stat("long_words", "alpha_words").tolist() == [1, 0, 1] and _stat("long_words", "alpha_wide_words").tolist() == [1, 1, 1]
    c = _case("limit_words")
    for unit in ck.UNITS:
        lens = {ck._units(w, unit) for raw in c["rows"] for w in raw.split()}
        assert {1, 5, 6} <= lens, "a word of exactly each limit and of one more, in this unit"
    leads = {int(c["text"][p]) >> 4 for p in range(CHUNK - 1, c["text"].size - 1, CHUNK) if c["text"][p] >= 0xC0 and (c["text"][p + 1] & 0xC0) == 0x80}
    assert {0xC, 0xE, 0xF} <= leads, "a two-, a three- and a four-byte character with its lead byte on a chunk's last lane"
    for name, edge in wordstat_cases.EDGES.items():
        c = _case(name)
        ends = c["offs"][1:].astype(np.int64)
        assert {-3, -2, -1, 0, 1, 2, 3} <= {int((e + 3) % edge) - 3 for e in ends}, name
        m = _marks(name)
        a, z = np.flatnonzero(m & ck.MARK_START), np.flatnonzero(m & ck.MARK_END)
        assert a.size == z.size and (a // edge != z // edge).sum() >= 7, "a word lies astride an edge in every round"
    rows = _case("rows_without_space")["rows"]
    assert any(rows[i] and rows[i + 1] and not rows[i][-1:].isspace() and not rows[i + 1][:1].isspace() for i in range(len(rows) - 1))
    offs = _case("rows_without_space")["offs"].astype(np.int64)
    assert any(o % CHUNK == 0 and o > 0 for o in offs[1:-1])
    c = _case("stop_words")
    assert (_stat("stop_words", "stop_words") != _stat("stop_words", "stop_words", fold=False)).any(), "The / THE count only under the fold"
    long_row = max(range(len(c["rows"])), key=lambda i: len(c["rows"][i]))
    of_bit = 1 << table_for(True, True).index(b"of")
    assert _stat("stop_words", "stop_words")[long_row] == 4 and _stat("stop_words", "stop_mask")[long_row] & of_bit and len(c["rows"][long_row]) > 3 * CHUNK
    stops = np.flatnonzero(_marks("stop_words") & ck.MARK_STOP)
    assert any(p % CHUNK in (0, 1) for p in stops) and any(p % CHUNK == 2 for p in stops), "matches whose bytes straddle a chunk"
    bullets = np.flatnonzero(_marks("bullets") & ck.MARK_BULLET)
    assert any(p % CHUNK == 0 for p in bullets) and any(p % CHUNK == 1 for p in bullets), "a bullet first in its chunk, U+2022 cut 1 | 2 and 2 | 1"
    assert _stat("bullets", "bullet_lines").sum() == bullets.size >= 10
    c = _case("ellipses")
    assert _stat("ellipses", "ellipsis").sum() >= 20 and _stat("ellipses", "ellipsis_lines").sum() >= 8 and _stat("ellipses", "punct_lines").sum() >= 6
    for name in wordstat_cases.NAMES:
        assert _case(name)["text"].size <= 16384, name


def test_past_cap_case_is_past_the_cap():
    c = _case("past_cap")
    offs = c["offs"].astype(np.int64)
    n = int(offs[-1])
    assert n == CAP * TILE + 2 * TILE + 70 == c["text"].size
    n_tiles = -(-n // TILE)
    per_block = -(-n_tiles // min(n_tiles, CAP))
    assert n_tiles > CAP and per_block == 2 and RUN == per_block * TILE
    assert n_tiles % per_block == 1 and n - (n_tiles - 1) * TILE == CHUNK + 6, "the last working block has one tile of two chunks, one short"
    raw = c["text"].tobytes()
    for kind in ("word", "indent"):
        row = c["where"][kind + "_row"]
        a, z = offs[row], offs[row + 1] - 1
        assert a // RUN + 1 == z // RUN and a // TILE + 2 <= z // TILE, "one row over both"
        (a, z), (a2, z2) = c["where"][kind + "_inside"], c["where"][kind + "_straddle"]
        assert offs[row] < a and z2 + 3 < offs[row + 1]
        assert a // RUN == z // RUN and a // TILE + 1 == z // TILE, "from a run's first tile into its second"
        assert a2 // RUN + 1 == z2 // RUN, "from one block's run into the next"
        for lo, hi in ((a, z), (a2, z2)):
            if kind == "word":
                assert len(raw[lo:hi + 1].split()) == 1 and raw[lo - 1:lo] == b" " and raw[hi + 1:hi + 2] == b" "
            else:
                assert raw[lo - 1:lo] == b"\n" and not raw[lo:hi + 1].strip() and raw[hi + 1:hi + 2] == b"-"
    lens = np.diff(offs)
    assert {0, 1, 2, 3} <= set(lens.tolist()) and lens[:3].tolist() == [0, 0, 0] and lens[-2:].tolist() == [0, 0]


# ---- the keep rule ------------------------------------------------------------------------------------------------------------

BASE = dict(words=100, word_units=500, max_word=9, long_words=0, alpha_words=100, alpha_wide_words=100, hash=0, ellipsis=0, lines=10, bullet_lines=0,
            ellipsis_lines=0, punct_lines=5, stop_words=7, stop_mask=0b11)
ON_THRESHOLD = [dict(words=50, word_units=250, alpha_words=50, alpha_wide_words=50), dict(words=100_000, word_units=500_000, alpha_words=100_000, alpha_wide_words=100_000),
                dict(word_units=300), dict(word_units=1000), dict(hash=10), dict(ellipsis=10), dict(bullet_lines=9), dict(ellipsis_lines=3), dict(alpha_wide_words=80),
                dict(stop_mask=0b101000), dict(stop_mask=1 << 62 | 1)]
DROPPED = [dict(words=49, word_units=245, alpha_words=49, alpha_wide_words=49), dict(words=100_001, word_units=500_005, alpha_words=100_001, alpha_wide_words=100_001),
           dict(word_units=299), dict(word_units=1001), dict(hash=11), dict(ellipsis=11), dict(bullet_lines=10), dict(ellipsis_lines=4), dict(alpha_wide_words=79),
           dict(stop_mask=0b100), dict(stop_mask=0), {name: 0 for name in ck.NAMES}]


def _table(rows):
    return np.asarray([[dict(BASE, **row)[name] for row in rows] for name in ck.NAMES], np.int64)


def test_keep_rule_on_hand_made_tables():
    import torch
    rows = [{}] + ON_THRESHOLD + DROPPED
    table = _table(rows)
    keep = tgx.gopher_quality_keep(torch.from_numpy(table))
    assert keep.dtype == torch.bool and keep.tolist() == [True] * (1 + len(ON_THRESHOLD)) + [False] * len(DROPPED)
    assert np.array_equal(ck.keep_of(table), np.arange(1 + len(ON_THRESHOLD)))
    # each rule alone drops its row: without that rule the row is kept
    relax = [dict(min_words=0), dict(max_words=10 ** 9), dict(mean_word=(0, 10)), dict(mean_word=(3, 100)), dict(max_symbol_ratio=1.0), dict(max_symbol_ratio=1.0),
             dict(max_bullet_lines=1.0), dict(max_ellipsis_lines=1.0), dict(min_alpha_words=0.0), dict(min_stop_words=1), dict(min_stop_words=0)]
    first = 1 + len(ON_THRESHOLD)
    for k, rule in enumerate(relax):
        got = tgx.gopher_quality_keep(torch.from_numpy(table), **rule).tolist()
        assert got[first + k] and got[:first] == [True] * first, rule
    # the letter test: ASCII alone where the non-ASCII bytes are not credited
    t = _table([dict(alpha_words=79, alpha_wide_words=100)])
    assert tgx.gopher_quality_keep(torch.from_numpy(t)).tolist() == [True] and tgx.gopher_quality_keep(torch.from_numpy(t), wide_is_alpha=False).tolist() == [False]
    assert tgx.gopher_quality_keep(torch.from_numpy(_table([]))).shape == (0,)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_twin_refuses_bad_arguments():
    lib = _lib.lib
    d = np.asarray([97, 32, 98], np.uint8)
    good, bad0, bad1 = (np.asarray(x, np.uint64) for x in ([0, 1, 3], [1, 2, 3], [0, 3, 2]))
    stats, marks = np.full((ck.N, 2), 9, np.int64), np.full(3, 9, np.uint8)
    p = _lib.ptr
    call = lib.tgx_word_stats_host
    for offs in (bad0, bad1):
        assert call(p(d), p(offs), 2, 5, None, None, 0, 0, p(stats), p(marks)) == _lib.ERR_INVALID
    assert call(None, p(good), 2, 5, None, None, 0, 0, p(stats), p(marks)) == _lib.ERR_INVALID
    assert call(p(d), p(good), 2, 5, None, None, 0, 4, p(stats), p(marks)) == _lib.ERR_INVALID, "an unknown flag"
    assert call(p(d), p(good), 2, 5, None, None, 0, 0, None, None) == _lib.ERR_INVALID
    many = [bytes([97 + k % 26, 97 + k // 26]) for k in range(64)]
    for bad, flags in (([b""], 0), ([b"the", b""], 0), ([b"ninebytes"], 0), ([b"a b"], 0), ([b"a\n"], 0), ([b"the", b"of", b"the"], 0), ([b"The"], 2), ([b"the", b"oF"], 3),
                       (many, 0)):
        flat, offs = _lib.pack(bad)
        assert call(p(d), p(good), 2, 5, p(flat) if flat.size else None, p(offs), len(bad), flags, p(stats), p(marks)) == _lib.ERR_INVALID, bad
        assert "tgx_word_stats_host" in lib.tgx_last_error().decode()
    flat, offs = _lib.pack([b"a"])
    assert call(p(d), p(good), 2, 5, p(flat), None, 1, 0, p(stats), p(marks)) == _lib.ERR_INVALID, "a table without offsets"
    assert (stats == 9).all() and (marks == 9).all(), "a refused call writes nothing"
    flat, offs = _lib.pack(many[:63] + [b"x"])   # 64 entries are refused, 63 are not
    assert call(p(d), p(good), 2, 5, p(flat), p(offs), 63, 3, p(stats), None) == 0 and stats[0].tolist() == [1, 1]   # either may be NULL
    flat, offs = _lib.pack([b"The", b"a"])
    assert call(p(d), p(good), 2, 5, p(flat), p(offs), 2, 1, None, p(marks)) == 0 and marks.tolist() == [1 | 2 | 4, 0, 1 | 2], "A-Z is allowed where nothing is folded"
    with pytest.raises(ValueError):
        _lib.word_stats_host(d, good, 5, (), "word")
    with pytest.raises(tgx.TokenGeeXError):
        _lib.word_stats_host(d, good, 5, ("The",))


# ---- who declares what ----------------------------------------------------------------------------------------------------------

def _functions(path):
    with open(os.path.join(ROOT, "include", path), encoding="utf-8") as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return text, set(re.findall(r"\b(tgx_[a-z0-9_]+)\s*\(", text))


def test_the_two_headers_and_the_two_tables_agree():
    words_text, words = _functions("tgx_words.h")
    _, core = _functions("tgx.h")
    assert words == set(_lib.WORD_SYMBOLS) == {"tgx_corpus_word_stats_device", "tgx_word_stats_host", "tgx_wordstat_last_times"}
    assert not words & core and not words & set(_lib.SYMBOLS), "the new calls live in the header of their own and in the second table"
    assert '#include "tgx.h"' in words_text
    with open(os.path.join(ROOT, "include", "tgx.h"), encoding="utf-8") as f:
        core_text = f.read()
    assert "word_stats" not in core_text and "wordstat" not in core_text
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in words:
        assert getattr(so, name) is not None and getattr(_lib.lib, name).argtypes == _lib.WORD_SYMBOLS[name][1]
    assert so.tgx_abi_version() == 1
    for macro, value in (("TGX_WORDSTAT_N", _lib.WORDSTAT_N), ("TGX_WORDSTAT_CHARS", _lib.WORDSTAT_CHARS), ("TGX_WORDSTAT_FOLD", _lib.WORDSTAT_FOLD)):
        assert int(re.search(rf"#define {macro} (\d+)", words_text).group(1)) == value, macro
    assert len(_lib.WORDSTAT_NAMES) == _lib.WORDSTAT_N == ck.N and _lib.WORDSTAT_NAMES == ck.NAMES and _lib.GOPHER_STOP_WORDS == ck.GOPHER
    # the registry of the pool-fill runs is tgx.h's: the new device call is put through the fills by tests/test_wordstat_gpu.py
    assert not words & (set(dirty_runs.EXCLUDED) | {fn for e in dirty_runs.ENTRIES.values() for fn in e.covers})
    names = (ctypes.c_char_p * 8)()
    ms = (ctypes.c_float * 8)()
    assert _lib.lib.tgx_wordstat_last_times(names, ms, 8) == 3
    assert [names[i].decode() for i in range(3)] == ["wordstat_summary_kernel", "wordstat_scan", "wordstat_kernel"], "the names are listed without a call"
    import tokengeex
    for name in ("word_stats", "WordStats", "gopher_quality_keep", "gopher_quality_rows", "GOPHER_STOP_WORDS"):
        assert getattr(tokengeex, name) is getattr(tgx, name) and name in tgx.__all__ and name in tokengeex.__all__
