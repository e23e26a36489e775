"""The text statistics and the line view without a device: the host twins (tgx_text_stats_host, tgx_lines_host; they walk
the kernels' chunks, tiles, summaries, carry and store / add rule through csrc/textstat.h) against the independent
checker (tests/textstat_checker.py) and Python's own strings on the batches of tests/textstat_cases.py, and the batches
against the geometry they claim.  Everything is compared exactly: this is integer work."""
import functools

import numpy as np
import pytest

from tokengeex_amd import _lib

import textstat_cases
import textstat_checker as tc
from textstat_cases import CAP, CHUNK, LIMITS, RUN, TILE

ALL = textstat_cases.NAMES + ("past_cap",)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = textstat_cases.past_cap_case() if name == "past_cap" else textstat_cases.case(name)
    for a in (c["text"], c["offs"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(name, limit, unit):
    stats, marks = tc.stats_of(_case(name)["text"], _case(name)["offs"], limit, unit)
    stats.setflags(write=False)
    marks.setflags(write=False)
    return stats, marks


@pytest.mark.parametrize("unit", tc.UNITS)
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("name", ALL)
def test_twin_matches_checker(name, limit, unit):
    c = _case(name)
    want, want_marks = _want(name, limit, unit)
    stats, marks = _lib.text_stats_host(c["text"], c["offs"], limit, unit)
    for k, stat in enumerate(tc.NAMES):
        assert np.array_equal(stats[k], want[k]), stat
    assert np.array_equal(marks, want_marks)


@pytest.mark.parametrize("name", ALL)
def test_twin_matches_pythons_strings(name):
    c = _case(name)
    stats, _ = _lib.text_stats_host(c["text"], c["offs"], 5, "char")
    d = dict(zip(tc.NAMES, stats))
    n_valid = 0
    for i, raw in enumerate(tc.rows_of(c["text"], c["offs"])):
        truth = tc.second_truth(raw)
        if truth is None:
            continue
        n_valid += 1
        n_chars, lens = truth
        assert (d["chars"][i], d["lines"][i], d["max_line"][i], d["long_lines"][i]) == (n_chars, len(lens), max(lens, default=0), sum(n > 5 for n in lens)), i
    assert n_valid >= 1


@pytest.mark.parametrize("name", ALL)
def test_lines_twin_matches_checker(name):
    c = _case(name)
    want_offs, line_row = tc.lines_of(c["text"], c["offs"])
    assert np.array_equal(_lib.lines_host(c["text"], c["offs"]), want_offs)
    lines = _want(name, 0, "byte")[0][tc.NAMES.index("lines")]
    assert np.array_equal(line_row, np.repeat(np.arange(lines.size), lines))


def test_no_rows_and_no_bytes():
    none, empty = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    stats, marks = _lib.text_stats_host(none, empty, 5, "char")
    assert stats.shape == (tc.N, 0) and marks.size == 0
    assert _lib.lines_host(none, empty).tolist() == [0]
    stats, marks = _lib.text_stats_host(none, np.zeros(4, np.uint64), 5, "byte")
    assert stats.shape == (tc.N, 3) and not stats.any(), "a corpus of empty rows: every statistic is written, as 0"
    assert _lib.lines_host(none, np.zeros(4, np.uint64)).tolist() == [0]


# ---- the batches hold the geometry they claim -----------------------------------------------------------------------------

def _newlines(c):
    return set(np.flatnonzero(c["text"] == 10).tolist())


def test_cases_hold_their_geometry():
    rows = _case("short_rows")["rows"]
    assert {b"", b"\n", b"\n\n", b"a", b"a\n"} <= set(rows) and {len(r) for r in rows} >= {0, 1, 2, 3}
    nl = _newlines(_case("nl_at_chunk_edges"))
    assert {CHUNK - 1, CHUNK} <= nl and 2 * CHUNK - 1 in nl and 2 * CHUNK not in nl and 3 * CHUNK in nl and 3 * CHUNK - 1 not in nl
    assert {TILE - 1, TILE} <= nl
    c = _case("limit_lines")
    for unit in tc.UNITS:
        lens = {tc._units(p, unit) for raw in c["rows"] for p in tc.pieces_of(raw)}
        assert {0, 1, 5, 6} <= lens, "a line of exactly each limit and of one more, in this unit"
    for name, edge in textstat_cases.EDGES.items():
        c = _case(name)
        ends = c["offs"][1:].astype(np.int64)
        assert {-3, -2, -1, 0, 1, 2, 3} <= {int((e + 3) % edge) - 3 for e in ends}, name
        line_offs, _ = tc.lines_of(c["text"], c["offs"])
        a, z = line_offs[:-1].astype(np.int64), line_offs[1:].astype(np.int64) - 1
        assert (a // edge != z // edge).sum() >= 7, "a line lies astride an edge in every round"
        lens = np.diff(c["offs"].astype(np.int64))
        assert any(lens[i] == 0 for i in range(len(lens)))
    c = _case("row_end_at_chunk_edge")
    offs = c["offs"].astype(np.int64)
    at_edge = [i for i in range(len(c["rows"]) - 1) if offs[i + 1] % CHUNK == 0 and not c["rows"][i].endswith(b"\n")]
    assert len(at_edge) >= 2
    for i in at_edge:
        assert len(tc.pieces_of(c["rows"][i])[-1]) > CHUNK and len(tc.pieces_of(c["rows"][i + 1])[0]) > 2 * CHUNK, "a long line on either side"
    lens = [len(r) for r in _case("empty_rows")["rows"]]
    assert lens[:3] == [0, 0, 0] and lens[-2:] == [0, 0] and sum(lens[i] == lens[i + 1] == 0 for i in range(len(lens) - 1)) >= 5
    offs = _case("empty_rows")["offs"].astype(np.int64)
    assert any(lens[i] == 0 and offs[i] % CHUNK == 0 and offs[i] > 0 for i in range(len(lens))) and any(lens[i] == 0 and offs[i] % TILE == 0 and offs[i] > 0 for i in range(len(lens)))
    rows = _case("long_line")["rows"]
    assert any(len(r) == 5 * TILE and b"\n" not in r for r in rows) and any(len(r) == 5 * TILE and r.find(b"\n") == 5 * TILE - 1 for r in rows)
    assert any(len(r) > CHUNK and set(r) == {10} for r in _case("only_newlines")["rows"])
    c = _case("chars_across_chunks")
    leads = {int(c["text"][p]) >> 4 for p in range(CHUNK - 1, c["text"].size, CHUNK) if c["text"][p] >= 0xC0 and (c["text"][p + 1] & 0xC0) == 0x80}
    assert {0xC, 0xE, 0xF} <= leads, "a two-, a three- and a four-byte character with its lead byte on a chunk's last lane"
    rows = _case("stray_continuations")["rows"]
    assert any((r[0] & 0xC0) == 0x80 for r in rows) and any(b"\n\x80" in r for r in rows)
    assert any(sorted(r) == list(range(256)) for r in _case("byte_classes")["rows"])
    for name in textstat_cases.NAMES:
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
    line_offs, line_row = tc.lines_of(c["text"], c["offs"])
    lines = {(int(a), int(z)): int(r) for a, z, r in zip(line_offs[:-1], line_offs[1:], line_row)}
    a, z = c["where"]["inside"]
    assert lines[(a, z + 1)] == c["where"]["row"] and a // RUN == z // RUN and a // TILE + 1 == z // TILE, "a line from a run's first tile into its second"
    a, z = c["where"]["straddle"]
    assert lines[(a, z + 1)] == c["where"]["row"] and a // RUN + 1 == z // RUN, "a line from one block's run into the next"
    a, z = offs[c["where"]["row"]], offs[c["where"]["row"] + 1] - 1
    assert a // RUN + 1 == z // RUN and a // TILE + 2 <= z // TILE, "one row over both"
    lens = np.diff(offs)
    assert {0, 1, 2, 3} <= set(lens.tolist()) and lens[:3].tolist() == [0, 0, 0] and lens[-2:].tolist() == [0, 0]


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_twins_refuse_bad_arguments():
    lib = _lib.lib
    d = np.asarray([97, 10, 98], np.uint8)
    good, bad0, bad1 = (np.asarray(x, np.uint64) for x in ([0, 1, 3], [1, 2, 3], [0, 3, 2]))
    stats, marks = np.full((tc.N, 2), 9, np.int64), np.full(3, 9, np.uint8)
    out_offs, nl = np.full(5, 9, np.uint64), _lib.C.c_uint64(77)
    p = _lib.ptr
    for offs in (bad0, bad1):
        assert lib.tgx_text_stats_host(p(d), p(offs), 2, 5, 0, p(stats), p(marks)) == _lib.ERR_INVALID
        assert lib.tgx_lines_host(p(d), p(offs), 2, p(out_offs), 4, _lib.C.byref(nl)) == _lib.ERR_INVALID
    assert lib.tgx_text_stats_host(None, p(good), 2, 5, 0, p(stats), p(marks)) == _lib.ERR_INVALID
    assert lib.tgx_text_stats_host(p(d), p(good), 2, 5, 2, p(stats), p(marks)) == _lib.ERR_INVALID, "an unknown flag"
    assert lib.tgx_text_stats_host(p(d), p(good), 2, 5, 0, None, None) == _lib.ERR_INVALID
    assert lib.tgx_lines_host(p(d), p(good), 2, p(out_offs), 4, None) == _lib.ERR_INVALID
    assert lib.tgx_lines_host(p(d), p(good), 2, p(out_offs), 3, _lib.C.byref(nl)) == _lib.ERR_INVALID and nl.value == 3, "too little room: n_lines says how much"
    assert lib.tgx_lines_host(p(d), p(good), 2, None, 4, _lib.C.byref(nl)) == _lib.ERR_INVALID
    assert (stats == 9).all() and (marks == 9).all() and (out_offs == 9).all(), "a refused call writes nothing"
    assert lib.tgx_text_stats_host(p(d), p(good), 2, 5, 1, p(stats), None) == 0 and stats[tc.NAMES.index("lines")].tolist() == [1, 2]   # either may be NULL
    assert lib.tgx_text_stats_host(p(d), p(good), 2, 5, 1, None, p(marks)) == 0 and marks.tolist() == [1, 1, 1]
    assert lib.tgx_lines_host(p(d), p(good), 2, p(out_offs), 4, _lib.C.byref(nl)) == 0 and out_offs.tolist() == [0, 1, 2, 3, 9]
    with pytest.raises(ValueError):
        _lib.text_stats_host(d, good, 5, "word")
