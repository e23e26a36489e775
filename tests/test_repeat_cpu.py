"""The repetition statistics without a device: the host twin (tgx_repeat_stats_host; it goes through csrc/repeat.h: the row
keys, a stable sort, the run rule, repeat_run_end, the kernel's chunks with the two-chunk window and the store / add
rule) against the independent checker (tests/repeat_checker.py: tuples in dicts, no hashing) on the batches of
tests/repeat_cases.py, the batches against the geometry they claim, the argument refusals, and the keep rules of
repetition_rows and line_repetition_rows.  Everything is compared exactly: this is integer work.

The torch glue of repetition_rows and line_repetition_rows needs a device for the statistics, so the rules are factored
out of it (tensors.repetition_keep over RepeatStats objects, tensors.line_dup_counts and tensors.line_dup_keep) and
tested here alone, on CPU tensors, against a plain Python evaluation of small hand-written rows; tests/test_repeat_gpu.py
tests the whole functions."""
import functools

import numpy as np
import pytest

from tokengeex_amd import _lib, tensors

import repeat_cases
import repeat_checker as rc
from gram_cases import CAP, CHUNK, RUN, TILE

SEED = 0xC0FFEE1234567890
PAST = [(kind, w) for kind in repeat_cases.KINDS for w in repeat_cases.widths(kind)]


@functools.lru_cache(maxsize=None)
def _case(name, kind, w):
    c = repeat_cases.past_cap_case(kind, w) if name == "past_cap" else repeat_cases.case(name, kind, w)
    c["want"] = rc.stats(c["data"], c["offs"], w)
    for a in (c["data"], c["offs"]) + c["want"]:
        a.setflags(write=False)
    return c


def _row(c, key):
    return c["want"][0][:, c["where"][key]].tolist()


@pytest.mark.parametrize("name,kind,w", repeat_cases.all_cases())
def test_twin_matches_checker(name, kind, w):
    c = _case(name, kind, w)
    want_stats, want_mask = c["want"]
    for seed in (0, SEED):
        assert rc.row_keys_are_distinct(c["data"], c["offs"], w, seed), "then equality by key is equality by gram"
        stats, mask = _lib.repeat_stats_host(c["data"], c["offs"], w, seed)
        assert np.array_equal(stats, want_stats) and np.array_equal(mask, want_mask), seed
    assert (want_mask[c["repeat_at"]] & 1).all(), "every planted repeat is one"
    assert not want_stats[1:3, c["clean_rows"]].any() and not want_stats[4:, c["clean_rows"]].any()


@pytest.mark.parametrize("kind,w", PAST)
def test_past_the_cap(kind, w):
    c = _case("past_cap", kind, w)
    assert rc.row_keys_are_distinct(c["data"], c["offs"], w, SEED)
    stats, mask = _lib.repeat_stats_host(c["data"], c["offs"], w, SEED)
    assert np.array_equal(stats, c["want"][0]) and np.array_equal(mask, c["want"][1])
    assert (mask[c["repeat_at"]] & 1).all()


def test_outputs_alone():
    c = _case("edges_chunk", "bytes", 5)
    lib, p = _lib.lib, _lib.ptr
    S, N = len(c["offs"]) - 1, c["data"].size
    stats, mask = np.full((6, S), -7, np.int64), np.full(N, 7, np.uint8)
    assert lib.tgx_repeat_stats_host(p(c["data"]), 1, p(c["offs"]), S, 5, 0, p(stats), None) == 0 and np.array_equal(stats, c["want"][0])
    assert lib.tgx_repeat_stats_host(p(c["data"]), 1, p(c["offs"]), S, 5, 0, None, p(mask)) == 0 and np.array_equal(mask, c["want"][1])


# ---- the batches hold the geometry they claim, and the answers that the issue states ---------------------------------------

@pytest.mark.parametrize("kind", repeat_cases.KINDS)
def test_cases_hold_their_geometry(kind):
    for w in repeat_cases.widths(kind):
        c = _case("short", kind, w)
        lens = [len(r) for r in c["rows"]]
        assert set(range(w + 3)) <= set(lens) and lens[:3] == [0, 0, 0] and lens[-2:] == [0, 0]
        assert any(lens[i] == lens[i + 1] == 0 for i in range(3, len(lens) - 3))
        c = _case("all_short", kind, w)
        assert max(len(r) for r in c["rows"]) < w and not c["want"][0].any() and not c["want"][1].any()
        c = _case("one_element", kind, w)
        for key, n in (("short", w + 1), ("long", w + 40)):
            grams = n - w + 1
            assert _row(c, key) == [grams, grams - 1, grams, grams, n - 1, n], (w, key)
        c = _case("period3", kind, w)
        n = 50 + w
        grams = n - w + 1
        assert _row(c, "row") == [grams, grams - 3, grams, (grams + 2) // 3, n - 3, n], w
        c = _case("twins", kind, w)
        assert c["rows"][1] == c["rows"][2] and c["clean_rows"].size == 4 and not c["want"][1].any(), "nothing is flagged"
        assert (c["want"][0][3, c["clean_rows"]] == 1).all()
        c = _case("lanes", kind, w)
        assert sorted(int(e) % CHUNK for e in c["repeat_at"]) == [0, CHUNK - 1]
        c = _case("reach", kind, w)
        r, edge = c["where"]["row"], c["where"]["edge"]
        assert c["repeat_at"].tolist() == [edge - (w - 1)] and edge % CHUNK == 0 and int(c["offs"][r + 1]) > edge + 1
        # the row's only repeat: the elements up to the chunk's first are covered, the one after it is not
        assert _row(c, "row")[1:] == [1, 2, 2, w, 2 * w], w
        c = _case("row_end", kind, w)
        after = c["where"]["after"]
        assert int(c["offs"][after]) - w in c["repeat_at"] and _row(c, "after") == [4, 0, 0, 1, 0, 0]
        for name, edge in repeat_cases.EDGES.items():
            c = _case(name, kind, w)
            from_edge = {int((e + 3) % edge) - 3 for e in c["offs"][1:].astype(np.int64)}
            assert {-3, -2, -1, 0, 1, 2, 3} <= from_edge, name
            astride = [e for e in c["repeat_at"] if e // edge != (e + w - 1) // edge]
            last = [e for e in c["repeat_at"] if e + w in c["offs"]]
            assert len(last) == 7 and len(c["repeat_at"]) == 14 and (w == 1 or len(astride) >= 7), (name, w)
        c = _case("alignments", kind, w)
        assert {int(o) % 4 for o in c["offs"][:-1]} == {0, 1, 2, 3}
        c = _case("five_tiles", kind, w)
        n = 5 * TILE
        assert _row(c, "row") == [n - w + 1, n - w, n - w + 1, n - w + 1, n - 1, n]


@pytest.mark.parametrize("kind,w", PAST)
def test_past_cap_case_is_past_the_cap(kind, w):
    c = _case("past_cap", kind, w)
    offs = c["offs"].astype(np.int64)
    n = int(offs[-1])
    n_tiles = -(-n // TILE)
    assert n == CAP * TILE + 2 * TILE + 70 and n_tiles > CAP and -(-n_tiles // CAP) == 2
    table = c["want"][0]
    a, z = offs[c["where"]["inside"]], offs[c["where"]["inside"] + 1] - 1
    assert a // RUN == z // RUN and a // TILE + 1 == z // TILE and table[1, c["where"]["inside"]] > 0
    a, z = offs[c["where"]["straddle"]], offs[c["where"]["straddle"] + 1] - 1
    assert a // RUN + 1 == z // RUN, "from one block's run into the next"
    edge = (a // RUN + 1) * RUN
    flagged = np.flatnonzero(c["want"][1][a:z + 1] & 1) + a
    assert (flagged < edge).any() and (flagged >= edge).any(), "both blocks add to the row's sums"
    assert table[1, c["where"]["long"]] >= 4 and len(c["repeat_at"]) >= 6


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_twin_refuses_bad_arguments():
    lib, p = _lib.lib, _lib.ptr
    d = np.asarray([1, 2, 3], np.uint8)
    good, bad0, bad1 = (np.asarray(x, np.uint64) for x in ([0, 1, 3], [1, 2, 3], [0, 3, 2]))
    stats, mask = np.full((6, 2), 9, np.int64), np.full(3, 9, np.uint8)
    for offs, eb, w in ((bad0, 1, 2), (bad1, 1, 2), (good, 3, 2), (good, 1, 0), (good, 1, 65), (good, 4, 17)):
        assert lib.tgx_repeat_stats_host(p(d), eb, p(offs), 2, w, 0, p(stats), p(mask)) == _lib.ERR_INVALID, (eb, w)
    assert lib.tgx_repeat_stats_host(p(d), 1, p(good), 2, 2, 0, None, None) == _lib.ERR_INVALID
    assert lib.tgx_repeat_stats_host(None, 1, p(good), 2, 2, 0, p(stats), p(mask)) == _lib.ERR_INVALID
    assert lib.tgx_repeat_stats_host(p(d), 1, None, 2, 2, 0, p(stats), p(mask)) == _lib.ERR_INVALID
    assert (stats == 9).all() and (mask == 9).all(), "a refused call writes nothing"
    assert lib.tgx_repeat_stats_host(p(d), 1, p(good), 0, 2, 0, p(stats), p(mask)) == 0 and (stats == 9).all(), "no row: nothing is written"
    assert lib.tgx_repeat_stats_host(p(d), 1, p(good), 2, 2, 0, p(stats), p(mask)) == 0
    assert stats.tolist() == [[0, 1], [0, 0], [0, 0], [0, 1], [0, 0], [0, 0]] and mask.tolist() == [0, 0, 0]
    for w, eb in ((0, 1), (65, 1), (17, 4), (-1, 4)):
        with pytest.raises(ValueError):
            _lib.repeat_check_width(w, eb)
    assert _lib.repeat_check_width(64, 1) == 64 and _lib.repeat_check_width(16, 4) == 16
    names = (_lib.C.c_char_p * 8)()
    ms = (_lib.C.c_float * 8)()
    assert lib.tgx_repeat_last_times(names, ms, 8) == 4
    assert [names[k].decode() for k in range(4)] == ["repeat_keys_kernel", "repeat_sort", "repeat_runs_kernel", "repeat_cover_kernel"]


# ---- the keep rules on CPU tensors -----------------------------------------------------------------------------------------

ROWS = [[], [1], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [1, 2] * 10, [3] * 30, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14],
        [1, 2, 3, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20], list(range(1, 41)) + [5, 6, 7, 8, 9], [4, 4, 5, 6, 7, 8, 9, 10, 11, 12]]


def _stats_on_cpu(data, offs, widths):
    import torch
    elems = torch.from_numpy(np.diff(offs.astype(np.int64)))
    return {w: tensors.RepeatStats(torch.from_numpy(_lib.repeat_stats_host(data, offs, w)[0]), elems, w) for w in widths}


@pytest.mark.parametrize("literal", (False, True))
def test_repetition_keep_rule(literal):
    import repeat_cases as cases
    data, offs = cases.pack(ROWS, "ids")
    for top, dup in ((rc.GOPHER_TOP, rc.GOPHER_DUP), (((2, .5),), ()), ((), ((3, .25), (5, .3))), (((1, .34), (4, .0)), ((2, .0),))):
        widths = sorted({w for w, _ in top + dup})
        stats = _stats_on_cpu(data, offs, widths)
        keep = tensors.repetition_keep(stats, top, dup, literal).nonzero().reshape(-1).numpy()
        want = rc.keep_rows(data, offs, top, dup, literal)
        assert np.array_equal(keep, want), (top, dup)
        assert 0 in keep and 1 in keep and 2 in keep, "rows without a repeat are kept, the empty row among them"
    s = _stats_on_cpu(data, offs, (2,))[2]
    table = rc.stats(data, offs, 2)[0]
    tf, cf, caf = rc.fracs(table, np.diff(offs.astype(np.int64)), 2)
    assert np.array_equal(s.top_frac.numpy(), tf) and np.array_equal(s.covered_frac.numpy(), cf) and np.array_equal(s.covered_all_frac.numpy(), caf)
    assert np.array_equal(s.repeated_frac.numpy(), table[1] / np.maximum(table[0], 1))
    assert s.top_frac[3] == 1.0 and s.top_frac[2] == 0.0 and s.width == 2 and s.grams is not None


TEXTS = [b"", b"a\nb\nc\n", b"x\nx\nx\nx\n", b"same\nsame", b"same\nsame\n", b"\n\n\n", b"one line", b"k\n" + b"long line here\n" * 2 + b"k\nz\nq\nr\ns\nt\nu\n",
         b"ab\ncd\nab\nef\ngh\nij\nkl\nmn\nop\nqr\n"]


def test_line_repetition_keep_rule():
    import torch
    for max_lines, max_bytes in ((0.30, 0.20), (0.0, 0.0), (1.0, 1.0), (0.5, 0.1)):
        want_keep, want_dl, want_db, want_nl = rc.line_keep_rows(TEXTS, max_lines, max_bytes)
        # the line view, first_equal of the lines and the lines' lengths as the device calls give them, from plain Python
        lines, line_row = [], []
        for i, t in enumerate(TEXTS):
            parts = t.split(b"\n")
            mine = [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
            lines += mine
            line_row += [i] * len(mine)
        first = {}
        cls = [first.setdefault(ln, k) for k, ln in enumerate(lines)]
        as_t = lambda v: torch.tensor(v, dtype=torch.int64)
        dl, db = tensors.line_dup_counts(as_t(line_row), as_t(cls), as_t([len(ln) for ln in lines]), len(TEXTS))
        assert np.array_equal(dl.numpy(), want_dl) and np.array_equal(db.numpy(), want_db)
        keep = tensors.line_dup_keep(dl, db, as_t(want_nl.tolist()), as_t([len(t) for t in TEXTS]), max_lines, max_bytes).nonzero().reshape(-1)
        assert np.array_equal(keep.numpy(), want_keep), (max_lines, max_bytes)
        assert 0 in want_keep, "an empty row is kept"
    assert rc.line_keep_rows(TEXTS)[1].tolist() == [0, 0, 3, 0, 1, 2, 0, 2, 1]
    dl, db = tensors.line_dup_counts(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3)
    assert dl.tolist() == [0, 0, 0] and db.tolist() == [0, 0, 0]
