"""Row selection and the seeded permutation without a GPU: the host twins (tgx_select_host, tgx_select_text_host, which
walk the fill kernels' tiles and thread slots through csrc/select.h, and tgx_shuffled_rows_host) against the independent
restatement in tests/select_checker.py.  Everything is compared exactly: this is integer data movement."""
import ctypes as C

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import select_cases
import select_checker as sc

TWIN = {"ids": _lib.select_host, "bytes": _lib.select_text_host}
SHUFFLE_N = (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 65_537)
SHUFFLE_SEEDS = (0, 2**64 - 1, 0x1234_5678_9ABC_DEF1, 987_654_321)


def _same(got, want, key):
    assert got[0].dtype == want[0].dtype, key
    assert np.array_equal(got[0], want[0]), (key, "data")
    assert np.array_equal(got[1], want[1]), (key, "offsets")


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_twins_match_the_checker_on_the_shapes(kind):
    for k in range(select_cases.N_BATCHES):
        case = select_cases.batch(k, kind)
        got = TWIN[kind](case["data"], case["offs"], case["rows"])
        _same(got, sc.select(case["data"], case["offs"], case["rows"]), (kind, k))
        assert int(got[1][-1]) == case["want_total"], (kind, k)
    case = select_cases.long_row(kind)
    got = TWIN[kind](case["data"], case["offs"], case["rows"])
    _same(got, sc.select(case["data"], case["offs"], case["rows"]), (kind, "long"))
    assert int(got[1][-1]) == case["want_total"]


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_the_cases_have_the_properties_they_are_there_for(kind):
    tile = select_cases.TILE[kind]
    patterns, ds = set(), set()
    src_res, dst_res, straddles, inside = set(), set(), 0, 0
    for k in range(select_cases.N_BATCHES):
        case = select_cases.batch(k, kind)
        offs, rows = case["offs"].astype(np.int64), case["rows"]
        lens = np.diff(offs)
        S = lens.size
        patterns.add(case["pattern"])
        # runs of empty rows at the start, in the middle and at the end of every source
        nz = np.flatnonzero(lens)
        assert lens[0] == 0 and lens[-1] == 0 and (lens[nz[0]:nz[-1]] == 0).any(), k
        assert rows.size == 0 or (0 <= rows.min() and rows.max() < S)
        if case["pattern"] == "identity":
            assert rows.tolist() == list(range(S))
        elif case["pattern"] == "reverse":
            assert rows.tolist() == list(range(S))[::-1]
        elif case["pattern"] == "subset":
            assert len(set(rows.tolist())) == rows.size < S and (np.diff(rows) > 0).all()
        elif case["pattern"] == "repeat":
            assert rows.size > S and np.bincount(rows, minlength=S).max() >= 3
        elif case["pattern"] == "empty":
            assert rows.size >= 1 and (lens[rows] == 0).all() and case["want_total"] == 0
        else:
            assert case["pattern"] == "multiset"
        out_offs = np.concatenate([[0], np.cumsum(lens[rows])])
        total = int(out_offs[-1])
        assert total == case["want_total"]
        if total:
            d = (total + 3) % tile - 3
            assert -3 <= d <= 3, (k, total)
            ds.add(d)
        if kind == "bytes":
            for j, r in enumerate(rows):
                if lens[r]:
                    src_res.add(int(offs[r]) % 16)
                    dst_res.add(int(out_offs[j]) % 16)
            # a slot of 16 output bytes straddles a row boundary / lies inside one row
            starts = set(int(x) for x in out_offs[1:-1])
            for e0 in range(0, total - 15, 16):
                if any(e0 < b < e0 + 16 for b in range(e0 + 1, e0 + 16) if b in starts):
                    straddles += 1
                else:
                    inside += 1
    assert patterns == set(select_cases.PATTERNS)
    assert ds == set(range(-3, 4)), ds
    if kind == "bytes":
        assert src_res == set(range(16)), sorted(src_res)
        assert dst_res == set(range(16)), sorted(dst_res)
        assert straddles >= 100 and inside >= 1000, (straddles, inside)
    case = select_cases.long_row(kind)
    assert np.diff(case["offs"].astype(np.int64)).max() == 70_000 and (case["rows"] == 2).sum() == 3


def test_shuffle_key_and_the_permutation_match_the_checker():
    big = 2**64 - 1
    pairs = [(0, 0), (0, 1), (big, 0), (big, big), (1, 2**63), (0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93)]
    rng = np.random.default_rng(1)
    pairs += [tuple(int(x) * 2 + 1 for x in rng.integers(0, 2**63, 2)) for _ in range(200)]
    for seed, g in pairs:
        assert _lib.shuffle_key(seed, g) == sc.key(seed, g), (seed, g)
    assert sc.keys(5, 7).tolist() == [sc.key(7, g) for g in range(5)]
    # a salt of its own: not the fill-in-the-middle hash's words
    assert sc.SALT == 0xD6E8FEB86659FD93 != 0xA0761D6478BD642F
    for n in SHUFFLE_N:
        seen = []
        for seed in SHUFFLE_SEEDS:
            got = _lib.shuffled_rows_host(n, seed)
            assert got.dtype == np.int64 and np.array_equal(got, sc.shuffled_rows(n, seed)), (n, seed)
            assert np.array_equal(np.sort(got), np.arange(n)), (n, seed)   # a permutation
            seen.append(got.tolist())
        if n >= 255:
            assert all(a != b for i, a in enumerate(seen) for b in seen[i + 1:]), n   # different seeds differ
    with pytest.raises(tgx.TokenGeeXError) as e:
        _lib.shuffled_rows_host(2**31, 0)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    assert _lib.lib.tgx_shuffled_rows_host(0, 5, None) == _lib.OK


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_the_twins_refusals_name_k(kind):
    twin = TWIN[kind]
    dt = np.uint32 if kind == "ids" else np.uint8
    data, offs = np.arange(10, dtype=dt), np.array([0, 3, 3, 10], np.uint64)

    def refused(*a, **kw):
        with pytest.raises(tgx.TokenGeeXError) as e:
            twin(*a, **kw)
        assert e.value.status == _lib.ERR_INVALID, e.value
        return str(e.value)

    assert "rows[2] = -1 " in refused(data, offs, [0, 1, -1, 7])          # the smallest bad k
    assert "rows[1] = 3 " in refused(data, offs, [2, 3, -5])              # index = S
    assert "rows[0] = 4611686018427387904 " in refused(data, offs, [2**62])
    assert "rows[0] = 0 is not a row of 0" in refused(np.zeros(0, dt), np.zeros(1, np.uint64), [0])   # S = 0 with M = 1
    assert "monotone" in refused(data, np.array([0, 5, 3, 10], np.uint64), [0])
    assert "offs[0]" in refused(data, np.array([1, 5, 6, 10], np.uint64), [0])
    assert "room for 9" in refused(data, offs, [2, 0], cap=9)             # T' = 10
    out, out_offs = twin(data, offs, [2, 0], cap=10)
    assert out.tolist() == list(range(3, 10)) + [0, 1, 2] and out_offs.tolist() == [0, 7, 10]
    # nothing selected, from rows and from none
    for src in ((data, offs), (np.zeros(0, dt), np.zeros(1, np.uint64))):
        out, out_offs = twin(*src, [])
        assert out.size == 0 and out_offs.tolist() == [0]
    # NULL arguments at the ABI
    fn = _lib.lib.tgx_select_host if kind == "ids" else _lib.lib.tgx_select_text_host
    one = np.zeros(1, np.int64)
    assert fn(_lib.ptr(data), _lib.ptr(offs), 3, _lib.ptr(one), 1, _lib.ptr(np.zeros(16, dt)), 16, None) == _lib.ERR_INVALID
    assert fn(_lib.ptr(data), _lib.ptr(offs), 3, None, 1, _lib.ptr(np.zeros(16, dt)), 16, _lib.ptr(np.zeros(2, np.uint64))) == _lib.ERR_INVALID
    assert fn(None, _lib.ptr(offs), 3, _lib.ptr(one), 1, _lib.ptr(np.zeros(16, dt)), 16, _lib.ptr(np.zeros(2, np.uint64))) == _lib.ERR_INVALID


def test_the_python_argument_forms_agree():
    case = select_cases.batch(2, "ids")
    data, offs = case["data"], case["offs"]
    S = offs.size - 1
    mask = np.zeros(S, bool)
    mask[[1, 3, S - 2]] = True
    idx = np.flatnonzero(mask)
    want = sc.select(data, offs, idx)
    for rows in (idx.tolist(), idx.astype(np.int32), idx.astype(np.uint8), idx.astype(np.uint64), mask, tuple(idx.tolist())):
        _same(_lib.select_host(data, offs, rows), want, type(rows))
    text = (data % 251).astype(np.uint8)
    _same(_lib.select_text_host(text, offs, mask), sc.select(text, offs, idx), "mask over bytes")
    with pytest.raises(ValueError):
        _lib.select_host(data, offs, mask[:-1])          # a mask of another length
    with pytest.raises(TypeError):
        _lib.select_host(data, offs, np.array([0.0, 1.0]))
    with pytest.raises(TypeError):
        _lib.select_host(data, offs, np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        _lib.select_host(data, offs, np.array([2**63], np.uint64))


def test_select_last_times_names_its_stages_without_a_call():
    times = _lib.select_last_times()
    assert list(times) == ["select_check", "select_offsets_scan", "select_fill_kernel"]
    names = (C.c_char_p * 2)()
    assert _lib.lib.tgx_select_last_times(names, None, 2) == 2 and names[1] == b"select_offsets_scan"
