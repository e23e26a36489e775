"""Exact row deduplication without a GPU: the host twin (tgx_first_equal_host: the device's rounds through csrc/dedup.h)
and tgx_row_hash against the independent restatement of tests/dedup_checker.py on the batches of tests/dedup_cases.py,
the collision rounds included (hash_bits 4, 1 and 0), the twin's error returns, and what the device entry points say on a
machine without a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dedup_cases
import dedup_checker as dc

STAGES = ["dedup_hash_kernel", "dedup_sort", "dedup_compare_kernel", "dedup_resolve"]


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    c = dedup_cases.case(name, kind)
    c["want"] = dc.first_equal(c["data"], c["offs"])
    for a in (c["data"], c["offs"], c["want"][0]):
        a.setflags(write=False)
    return c


def test_case_is_as_designed():
    cases = [_case(n, k) for n, k in dedup_cases.all_cases()]
    for kind in dedup_cases.KINDS:
        mine = {c["name"]: c for c in cases if c["kind"] == kind}
        tile = dedup_cases.TILE[kind]
        lens = {len(r) for c in mine.values() for r in c["rows"]}
        assert set(dedup_cases.SMALL_LENGTHS) <= lens
        assert {m * tile + d for m in (1, 4) for d in (-3, -2, -1, 1, 2, 3)} <= lens
        assert 70_000 in lens
        # runs of empty rows at the start, in the middle and at the end of one batch
        e = [len(r) == 0 for r in mine["lengths"]["rows"]]
        inner = [i for i in range(2, len(e) - 2) if e[i] and e[i + 1] and not e[i - 1]]
        assert e[0] and e[1] and e[-1] and e[-2] and inner and not all(e)
        # the duplicate patterns
        first = lambda name: [int(x) for x in mine[name]["want"][0]]
        assert set(first("all_equal")) == {0} and len(first("all_equal")) >= 2
        assert first("all_distinct") == list(range(len(first("all_distinct"))))
        f = first("first_last")
        assert f[-1] == 0 and f[:-1] == list(range(len(f) - 1))
        f = first("pairs")
        gaps = {k - f[k] for k in range(len(f)) if f[k] != k}
        assert 1 in gaps and max(gaps) == len(f) - 1
        assert max(np.bincount(first("group40"))) == 40
        # rows that differ in one place only
        for name, at in (("last_element", -1), ("first_element", 0)):
            rows = mine[name]["rows"]
            for a, b in zip(rows[0:12:2], rows[1:12:2]):
                assert len(a) == len(b) and a != b and a[at] != b[at]
                assert (a[:-1] == b[:-1]) if at == -1 else (a[1:] == b[1:])
        rows = mine["trailing_zero"]["rows"]
        for i in range(0, 12, 3):
            assert rows[i + 1] == rows[i] + (0,) and rows[i + 2] == rows[i] + (0, 0) and 0 not in rows[i]
        per = 8 if kind == "bytes" else 2
        words = lambda r: sorted(r[i:i + per] for i in range(0, len(r), per))
        rows = mine["word_swap"]["rows"]
        assert len(set(rows[:4])) == 4 and all(words(r) == words(rows[0]) for r in rows[:4])
        rows = mine["long"]["rows"]
        big = [r for r in rows if len(r) == 70_000]
        assert len(big) == 4 and len(set(big)) == 2 and sorted(big.count(r) for r in set(big)) == [1, 3]
        odd = [r for r in big if big.count(r) == 1][0]
        assert odd[:-1] == big[0][:-1] and odd[-1] != big[0][-1]
        for c in mine.values():
            assert 1 <= c["n_distinct"] <= dedup_cases.MAX_DISTINCT, c["name"]
            assert c["n_distinct"] == c["want"][1]
    # text rows start at every byte alignment mod 8, and so do rows that have an earlier equal
    c = _case("alignments", "bytes")
    starts = [int(x) % 8 for x in c["offs"][:-1]]
    assert set(starts) == set(range(8))
    assert {starts[k] for k in range(len(starts)) if c["want"][0][k] != k} == set(range(8))


@pytest.mark.parametrize("name,kind", dedup_cases.all_cases())
def test_twin_matches_the_checker(name, kind):
    c = _case(name, kind)
    want_first, want_unique = c["want"]
    for bits in (64, 4, 1, 0):
        first, n_unique, n_rounds = _lib.first_equal_host(c["data"], c["offs"], hash_bits=bits)
        assert np.array_equal(first, want_first), bits
        assert n_unique == want_unique, bits
        if bits == 64:
            assert n_rounds == 1
        elif bits == 0:
            assert n_rounds == c["n_distinct"]
        else:
            assert 1 <= n_rounds <= c["n_distinct"]


def test_row_hash_matches_the_restatement():
    rng = np.random.default_rng(7)
    lengths = list(dedup_cases.SMALL_LENGTHS) + [4093, 4096, 4099, 16381, 16387]
    for n in lengths:
        row = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        for seed in (0, 1, 0xDEADBEEFCAFEF00D):
            assert _lib.row_hash(row, seed) == dc.row_hash(row, seed), (n, seed)
    # trailing zeros: the same words, another length, another hash
    assert len({_lib.row_hash(b"abc" + b"\0" * k) for k in range(6)}) == 6
    assert _lib.row_hash(b"") == dc.row_hash(b"") and _lib.row_hash(b"", 5) != _lib.row_hash(b"", 6)


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_vectorised_row_hash_matches_the_scalar_one(kind):
    for name in dedup_cases.NAMES:
        c = _case(name, kind)
        rows = dc.row_bytes(c["data"], c["offs"])
        for seed in (0, 0x9E3779B97F4A7C15):
            want = np.asarray([dc.row_hash(r, seed) for r in rows], np.uint64)
            assert np.array_equal(dc.row_hashes(c["data"], c["offs"], seed), want), (name, seed)
    assert dc.row_hash_equal_length(np.zeros((3, 0), np.uint8), 5).tolist() == [dc.row_hash(b"", 5)] * 3


@functools.lru_cache(maxsize=None)
def _past_cap(kind):
    c = dedup_cases.past_cap_case(kind)
    c["want"] = dc.first_equal(c["data"], c["offs"])
    for a in (c["data"], c["offs"], c["want"][0]):
        a.setflags(write=False)
    return c


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_past_cap_case_reaches_every_threshold(kind):
    """the arithmetic of csrc/dedup.hip's launchers on the batch, from the mirrored constants"""
    c = _past_cap(kind)
    cap, tile_h, cmp_tile = 2048, 4096, dedup_cases.TILE[kind]   # kDedupMaxBlocks, kDedupTile, kDedupCmpByteTile / kDedupCmpTile
    w = c["data"].dtype.itemsize
    lens = np.diff(c["offs"].astype(np.int64))
    S = lens.size
    where = c["where"]
    first, n_unique = c["want"]
    pad_offs = np.concatenate([[0], np.cumsum(dedup_cases.pad_bytes(lens, w))])
    n_pad = int(pad_offs[-1])
    n_tiles = -(-n_pad // tile_h)
    grid = min(cap, -(-(c["data"].size * w + 7 * S) // tile_h))
    per_block = -(-n_tiles // grid)
    print(f"{kind}: rows {S}, padded bytes {n_pad}, n_tiles {n_tiles}, grid {grid}, per_block {per_block}")
    assert n_pad > cap * tile_h + tile_h and n_tiles >= 2050 and grid == cap and per_block == 2
    working = -(-n_tiles // per_block)
    assert n_tiles % 2 == 1 and working < grid, "the last working block has a run of one tile, and blocks behind it have none"
    run = per_block * tile_h
    k = where["carry"]      # inside one block's run, over both of its tiles
    assert pad_offs[k] % run == tile_h // 2 and pad_offs[k] // run == (pad_offs[k + 1] - 1) // run
    assert pad_offs[k] // tile_h + 1 == (pad_offs[k + 1] - 1) // tile_h and lens[k] == cmp_tile + 3
    k = where["two_blocks"]  # from the second tile of one block's run into the first tile of the next block's
    assert (pad_offs[k] // tile_h) % 2 == 1 and (pad_offs[k + 1] - 1) // tile_h == pad_offs[k] // tile_h + 1 and lens[k] == cmp_tile - 1
    assert {int(n) - cmp_tile for n in lens[where["rows"]]} >= {-3, -2, -1, 1, 2, 3}
    # the compare at 64 key bits: the candidates are the rows with an earlier equal
    dup = first != np.arange(S)
    cmp_total = int(lens[dup].sum())
    print(f"{kind}: duplicates {int(dup.sum())}, compare total {cmp_total} elements, compare tiles {-(-cmp_total // cmp_tile)}")
    assert cmp_total > cap * cmp_tile + cmp_tile
    big = where["big"]
    assert (lens[big] == 70_000).all() and (first[big] == big[0]).all()
    data, offs = c["data"], c["offs"].astype(np.int64)
    row = lambda k: data[offs[k]:offs[k + 1]]
    a = row(big[0])
    top = lambda r: dc.row_hash(dc.row_bytes(r, np.asarray([0, r.size]))[0]) >> (64 - c["low_bits"])
    for name, at in (("mid", 35_000), ("first", 0), ("last", 69_999)):
        k = where[name]
        b = row(k)
        assert b.size == a.size and np.flatnonzero(a != b).tolist() == [at] and first[k] == k
        assert top(a) == top(b), "a candidate of the row it was made from under the knob"
        # the candidates of 70 000 elements before it in that round: every earlier copy but the head
        assert ((big < k).sum() - 1) * 70_000 >= cap * cmp_tile, "every element of the row is compared in the second trip"
    assert big[-1] > where["last"]
    # the kernels with a thread per row
    assert S > 256 * cap and (lens[256 * cap - 2:256 * cap + 3] == 0).all()
    assert (lens[:3] == 0).all() and (lens[-3:] == 0).all()
    # a run of empty rows at the edge between the two tiles of a block's run
    e = np.flatnonzero((lens[:-1] == 0) & (lens[1:] == 0) & (pad_offs[:-2] % run == tile_h))
    assert e.size and (lens[e[0] + 1:] > 0).any()
    # the collision run: a short content before the long part has the 70 000-element row's key, so round two lists every copy
    pool_keys = {dc.row_hash(dc.row_bytes(p, np.asarray([0, p.size]))[0]) >> (64 - c["low_bits"]) for p in c["pool"]}
    assert top(a) in pool_keys and where["rows"][0] >= dedup_cases.SHORT_A
    assert big.size * int(dedup_cases.pad_bytes(70_000, w)) > cap * tile_h + tile_h
    assert n_unique == len(c["pool"]) + c["n_long_contents"]
    assert where["edge_rows"].size > 1000, "the rows on either side of the tile edges that short rows own"


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_twin_matches_the_checker_past_the_caps(kind):
    c = _past_cap(kind)
    want_first, want_unique = c["want"]
    for bits in (64, c["low_bits"]):
        first, n_unique, n_rounds = _lib.first_equal_host(c["data"], c["offs"], hash_bits=bits)
        assert np.array_equal(first, want_first) and n_unique == want_unique, bits
        print(f"{kind}: {bits} key bits, {n_rounds} rounds")
        assert (n_rounds == 1) if bits == 64 else (2 <= n_rounds <= dedup_cases.MAX_DISTINCT)


def test_twin_refuses_bad_arguments():
    lib = _lib.lib
    data = np.arange(8, dtype=np.uint8)
    first = np.full(4, -7, np.int64)
    nu, nr = C.c_uint64(99), C.c_uint32(99)

    def call(offs, n_rows, elem=1, bits=64, d=data, f=first):
        offs = np.asarray(offs, np.uint64)
        return lib.tgx_first_equal_host(_lib.ptr(d) if d is not None else None, elem, _lib.ptr(offs) if offs.size else None, n_rows, bits,
                                        _lib.ptr(f) if f is not None else None, C.byref(nu), C.byref(nr))

    assert call([0, 2, 4, 6, 8], 4) == 0 and first.tolist() == [0, 1, 2, 3]
    first[:] = -7
    assert call([1, 2, 4, 6, 8], 4) == _lib.ERR_INVALID and b"offs[0] must be 0" in lib.tgx_last_error()
    assert call([0, 4, 2, 6, 8], 4) == _lib.ERR_INVALID and b"not monotone" in lib.tgx_last_error()
    assert call([], 4) == _lib.ERR_INVALID
    assert call([0, 2, 4, 6, 8], 4, elem=3) == _lib.ERR_INVALID and b"elem_bytes" in lib.tgx_last_error()
    assert call([0, 2, 4, 6, 8], 4, elem=2) == _lib.ERR_INVALID
    assert call([0, 2, 4, 6, 8], 4, bits=65) == _lib.ERR_INVALID and b"hash_bits" in lib.tgx_last_error()
    assert call([0, 2, 4, 6, 8], 4, d=None) == _lib.ERR_INVALID
    assert call([0, 2, 4, 6, 8], 4, f=None) == _lib.ERR_INVALID
    assert first.tolist() == [-7] * 4          # a refused call writes nothing
    # no rows: nothing to write, and neither data nor first is looked at
    assert call([0], 0, d=None, f=None) == 0 and (nu.value, nr.value) == (0, 0)
    f, n_unique, n_rounds = _lib.first_equal_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert f.size == 0 and (n_unique, n_rounds) == (0, 0)
    # rows without elements only: one content, one round
    f, n_unique, n_rounds = _lib.first_equal_host(np.zeros(0, np.uint32), np.zeros(6, np.uint64), hash_bits=0)
    assert f.tolist() == [0] * 5 and (n_unique, n_rounds) == (1, 1)
    with pytest.raises(TypeError):
        _lib.first_equal_host(np.zeros(4, np.uint16), np.asarray([0, 4], np.uint64))


def test_stage_names_are_listed_without_a_call():
    assert list(_lib.dedup_last_times()) == STAGES
    assert isinstance(_lib.dedup_last_rounds(), int)
    for name in ("first_equal", "unique_rows", "row_hashes"):
        assert getattr(tgx, name) is getattr(tgx.tensors, name)


def test_device_calls_ask_for_a_device_first():
    """NULL handles: without a device TGX_ERR_DEVICE (there is no host fallback), with one TGX_ERR_INVALID."""
    have_gpu = tgx.device_count() > 0
    lib = _lib.lib
    nu = C.c_uint64()
    calls = {
        "tgx_corpus_first_equal_device": lambda: lib.tgx_corpus_first_equal_device(None, 0, None, None, C.byref(nu)),
        "tgx_result_first_equal_device": lambda: lib.tgx_result_first_equal_device(None, 0, None, None, C.byref(nu)),
        "tgx_corpus_row_hashes_device": lambda: lib.tgx_corpus_row_hashes_device(None, 0, None, None),
        "tgx_result_row_hashes_device": lambda: lib.tgx_result_row_hashes_device(None, 0, None, None),
    }
    for name, call in calls.items():
        status = call()
        msg = lib.tgx_last_error() or b""
        if have_gpu:
            assert status == _lib.ERR_INVALID and msg.startswith(name.encode() + b": "), name
        else:
            assert (status, msg) == (_lib.ERR_DEVICE, b"no usable HIP device (gfx950 required)"), name
