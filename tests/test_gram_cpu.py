"""The shared n-grams without a device: the host twins (tgx_gram_keys_host, tgx_gram_hits_host, tgx_gram_contains_host,
tgx_gram_key; they walk the kernels' chunks, tiles, directory and store / add rule through csrc/gram.h) against the
independent checker (tests/gram_checker.py) on the batches of tests/gram_cases.py, and the batches against the geometry
they claim.  Everything is compared exactly: this is integer work."""
import functools

import numpy as np
import pytest

from tokengeex_amd import _lib

import gram_cases
import gram_checker as gc
from gram_cases import CAP, CHUNK, RUN, TILE

SEED = 0xC0FFEE1234567890


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    c = gram_cases.past_cap_case(kind) if name == "past_cap" else gram_cases.case(name, kind)
    for a in (c["data"], c["offs"], c["eval_data"], c["eval_offs"]):
        a.setflags(write=False)
    return c


@pytest.mark.parametrize("name,kind", gram_cases.all_cases() + [("past_cap", k) for k in gram_cases.KINDS])
def test_twins_match_checker(name, kind):
    c = _case(name, kind)
    w = c["width"]
    for seed in (0, SEED):
        keys = gc.keys_of(c["eval_data"], c["eval_offs"], w, seed)
        assert np.array_equal(_lib.gram_keys_host(c["eval_data"], c["eval_offs"], w, seed), keys), seed
        want_count, want_mask = gc.hits(c["data"], c["offs"], w, seed, keys)
        count, mask = _lib.gram_hits_host(c["data"], c["offs"], w, seed, keys)
        assert np.array_equal(count, want_count) and np.array_equal(mask, want_mask), seed
        assert (mask[c["planted"]] == 1).all(), "every planted gram is found"
    # distinct grams have distinct keys, so membership by key is membership by gram
    assert gc.distinct_grams_have_distinct_keys([(c["data"], c["offs"]), (c["eval_data"], c["eval_offs"])], w, SEED)
    true_count, true_mask = gc.true_hits(c["data"], c["offs"], w, c["eval_data"], c["eval_offs"])
    assert np.array_equal(want_count, true_count) and np.array_equal(want_mask, true_mask)


@pytest.mark.parametrize("name,kind", gram_cases.all_cases())
def test_a_source_against_its_own_set(name, kind):
    c = _case(name, kind)
    w = c["width"]
    keys = _lib.gram_keys_host(c["data"], c["offs"], w, SEED)
    assert np.array_equal(keys, gc.keys_of(c["data"], c["offs"], w, SEED))
    count, mask = _lib.gram_hits_host(c["data"], c["offs"], w, SEED, keys)
    lens = np.diff(c["offs"].astype(np.int64))
    assert np.array_equal(count, np.maximum(0, lens - w + 1))
    assert np.array_equal(mask.astype(bool), gc.validity(c["offs"], w))


def test_gram_key_is_the_row_hash_of_the_grams_bytes():
    import dedup_checker as dc
    c = _case("short_w5", "ids")
    row = next(r for r in c["rows"] if len(r) == 5)
    raw = np.asarray(row, "<u4").tobytes()
    for seed in (0, SEED):
        want = dc.row_hash(raw, (seed ^ gc.MINHASH_SALT) & dc.M64)
        assert _lib.gram_key(raw, seed) == want == _lib.row_hash(raw, seed ^ gc.MINHASH_SALT)
        data, offs = gram_cases.pack([row], "ids")
        assert _lib.gram_keys_host(data, offs, 5, seed).tolist() == [want]


# ---- the batches hold the geometry they claim -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", gram_cases.KINDS)
def test_cases_hold_their_geometry(kind):
    for name in ("short_w1", "short_w5", "short_w13", "short_wmax"):
        c = _case(name, kind)
        w = c["width"]
        lens = [len(r) for r in c["rows"]]
        assert w == gram_cases.width_of(name, kind) and set(range(w + 3)) <= set(lens)
        assert lens[:3] == [0, 0, 0] and lens[-2:] == [0, 0] and any(lens[i] == lens[i + 1] == 0 for i in range(3, len(lens) - 3))
    assert _case("short_wmax", kind)["width"] * gram_cases.DTYPE[kind]().itemsize == 64
    for name, edge in gram_cases.EDGES.items():
        c = _case(name, kind)
        ends = c["offs"][1:].astype(np.int64)
        from_edge = {int((e + 3) % edge) - 3 for e in ends}
        assert {-3, -2, -1, 0, 1, 2, 3} <= from_edge, name
        astride = [p for p in c["planted"] if p // edge != (p + c["width"] - 1) // edge]
        assert len(astride) >= 7, "a planted gram straddles an edge in every round"
    c = _case("all_short", kind)
    assert max(len(r) for r in c["rows"]) < c["width"] and max(np.diff(c["eval_offs"].astype(np.int64))) < c["width"]
    assert _lib.gram_keys_host(c["eval_data"], c["eval_offs"], c["width"], 0).size == 0
    count, mask = _lib.gram_hits_host(c["data"], c["offs"], c["width"], 0, np.zeros(0, np.uint64))
    assert not count.any() and not mask.any()
    c = _case("alignments", kind)
    assert {int(o) % 4 for o in c["offs"][:-1]} == {0, 1, 2, 3}
    c = _case("long_among_short", kind)
    lens = np.diff(c["offs"].astype(np.int64))
    assert lens.max() == 5 * TILE + 37 and np.median(lens) < 40


@pytest.mark.parametrize("kind", gram_cases.KINDS)
def test_past_cap_case_is_past_the_cap(kind):
    c = _case("past_cap", kind)
    offs = c["offs"].astype(np.int64)
    n = int(offs[-1])
    assert n == CAP * TILE + 2 * TILE + 70
    n_tiles = -(-n // TILE)
    per_block = -(-n_tiles // min(n_tiles, CAP))
    assert n_tiles > CAP and per_block == 2 and RUN == per_block * TILE
    assert n_tiles % per_block == 1 and n - (n_tiles - 1) * TILE == CHUNK + 6, "the last working block has one tile of two chunks, one short"
    a, z = offs[c["where"]["inside"]], offs[c["where"]["inside"] + 1] - 1
    assert a // RUN == z // RUN and a // TILE + 1 == z // TILE, "from a run's first tile into its second"
    a, z = offs[c["where"]["straddle"]], offs[c["where"]["straddle"] + 1] - 1
    assert a // RUN + 1 == z // RUN, "from one block's run into the next"
    a, z = offs[c["where"]["long"]], offs[c["where"]["long"] + 1] - 1
    assert z // RUN - a // RUN >= 2
    lens = np.diff(offs)
    assert {0, 1, c["width"] - 1, c["width"]} <= set(lens.tolist()) and lens[:3].tolist() == [0, 0, 0] and lens[-2:].tolist() == [0, 0]


# ---- hostile key sets ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gram_cases.HOSTILE)
def test_membership_in_hostile_sets(name):
    keys = gram_cases.hostile_keys(name)
    probes = gram_cases.hostile_probes(keys)
    got = _lib.gram_contains_host(keys, probes)
    assert np.array_equal(got, np.isin(probes, keys)), name
    assert got[:keys.size].all()
    # and through the whole twin: a source's own keys against the hostile keys, half of the source's and the rest's neighbours
    c = _case("edges_chunk", "ids")
    mine = gc.keys_of(c["data"], c["offs"], c["width"], SEED)
    with np.errstate(over="ignore"):
        mixed = np.concatenate([keys, mine[::2], mine[1::2] + np.uint64(1), mine[1::4] - np.uint64(1)])
    count, mask = _lib.gram_hits_host(c["data"], c["offs"], c["width"], SEED, mixed)
    want_count, want_mask = gc.hits(c["data"], c["offs"], c["width"], SEED, mixed)
    assert np.array_equal(count, want_count) and np.array_equal(mask, want_mask) and 0 < mask.sum() < gc.validity(c["offs"], c["width"]).sum()


def test_hostile_sets_hold_their_geometry():
    bits = {n: gram_cases.dir_bits(np.unique(gram_cases.hostile_keys(n)).size) for n in gram_cases.HOSTILE}
    assert bits["empty"] == bits["one"] == 0 and bits["ends"] == 1 and (bits["n255"], bits["n256"], bits["n257"]) == (8, 8, 9)
    keys = gram_cases.hostile_keys("one_bucket")
    assert np.unique(keys).size == 300 and np.unique(keys >> np.uint64(36)).size == 1 and bits["one_bucket"] == 9
    keys = gram_cases.hostile_keys("unsorted_dups")
    assert np.unique(keys).size < keys.size and (np.diff(keys.astype(np.float64)) < 0).any()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_twins_refuse_bad_arguments():
    lib = _lib.lib
    d = np.asarray([1, 2, 3], np.uint8)
    good, bad0, bad1 = (np.asarray(x, np.uint64) for x in ([0, 1, 3], [1, 2, 3], [0, 3, 2]))
    keys_out, nk = np.full(3, 9, np.uint64), _lib.C.c_uint64(77)
    count, mask = np.full(2, 9, np.int64), np.full(3, 9, np.uint8)
    p = _lib.ptr
    for offs, eb, w in ((bad0, 1, 2), (bad1, 1, 2), (good, 3, 2), (good, 1, 0), (good, 1, 65), (good, 4, 17)):
        assert lib.tgx_gram_keys_host(p(d), eb, p(offs), 2, w, 0, p(keys_out), _lib.C.byref(nk)) == _lib.ERR_INVALID, (eb, w)
        assert lib.tgx_gram_hits_host(p(d), eb, p(offs), 2, w, 0, None, 0, p(count), p(mask)) == _lib.ERR_INVALID, (eb, w)
    assert lib.tgx_gram_hits_host(p(d), 1, p(good), 2, 2, 0, None, 0, None, None) == _lib.ERR_INVALID
    assert lib.tgx_gram_hits_host(p(d), 1, p(good), 2, 2, 0, None, 5, p(count), p(mask)) == _lib.ERR_INVALID
    assert (keys_out == 9).all() and (count == 9).all() and (mask == 9).all(), "a refused call writes nothing"
    assert lib.tgx_gram_hits_host(p(d), 1, p(good), 2, 2, 0, None, 0, p(count), None) == 0 and count.tolist() == [0, 0]   # either may be NULL
    assert lib.tgx_gram_hits_host(p(d), 1, p(good), 2, 2, 0, None, 0, None, p(mask)) == 0 and mask.tolist() == [0, 0, 0]
