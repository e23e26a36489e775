"""Near-duplicate rows without a GPU: the host twins (tgx_minhash_host, tgx_minhash_bands_host,
tgx_minhash_near_first_host: the kernel's tiles, chunks and rules through csrc/minhash.h) and tgx_minhash_value against
the independent restatement of tests/minhash_checker.py on the batches of tests/minhash_cases.py, the twins' error
returns, what the device entry points say on a machine without a device, and the estimator: the share of agreeing
signature values against the true Jaccard similarity, within the binomial standard error."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dedup_checker as dc
import minhash_cases
import minhash_checker as mc

STAGES = ["minhash_sig_kernel", "minhash_band_keys", "minhash_sort", "minhash_heads", "minhash_verify", "minhash_roots"]
SEEDS = (0, 0xC0FFEE1234567890)


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """a case with the checker's answers under seed 0: computed once, never changed"""
    c = minhash_cases.case(name, kind)
    c["sig"] = mc.signatures(c["data"], c["offs"], c["width"], c["n_perm"])
    for a in (c["data"], c["offs"], c["sig"]):
        a.setflags(write=False)
    return c


def test_cases_are_as_designed():
    for kind in minhash_cases.KINDS:
        mine = {n: _case(n, kind) for n in minhash_cases.NAMES}
        for name in ("short_w1", "short_w5", "short_wmax"):
            c = mine[name]
            lens = [len(r) for r in c["rows"]]
            assert set(range(c["width"] + 3)) <= set(lens)
            e = [n == 0 for n in lens]
            inner = [i for i in range(3, len(e) - 3) if e[i] and e[i + 1] and not e[i - 1]]
            assert e[0] and e[1] and e[-1] and e[-2] and inner
        assert mine["short_wmax"]["width"] * c["data"].dtype.itemsize == 64
        for name, edge in zip(("edges_chunk", "edges_tile", "edges_four_tiles"), minhash_cases.EDGES):
            c = mine[name]
            ends = np.cumsum([minhash_cases.positions(len(r), c["width"]) for r in c["rows"]])
            assert {d for d in range(-3, 4) if any((int(x) - d) % edge == 0 and int(x) - d > 0 for x in ends)} == set(range(-3, 4))
        c = mine["long_among_short"]
        m = [minhash_cases.positions(len(r), c["width"]) for r in c["rows"]]
        assert 5 * minhash_cases.TILE < max(m) < 6 * minhash_cases.TILE and sorted(m)[-3] < minhash_cases.CHUNK
        rows = mine["contents"]["rows"]
        assert rows[1] == rows[0] + (0,) and rows[2] == rows[0] + (0, 0) and len(rows[0]) < 5 and rows[4] == rows[3] + (0,)
        assert len(set(rows[6])) == 1 and len(set(mc.shingles(rows[6], 5))) == 1
        assert sum(a != b for a, b in zip(rows[8], rows[9])) == 1 and len(rows[8]) == len(rows[9])
        assert sorted(rows[10]) == sorted(rows[11]) and rows[10] != rows[11]
        top = minhash_cases.TOP[kind]
        assert {0, top} == set(mine["extremes"]["data"].tolist())
    assert {minhash_cases.SHAPE[n][1] for n in minhash_cases.NAMES} == {1, 64, 65, 128, 250}
    assert (25 in minhash_cases.SHAPE["long_among_short"][2]) and minhash_cases.SHAPE["long_among_short"][1] == 250


@pytest.mark.parametrize("name,kind", minhash_cases.all_cases() + minhash_cases.wide_cases())
def test_twins_match_the_checker(name, kind):
    c = _case(name, kind)
    K = c["n_perm"]
    sig = _lib.minhash_host(c["data"], c["offs"], c["width"], K)
    assert sig.dtype == np.uint32 and np.array_equal(sig, c["sig"])
    seeded = _lib.minhash_host(c["data"], c["offs"], c["width"], K, SEEDS[1])
    assert np.array_equal(seeded, mc.signatures(c["data"], c["offs"], c["width"], K, SEEDS[1])) and not np.array_equal(seeded, sig)
    for bands in c["bands"]:
        for seed in SEEDS:
            keys, heads = _lib.minhash_bands_host(sig, bands, seed)
            want_keys = mc.band_keys(c["sig"], bands, seed)
            want_heads = mc.heads_of(want_keys)
            assert np.array_equal(keys, want_keys), (bands, seed)
            assert np.array_equal(heads, want_heads), (bands, seed)
        for min_agree in sorted({1, (K + 1) // 2, K}):
            first, n_clusters = _lib.minhash_near_first_host(sig, heads, min_agree)
            want_first, want_clusters, _ = mc.near_first(c["sig"], want_heads, min_agree)
            assert np.array_equal(first, want_first), (bands, min_agree)
            assert n_clusters == want_clusters, (bands, min_agree)


def test_wide_cases_take_the_wide_kernels():
    """P = ceil(K / 64) of the wide cases: 5 and 8 (minhash_sig_kernel<*, 8>), 9 and 16 (<*, 16>), with and without a tail"""
    K = [minhash_cases.WIDE[n][1] for n in minhash_cases.WIDE_NAMES]
    assert K == [257, 512, 513, 1000, 1024] and [-(-k // 64) for k in K] == [5, 8, 9, 16, 16] and [k % 64 for k in K] == [1, 0, 1, 40, 0]
    assert [minhash_cases.WIDE[n][2] for n in minhash_cases.WIDE_NAMES] == [(1, 257), (128,), (1, 27), (250, 8), (32,)]
    for name in minhash_cases.WIDE_NAMES:
        base = minhash_cases.WIDE[name][0]
        a, b = _case(name, "ids"), _case(base, "ids")
        assert [len(r) for r in a["rows"]] == [len(r) for r in b["rows"]] and a["width"] == b["width"] and a["rows"] != b["rows"]
    assert not set(minhash_cases.WIDE_NAMES) & set(minhash_cases.NAMES)


@pytest.mark.parametrize("name,kind", minhash_cases.all_cases() + minhash_cases.wide_cases())
def test_vectorised_references_match_the_scalar_ones(name, kind):
    c = _case(name, kind)
    K = c["n_perm"]
    for bands in c["bands"]:
        for seed in SEEDS:
            keys = mc.band_keys(c["sig"], bands, seed)
            assert np.array_equal(mc.band_keys_np(c["sig"], bands, seed), keys), (bands, seed)
            heads = mc.heads_of(keys)
            assert np.array_equal(mc.heads_of_np(keys), heads), (bands, seed)
        for min_agree in sorted({1, (K + 1) // 2, K}):
            want, got = mc.near_first(c["sig"], heads, min_agree), mc.near_first_memo(c["sig"], heads, min_agree)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and np.array_equal(got[2], want[2]), (bands, min_agree)


@pytest.mark.parametrize("kind", minhash_cases.KINDS)
def test_past_cap_case_reaches_every_threshold(kind):
    """the arithmetic of launch_minhash_sig and of minhash_sig_kernel on the batch, from the mirrored constants"""
    cap, tile, chunk = 2048, 256, 64          # kMinhashMaxBlocks, kMinhashTile, kMinhashChunk
    c = minhash_cases.past_cap_case(kind)
    w, where = c["width"], c["where"]
    lens = np.diff(c["offs"].astype(np.int64))
    S = lens.size
    sh_offs = np.concatenate([[0], np.cumsum(np.maximum(1, lens - w + 1))])
    M = int(sh_offs[-1])
    n_tiles = -(-M // tile)
    grid = min(cap, -(-(c["data"].size + S) // tile))
    per_block = -(-n_tiles // grid)
    print(f"{kind}: rows {S}, positions {M}, n_tiles {n_tiles}, grid {grid}, per_block {per_block}")
    assert M >= cap * tile + tile + 1 and grid == cap and per_block == 2 and 2000 < S < 5000
    assert n_tiles % 2 == 1 and -(-n_tiles // 2) < grid and chunk < M % tile <= 2 * chunk
    assert w == 2 and c["n_perm"] == 65 and np.unique(c["data"]).size <= 16
    run = per_block * tile
    assert {(e, d) for _, e, d in where["ends"]} == {(e, d) for e in (tile, tile + chunk, run) for d in range(-3, 4)}
    for row, edge, d in where["ends"]:
        assert (sh_offs[row + 1] - edge - d) % run == 0 and sh_offs[row + 1] - sh_offs[row] > chunk, (row, edge, d)
    k = where["inside"]
    assert sh_offs[k] % run == 30 and sh_offs[k + 1] - sh_offs[k] == 410 and sh_offs[k] // run == (sh_offs[k + 1] - 1) // run
    k = where["straddle"]
    assert sh_offs[k] % run == 300 and sh_offs[k + 1] - sh_offs[k] == 5 * tile + 37
    assert (sh_offs[k + 1] - 1) // run - sh_offs[k] // run == 3
    assert set(range(w + 3)) <= set(lens.tolist()) and (lens[:3] == 0).all() and (lens[-3:] == 0).all()
    for seed in SEEDS:
        assert np.array_equal(_lib.minhash_host(c["data"], c["offs"], w, 65, seed), mc.signatures(c["data"], c["offs"], w, 65, seed)), seed


def test_twins_match_the_references_past_the_row_caps():
    cap, block = 2048, 256                     # kMinhashMaxBlocks, kMinhashBlock
    sig, alone = minhash_cases.band_rows_sig()
    S = sig.shape[0]
    assert S > block * cap and sig.shape[1] == 2
    for bands in (1, 2):
        keys = mc.band_keys_np(sig, bands, 3)
        heads = mc.heads_of_np(keys)
        twin_keys, twin_heads = _lib.minhash_bands_host(sig, bands, 3)
        assert np.array_equal(twin_keys, keys) and np.array_equal(twin_heads, heads), bands
        sizes = np.bincount(heads[:, 0], minlength=S)
        assert (sizes[alone] == 1).all() and (sizes > 1000).sum() >= 12 and (sizes == 1).sum() == alone.size
    sig = minhash_cases.verify_rows_sig()
    S, K = sig.shape
    assert S > 4 * 16384 and K == 65            # launch_minhash_verify: four rows per block, 8 * kMinhashMaxBlocks blocks
    heads = mc.heads_of_np(mc.band_keys_np(sig, 13))
    first, n_clusters, first0 = mc.near_first_memo(sig, heads, 40)
    twin_first, twin_clusters = _lib.minhash_near_first_host(sig, heads, 40)
    assert np.array_equal(twin_first, first) and twin_clusters == n_clusters
    me = np.arange(S)
    linked = first0 != me
    agree = (sig == sig[first0]).sum(axis=1)
    shares_a_band = (heads < me[:, None]).any(axis=1)
    print(f"rows {S}, clusters {n_clusters}, linked {int(linked.sum())}, share a band with an earlier row but are not linked {int((shares_a_band & ~linked).sum())}")
    assert linked.sum() > S // 4 and (shares_a_band & ~linked).sum() > 100 and (agree[linked] >= 40).all() and (agree[linked] < 65).any()


def test_chains_and_heads_from_elsewhere():
    for S in minhash_cases.CHAIN_SIZES:
        sig, heads, want_first, want_clusters, min_agree = minhash_cases.chain_case(S)
        first, n_clusters = _lib.minhash_near_first_host(sig, heads, min_agree)
        assert np.array_equal(first, want_first) and n_clusters == want_clusters == 1, S
    sig, heads, want_first, want_clusters, min_agree = minhash_cases.forest_case()
    first, n_clusters = _lib.minhash_near_first_host(sig, heads, min_agree)
    assert np.array_equal(first, want_first) and n_clusters == want_clusters == 16
    assert np.bincount(want_first)[np.unique(want_first)].tolist()[:6] == [1, 2, 3, 5, 8, 13]
    ref = mc.near_first_memo(sig, heads, min_agree)
    assert np.array_equal(ref[0], want_first) and ref[1] == want_clusters
    # heads that are no row before i are not followed
    c = _case("contents", "ids")
    S = len(c["rows"])
    heads = mc.heads_of(mc.band_keys(c["sig"], 32))
    wild, tame = minhash_cases.heads_from_elsewhere(heads)
    me = np.arange(S)[:, None]
    changed = wild != tame
    assert changed.sum() > S * 32 // 4 and ((wild[changed] < 0) | (wild[changed] >= np.broadcast_to(me, wild.shape)[changed])).all()
    assert {int(x) for x in wild[changed]} >= {S, 1 << 40, -1, -(1 << 63)}
    for min_agree in (1, 64):
        want = mc.near_first_memo(c["sig"], tame, min_agree)
        assert np.array_equal(mc.near_first_memo(c["sig"], wild, min_agree)[0], want[0])
        for h in (wild, tame):
            first, n_clusters = _lib.minhash_near_first_host(c["sig"], h, min_agree)
            assert np.array_equal(first, want[0]) and n_clusters == want[1], min_agree
    assert mc.near_first_memo(c["sig"], tame, 1)[1] < S, "some heads are still followed"


def test_value_matches_the_checker():
    rng = np.random.default_rng(11)
    for h in [0, 1, (1 << 64) - 1, 1 << 32, (1 << 32) - 1] + [int(x) for x in rng.integers(0, 1 << 63, 40, dtype=np.uint64)]:
        for k in (0, 1, 63, 64, 1023):
            for seed in SEEDS:
                assert _lib.minhash_value(h, k, seed) == mc.value(h, k, seed), (h, k, seed)
    # a signature extended elsewhere: the minimum with the values of a further shingle
    c = _case("contents", "ids")
    row = c["rows"][3]
    h = mc.shingle_hash(row[:5], 4)
    assert all(_lib.minhash_value(h, k) >= int(c["sig"][3, k]) for k in range(c["n_perm"]))


@pytest.mark.parametrize("kind", minhash_cases.KINDS)
def test_equal_rows_share_a_signature_and_a_cluster(kind):
    for name in ("contents", "short_w5", "extremes"):
        c = _case(name, kind)
        first_eq, _ = dc.first_equal(c["data"], c["offs"])
        assert (first_eq != np.arange(first_eq.size)).any()
        sig = _lib.minhash_host(c["data"], c["offs"], c["width"], c["n_perm"])
        for k, f in enumerate(first_eq):
            assert np.array_equal(sig[k], sig[f])
        for bands in c["bands"]:
            _, heads = _lib.minhash_bands_host(sig, bands)
            for min_agree in (1, c["n_perm"] // 2 + 1, c["n_perm"]):
                first, _ = _lib.minhash_near_first_host(sig, heads, min_agree)
                assert np.array_equal(first[first_eq], first), "every group of equal rows lies inside one cluster"
    # rows that differ only in trailing zeros are different rows with different signatures
    c = _case("contents", kind)
    assert len({c["sig"][i].tobytes() for i in (0, 1, 2)}) == 3


def _pair(rng, n_shared, n_own):
    """two id rows of distinct ids: a shared stretch and a stretch of each one's own, under w = 1 (a shingle is an id)"""
    ids = rng.permutation(60_000)[:n_shared + 2 * n_own].astype(np.uint32)
    a = np.concatenate([ids[:n_shared], ids[n_shared:n_shared + n_own]])
    b = np.concatenate([ids[:n_shared], ids[n_shared + n_own:]])
    return rng.permutation(a), rng.permutation(b)


def test_agreement_estimates_the_jaccard_similarity():
    """K = 1024 over 16 pairs with true J spread over (0, 1]: |agree/K - J| <= 5·sqrt(J(1-J)/K), the binomial standard error
    of K independent trials of probability J times five, and equality at J = 1.  Nothing here is measured on the code."""
    K = 1024
    rng = np.random.default_rng(2024)
    for q in range(16):
        n_own = (0, 2, 5, 10, 20, 35, 50, 70, 90, 120, 160, 220, 300, 450, 700, 1500)[q]
        a, b = _pair(rng, 200, n_own)
        data = np.concatenate([a, b])
        offs = np.asarray([0, a.size, a.size + b.size], np.uint64)
        J = mc.jaccard(tuple(a.tolist()), tuple(b.tolist()), 1)
        assert abs(J - 200 / (200 + 2 * n_own)) < 1e-12
        sig = _lib.minhash_host(data, offs, 1, K, seed=q)
        share = int((sig[0] == sig[1]).sum()) / K
        bound = 5 * math.sqrt(J * (1 - J) / K)
        print(f"pair {q}: J = {J:.4f}, agree/K = {share:.4f}, bound = {bound:.4f}")
        assert abs(share - J) <= bound, (q, J, share, bound)
        if J == 1.0:
            assert share == 1.0


def test_twins_refuse_bad_arguments():
    lib = _lib.lib
    data = np.arange(8, dtype=np.uint8)
    sig = np.full((4, 4), 7, np.uint32)

    def call(offs, n_rows, elem=1, w=2, K=4, d=data, s=sig):
        offs = np.asarray(offs, np.uint64)
        return lib.tgx_minhash_host(_lib.ptr(d) if d is not None else None, elem, _lib.ptr(offs) if offs.size else None, n_rows, w, K, 0,
                                    _lib.ptr(s) if s is not None else None)

    good = [0, 2, 4, 6, 8]
    assert call([1, 2, 4, 6, 8], 4) == _lib.ERR_INVALID and b"offs[0] must be 0" in lib.tgx_last_error()
    assert call([0, 4, 2, 6, 8], 4) == _lib.ERR_INVALID and b"not monotone" in lib.tgx_last_error()
    assert call([], 4) == _lib.ERR_INVALID
    assert call(good, 4, elem=3) == _lib.ERR_INVALID and b"elem_bytes" in lib.tgx_last_error()
    assert call(good, 4, w=0) == _lib.ERR_INVALID and b"width" in lib.tgx_last_error()
    assert call(good, 4, w=65) == _lib.ERR_INVALID
    assert call([0, 0, 1, 1, 2], 4, elem=4, w=17, d=np.arange(2, dtype=np.uint32)) == _lib.ERR_INVALID
    assert call(good, 4, K=0) == _lib.ERR_INVALID and b"n_perm" in lib.tgx_last_error()
    assert call(good, 4, K=1025) == _lib.ERR_INVALID
    assert call(good, 4, d=None) == _lib.ERR_INVALID
    assert call(good, 4, s=None) == _lib.ERR_INVALID
    assert (sig == 7).all()                       # a refused call writes nothing
    assert call(good, 4, w=64) == 0 and not (sig == 7).all()
    assert call([0], 0, d=None, s=None) == 0      # no rows: nothing is looked at
    assert _lib.minhash_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).shape == (0, 128)
    with pytest.raises(TypeError):
        _lib.minhash_host(np.zeros(4, np.uint16), np.asarray([0, 4], np.uint64))
    # rows without elements only: every row has the signature of the empty shingle
    sig0 = _lib.minhash_host(np.zeros(0, np.uint32), np.zeros(6, np.uint64), 5, 64)
    assert np.array_equal(sig0, mc.signatures(np.zeros(0, np.uint32), np.zeros(6, np.uint64), 5, 64)) and (sig0 == sig0[0]).all()

    sig = _lib.minhash_host(data, np.asarray(good, np.uint64), 2, 8)
    keys, heads = np.full((4, 4), 9, np.uint64), np.full((4, 4), -9, np.int64)
    bands_fn, near_fn = lib.tgx_minhash_bands_host, lib.tgx_minhash_near_first_host
    for bands in (0, 3, 16):
        assert bands_fn(_lib.ptr(sig), 4, 8, bands, 0, _lib.ptr(keys), _lib.ptr(heads)) == _lib.ERR_INVALID and b"bands" in lib.tgx_last_error()
    assert bands_fn(_lib.ptr(sig), 4, 8, 4, 0, None, None) == _lib.ERR_INVALID
    assert bands_fn(None, 4, 8, 4, 0, _lib.ptr(keys), _lib.ptr(heads)) == _lib.ERR_INVALID
    assert bands_fn(_lib.ptr(sig), 4, 0, 4, 0, _lib.ptr(keys), _lib.ptr(heads)) == _lib.ERR_INVALID
    assert (keys == 9).all() and (heads == -9).all()
    assert bands_fn(_lib.ptr(sig), 4, 8, 4, 0, _lib.ptr(keys), None) == 0 and (heads == -9).all()
    assert bands_fn(_lib.ptr(sig), 4, 8, 4, 0, None, _lib.ptr(heads)) == 0 and np.array_equal(heads, mc.heads_of(keys))
    first = np.full(4, -7, np.int64)
    nc = C.c_uint64(99)
    for min_agree in (0, 9):
        assert near_fn(_lib.ptr(sig), 4, 8, _lib.ptr(heads), 4, min_agree, _lib.ptr(first), C.byref(nc)) == _lib.ERR_INVALID
        assert b"min_agree" in lib.tgx_last_error()
    assert near_fn(_lib.ptr(sig), 4, 8, None, 4, 1, _lib.ptr(first), C.byref(nc)) == _lib.ERR_INVALID
    assert near_fn(_lib.ptr(sig), 4, 8, _lib.ptr(heads), 4, 1, None, C.byref(nc)) == _lib.ERR_INVALID
    assert near_fn(_lib.ptr(sig), 4, 8, _lib.ptr(heads), 0, 1, _lib.ptr(first), C.byref(nc)) == _lib.ERR_INVALID
    assert first.tolist() == [-7] * 4
    # heads that are no earlier row are never followed
    wild = np.asarray([[5, -1, 99, 1 << 40]] * 4, np.int64)
    assert near_fn(_lib.ptr(sig), 4, 8, _lib.ptr(wild), 4, 1, _lib.ptr(first), None) == 0 and first.tolist() == [0, 1, 2, 3]


def test_stage_names_are_listed_without_a_call():
    assert list(_lib.minhash_last_times()) == STAGES
    for name in ("minhash", "minhash_bands", "near_first", "near_unique_rows"):
        assert getattr(tgx, name) is getattr(tgx.tensors, name)


def test_device_calls_ask_for_a_device_first():
    """NULL handles and pointers: without a device TGX_ERR_DEVICE (there is no host fallback), with one TGX_ERR_INVALID."""
    have_gpu = tgx.device_count() > 0
    lib = _lib.lib
    calls = {
        "tgx_corpus_minhash_device": lambda: lib.tgx_corpus_minhash_device(None, 5, 128, 0, 0, None, None),
        "tgx_result_minhash_device": lambda: lib.tgx_result_minhash_device(None, 5, 128, 0, 0, None, None),
        "tgx_minhash_bands_device": lambda: lib.tgx_minhash_bands_device(0, None, 4, 128, 32, 0, None, None, None),
        "tgx_minhash_near_first_device": lambda: lib.tgx_minhash_near_first_device(0, None, 4, 128, None, 32, 90, None, None, None),
    }
    for name, call in calls.items():
        status = call()
        msg = lib.tgx_last_error() or b""
        if have_gpu:
            assert status == _lib.ERR_INVALID and msg.startswith(name.encode() + b": "), name
        else:
            assert (status, msg) == (_lib.ERR_DEVICE, b"no usable HIP device (gfx950 required)"), name
