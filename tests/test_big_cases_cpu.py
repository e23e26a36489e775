"""The construction of tests/big_cases.py, without a device: the base's sizes and its rows, the row of each tier that
straddles the tier's boundary, the copies behind it, the sizes of the three sources, the mirrored limits against the
sources of the library, the tiled expectation on small tensors — and, on the base itself, every host twin that
tests/test_past_4gib_gpu.py leans on against its Python checker, and the oracle's encode for the ids."""
import functools
import os
import re
from math import gcd

import numpy as np
import pytest

from oracle import oracle as orc
from tokengeex_amd import _lib, synth, tensors

import big_cases as bc
import dedup_checker
import gram_checker
import minhash_checker
import past_cap
import phrase_checker
import select_checker
import textstat_checker
import wordstat_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle():
    toks, scores, _ = synth.load_spec_vocab(bc.VOCAB)
    return orc.OracleModel(toks, scores), toks


def _encode(text, offs):
    return _oracle()[0].encode_batch_flat(text, offs, 0.0, 0, threads=8)


@functools.lru_cache(maxsize=None)
def _base_ids():
    text, offs = bc.base_corpus()
    ids, id_offs = _encode(text, offs)
    ids.setflags(write=False)
    id_offs.setflags(write=False)
    return ids, id_offs


def test_the_base_has_the_sizes_that_put_the_boundaries_in_the_long_row():
    text, offs = bc.base_corpus()
    ids, id_offs = _base_ids()
    assert text.size == bc.N0 == int(offs[-1]) and 256 << 10 <= bc.N0 <= 2 << 20 and gcd(bc.N0, 4096) == 1
    assert ids.size == bc.T0 == int(id_offs[-1]) and gcd(bc.T0, 4096) == 1, "the vocabulary covers the text, to T0 ids"
    assert int(ids.max()) < bc.VOCAB and np.array_equal(offs[[0, -1]], [0, bc.N0])
    long_row = bc.long_row_index()
    for limit, base_offs, R in ((bc.LIMIT_A, offs, 4160), (bc.LIMIT_B, id_offs, 4160), (bc.LIMIT_C, id_offs, 16448)):
        n0, s0 = int(base_offs[-1]), base_offs.size - 1
        copy, row, begin, end = bc.straddling_row(base_offs, limit)
        assert row == long_row and begin < limit < end, (limit, copy, row, begin, end)
        assert bc.copies(n0, limit) == R
        assert (R - bc.SPARE) * n0 >= limit > (R - bc.SPARE - 1) * n0, "SPARE whole copies begin at or after the limit, and no more"
        rows = bc.big_rows(n0, s0, limit)
        assert rows.dtype == np.int64 and rows.size == R * s0 < 2**31 and np.array_equal(rows[:s0], np.arange(s0)) and np.array_equal(rows[-s0:], rows[:s0])
        big = bc.big_offsets(base_offs, R)
        assert big.size == R * s0 + 1 and int(big[-1]) == R * n0 and int(big[copy * s0 + row]) == begin and int(big[copy * s0 + row + 1]) == end
        assert int(np.diff(big.astype(np.int64)).max()) < 2**31
        want = np.concatenate([[0], np.cumsum(np.tile(np.diff(base_offs.astype(np.int64)), 3))]).astype(np.uint64)
        assert np.array_equal(bc.big_offsets(base_offs, 3), want)


def test_tier_c_has_more_than_2_pow_32_shingles_at_width_1_only():
    ids, id_offs = _base_ids()
    rc = bc.copies(bc.T0, bc.LIMIT_C)
    assert bc.MINHASH_WIDTHS == (bc.MINHASH_WIDTH, 1)
    assert bc.shingles(id_offs, 1, rc) > 2**32 > bc.shingles(id_offs, bc.MINHASH_WIDTH, rc)
    assert bc.shingles(id_offs, 1) == minhash_checker_positions(id_offs, 1)


def minhash_checker_positions(offs, w):
    return sum(len(minhash_checker.shingles(range(int(n)), w)) for n in np.diff(offs.astype(np.int64)))


def test_the_exact_sizes_of_the_three_sources():
    s0 = bc.base_corpus()[1].size - 1
    assert bc.tier_sizes(s0) == {"A": (4160, 4160 * s0, 4_362_080_320, 4_362_080_320),
                                 "B": (4160, 4160 * s0, 1_090_523_200, 4_362_092_800),
                                 "C": (16448, 16448 * s0, 4_311_760_960, 17_247_043_840)}
    for tier, (R, rows, elems, nbytes) in bc.tier_sizes(s0).items():
        assert rows < 2**31 and nbytes > 2**32 and (tier != "C" or elems > 2**32)
    need = bc.tier_c_needs(s0, 4)
    assert 2 * 17_247_043_840 < need < 2 * 17_247_043_840 + 2 * 16 * 16448 * s0 + (1 << 20)


def test_the_selection_without_the_long_row_still_straddles():
    ids, id_offs = _base_ids()
    keep, t, R = bc.short_selection(id_offs)
    n = np.diff(id_offs.astype(np.int64))
    assert keep.size == n.size - 1 and bc.long_row_index() not in keep and t == bc.T0 - int(n.max()) and R == bc.copies(t, bc.LIMIT_B)
    offs = _lib.select_host(ids, id_offs, keep)[1]
    copy, row, begin, end = bc.straddling_row(offs, bc.LIMIT_B)
    assert begin < bc.LIMIT_B < end and copy + bc.SPARE < R and R > bc.copies(bc.T0, bc.LIMIT_B)
    assert R * keep.size * bc.PAD_LEN > 2**32 and R * keep.size < bc.LAYOUT_REFUSED_ROWS, "the padded ids are more than 2^32 elements"
    assert 0 < (n[keep] > bc.PAD_LEN).sum() < keep.size, "some rows are truncated at PAD_LEN, and become several windows"
    whole = bc.base_corpus()[0].tobytes()
    assert all(s in whole for s in bc.SPECIALS) and 300 < sum(whole.count(s) for s in bc.SPECIALS) < 3000


def test_the_rows_the_base_holds():
    text, offs = bc.base_corpus()
    rows = bc.base_rows()
    n = np.diff(offs.astype(np.int64))
    assert n[0] == 0 and n[-1] == 0 and n.max() >= 70_000 and (n >= 70_000).sum() == 1
    pattern = list(past_cap.PATTERN)
    assert n[1:13].tolist() == pattern * 2 and n[-9:-3].tolist() == pattern, "rows of 0 and 1 bytes first and last"
    runs = "".join("0" if k == 0 else "x" for k in n)
    assert "00000" in runs[13:-9], "a run of empty rows in the middle"
    whole = text.tobytes()
    chars = whole.decode("utf-8")       # valid UTF-8 throughout
    widths = {len(c.encode()) for c in set(chars)}
    assert widths == {1, 2, 3, 4}
    assert b"\r\n" in whole and b"\r" in whole.replace(b"\r\n", b"")
    lines = np.array([len(l) for r in rows for l in r.split(b"\n")])
    assert {1, 63, 64, 65, 255, 256, 257, 1000, 1001, 4097} <= set(lines.tolist())
    low = whole.lower()
    assert bc.PHRASES[:5] == tuple(p.encode() for p in tensors.AUTOGENERATED) and all(p in low for p in bc.PHRASES) and all(b" " + w + b" " in whole for w in _lib.GOPHER_STOP_WORDS)
    assert _lib.normalize_flat("nfc", text, offs)[0].size != text.size and _lib.normalize_flat("nfkc", text, offs)[0].size != text.size


def test_the_fitted_constants():
    """fit() on this machine gives the constants that big_cases.py carries: the base is what the docstring says it is"""
    oracle, toks = _oracle()
    assert bc.fit(_encode, toks) == (bc.K_PROSE, bc.K_HEAVY, bc.A16, bc.R_TOKEN, bc.B1)
    assert len(bc.HEAVY_TOKEN) == 16 and _encode(*bc._pack([bc.HEAVY_TOKEN]))[0].size == 1


def _constant(path, pattern):
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        found = re.findall(pattern, f.read())
    assert found, (path, pattern)
    return found


def test_the_mirrored_limits_are_the_librarys():
    csrc = "tokengeex_amd/csrc/"
    assert [int(v, 16) for v in _constant(csrc + "repeat.h", r"kRepeatMaxElems = (0x[0-9A-Fa-f]+)ull")] == [bc.REPEAT_MAX_ELEMS]
    assert _constant(csrc + "repeat_ops.cpp", r"if \(N > tgx::kRepeatMaxElems\) return fail\(TGX_ERR_UNSUPPORTED")
    freq = _constant(csrc + "tgx_api.cpp", r"if \(T >= (0x[0-9A-Fa-f]+)ull\) return fail\(TGX_ERR_UNSUPPORTED, \"frequency pass")
    pairs = _constant(csrc + "tgx_api.cpp", r"if \(T >= (0x[0-9A-Fa-f]+)ull\) return fail\(TGX_ERR_UNSUPPORTED, \"pair scan")
    assert [int(v, 16) for v in freq] == [bc.FREQ_REFUSED_TOKENS] and [int(v, 16) for v in pairs] == [bc.PAIRS_REFUSED_TOKENS]
    shuffle = _constant(csrc + "result_ops.cpp", r"if \(n >= (0x[0-9A-Fa-f]+)ull\) return fail\(TGX_ERR_UNSUPPORTED, \"%s: 2\^31 rows or more\"")
    layout = _constant(csrc + "result_ops.cpp", r"if \(r->n_samples >= (0x[0-9A-Fa-f]+)ull\) return fail\(TGX_ERR_UNSUPPORTED, \"%s: 2\^31 rows or more\"")
    assert [int(v, 16) for v in shuffle] == [bc.SHUFFLE_REFUSED_ROWS] and [int(v, 16) for v in layout] == [bc.LAYOUT_REFUSED_ROWS]
    # the tiers stand on the right side of each
    sizes = bc.tier_sizes(bc.base_corpus()[1].size - 1)
    assert sizes["A"][2] > bc.REPEAT_MAX_ELEMS and sizes["C"][2] > bc.REPEAT_MAX_ELEMS and sizes["B"][2] <= bc.REPEAT_MAX_ELEMS
    assert sizes["A"][2] >= bc.FREQ_REFUSED_TOKENS, "a model of single bytes gives Tier A one token per byte: refused"
    assert sizes["A"][0] * bc.T0 < bc.FREQ_REFUSED_TOKENS, "the spec vocabulary's tokens of Tier A are counted"
    assert all(s[1] < bc.LAYOUT_REFUSED_ROWS for s in sizes.values())
    assert _lib.lib.tgx_shuffled_rows_host(bc.SHUFFLE_REFUSED_ROWS, 1, None) == _lib.ERR_UNSUPPORTED      # refused before rows is looked at


def test_the_tiled_expectation_finds_one_wrong_entry():
    import torch
    rng = np.random.default_rng(3)
    for shape, axis, R in (((7,), 0, 130), ((11, 5), 1, 67), ((5, 4), 0, 65), ((6,), -1, 1)):
        base = rng.integers(0, 1 << 40, shape).astype(np.int64)
        for step in (0, 1000):
            e = bc.expect_rows(base, R, axis, step)
            want = e.numpy()
            assert want.shape[axis] == R * shape[axis]
            e.check(torch.from_numpy(want.copy()))
            for at in (0, want.size // 2, want.size - 1):      # the first slab, one in the middle, the last
                bad = want.copy()
                bad.reshape(-1)[at] ^= 1
                with pytest.raises(AssertionError):
                    e.check(torch.from_numpy(bad))
        with pytest.raises(AssertionError):
            bc.expect_rows(base, R + 1, axis).check(torch.from_numpy(bc.expect_rows(base, R, axis).numpy()))
    u = rng.integers(0, 1 << 63, 9).astype(np.uint64) * np.uint64(2) + np.uint64(1)    # u64 bits in an int64 tensor
    bc.expect_elems(u, 70).check(torch.from_numpy(np.tile(u, 70).view(np.int64)))
    u32 = rng.integers(1 << 31, 1 << 32, (4, 3)).astype(np.uint32)
    bc.expect_rows(u32, 70, 0).check(torch.from_numpy(np.tile(u32, (70, 1)).view(np.int32)))
    assert np.array_equal(bc.strided_mask(7), [True, False, False, True, False, False, True])


# ---- the host twins on the base, against their checkers: the GPU file leans on the twins alone ---------------------------

def test_text_stats_and_lines_twins_equal_the_checker_on_the_base():
    text, offs = bc.base_corpus()
    for unit in ("char", "byte"):
        stats, starts = _lib.text_stats_host(text, offs, 1000, unit)
        want, want_starts = textstat_checker.stats_of(text, offs, 1000, unit)
        assert np.array_equal(stats, want) and np.array_equal(starts, want_starts), unit
    assert np.array_equal(_lib.lines_host(text, offs), textstat_checker.lines_of(text, offs)[0])


def test_word_stats_twin_equals_the_checker_on_the_base():
    text, offs = bc.base_corpus()
    stats, marks = _lib.word_stats_host(text, offs, 20, _lib.GOPHER_STOP_WORDS, "char", True)
    want, want_marks = wordstat_checker.stats_of(text, offs, 20, _lib.GOPHER_STOP_WORDS, "char", True)
    assert np.array_equal(stats, want) and np.array_equal(marks, want_marks)
    assert int(stats[_lib.WORDSTAT_NAMES.index("stop_words")].sum()) > 20


def test_phrase_hits_twin_equals_the_checker_on_the_base():
    text, offs = bc.base_corpus()
    ids, id_offs = _base_ids()
    for fold_case, whole_word in ((True, False), (False, True)):
        got = _lib.phrase_hits_host(text, offs, bc.PHRASES, fold_case, whole_word)
        want = phrase_checker.hits_of(text, offs, bc.PHRASES, fold_case, whole_word)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and int(want[2].sum()) >= 5
    phrases = bc.id_phrases(ids, id_offs)
    got = _lib.phrase_hits_host(ids, id_offs, phrases)
    want = phrase_checker.hits_of(ids, id_offs, phrases)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and (want[2] > 0).all()


@pytest.mark.parametrize("kind", ["bytes", "ids"])
def test_gram_minhash_and_first_equal_twins_equal_the_checkers_on_the_base(kind):
    data, offs = bc.base_corpus() if kind == "bytes" else _base_ids()
    w = bc.GRAM_WIDTH[kind]
    held = bc.held_out(data, offs)
    keys = _lib.gram_keys_host(*held, w, 0)
    assert np.array_equal(keys, gram_checker.keys_of(*held, w, 0))
    count, mask = _lib.gram_hits_host(data, offs, w, 0, keys)
    want_count, want_mask = gram_checker.hits(data, offs, w, 0, keys)
    assert np.array_equal(count, want_count) and np.array_equal(mask, want_mask) and 0 < int(mask.sum()) < mask.size
    for width in bc.MINHASH_WIDTHS:
        sig = _lib.minhash_host(data, offs, width, bc.N_PERM, 0)
        assert np.array_equal(sig, minhash_checker.signatures(data, offs, width, bc.N_PERM, 0)), width
    first, n_unique, _ = _lib.first_equal_host(data, offs)
    want_first, want_unique = dedup_checker.first_equal(data, offs)
    assert np.array_equal(first, want_first) and n_unique == want_unique < first.size


@pytest.mark.parametrize("kind", ["bytes", "ids"])
def test_select_twin_equals_the_checker_on_the_base(kind):
    data, offs = bc.base_corpus() if kind == "bytes" else _base_ids()
    twin = _lib.select_text_host if kind == "bytes" else _lib.select_host
    s0 = offs.size - 1
    for rows in (np.flatnonzero(bc.strided_mask(s0)), np.tile(np.arange(s0), 3)):
        got, got_offs = twin(data, offs, rows)
        want, want_offs = select_checker.select(data, offs, rows)
        assert np.array_equal(got, want) and np.array_equal(got_offs, want_offs)
    assert np.array_equal(twin(data, offs, np.tile(np.arange(s0), 3))[1], bc.big_offsets(offs, 3))
