"""Fill-in-the-middle without a GPU: the library's uniform (tgx_fim_u01) and host twin (tgx_fim_host, which walks the fill
kernel's tiles and thread slots through csrc/fim.h) against the independent restatement in tests/fim_checker.py.
Everything is compared exactly: this is integer data movement."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import fim_cases
import fim_checker as fc


def _twin(case, **over):
    kw = dict(fim_cases.args(case), **over)
    return _lib.fim_host(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **kw)


def _same(got, want, key):
    for g, w, name in zip(got, want, ("ids", "offsets", "vocab_size", "mode", "cuts", "n_applied")):
        assert np.array_equal(g, w), (key, name)


def test_u01_matches_the_checker():
    big = 2**64 - 1
    triples = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (big, 0, 0), (big, big, 3), (0, big, 2), (1, 2, 3), (12345, 2**40 + 7, 2),
               (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0xA0761D6478BD642F), (big, 2**63, 2**32)]
    rng = np.random.default_rng(0)
    triples += [tuple(int(x) * 2 + 1 for x in rng.integers(0, 2**63, 3)) for _ in range(200)]
    for s, r, d in triples:
        u = _lib.fim_u01(s, r, d)
        assert u == fc.u01(s, r, d) and 0.0 <= u < 1.0, (s, r, d)
    # a salt of its own: neither the dropout hash nor the sampling hash with the same words
    assert _lib.fim_u01(1, 2, 3) != _lib.dropout_u01(1, 2, 3, 0)
    assert fc.SALT != 0xD6E8FEB86659FD93


@pytest.mark.parametrize("part", range(6))
def test_twin_matches_the_checker_on_random_batches(part):
    seen = set()
    for k in range(part, fim_cases.N_BATCHES, 6):
        case = fim_cases.batch(k)
        want = fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case))
        got = _twin(case)
        _same(got, want, k)
        ids, offs, vocab, mode, cuts, n_applied = got
        T2 = int(offs[-1])
        assert T2 == case["want_total"] and (T2 + 3) % 1024 <= 6                # T' at 1024·k - 3 .. 1024·k + 3
        assert T2 == case["ids"].size + 3 * n_applied and n_applied == int((mode != 0).sum())
        assert vocab == max(case["vocab_size"], 1 + max(case["pre"], case["suf"], case["mid"]))
        seen.add(T2 % 4)
        if case["rate"] == 0.0:
            assert np.array_equal(ids, case["ids"]) and np.array_equal(offs, case["offs"]) and not mode.any() and not cuts.any()
        if case["rate"] == 1.0:
            assert np.array_equal(mode != 0, np.diff(case["offs"].astype(np.int64)) > 0)
        if case["rate"] > 0 and case["spm_rate"] in (0.0, 1.0):
            assert set(mode.tolist()) <= {0, 2 if case["spm_rate"] else 1}
        # every output row, undone by its (mode, a, b), is the input row; the sentinels stand where the header says
        sent = (case["pre"], case["suf"], case["mid"])
        for i in range(offs.size - 1):
            row = ids[int(offs[i]):int(offs[i + 1])].tolist()
            src = case["ids"][int(case["offs"][i]):int(case["offs"][i + 1])].tolist()
            m, a, b = int(mode[i]), int(cuts[i, 0]), int(cuts[i, 1])
            assert fc.invert_row(row, m, a, b) == src, (k, i)
            if m == 0:
                assert (a, b) == (0, 0) and row == src
                continue
            n = len(src)
            assert 0 <= a <= b <= n and len(row) == n + 3
            at = (0, a + 1, a + 2 + n - b) if m == 1 else (0, 1, 2 + n - b)
            assert tuple(row[p] for p in at) == sent, (k, i)
            if min(sent) >= case["vocab_size"]:   # the sentinels are no ids of the input: exactly three, in this order
                assert [x for x in row if x in sent] == list(sent), (k, i)
    assert seen == {0, 1, 2, 3}   # tails of the last tile that are and are not whole thread slots


def test_a_row_of_70000_tokens():
    case = fim_cases.long_row()
    _same(_twin(case), fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case)), "long")


def test_a_shard_draws_what_the_whole_batch_draws():
    for k in (5, 40, 101, 160):
        case = fim_cases.batch(k)
        ids, offs, _, mode, cuts, _ = _twin(case)
        S = offs.size - 1
        for cut in (1, S // 2, S - 1, S):
            o = case["offs"]
            shard = dict(case, ids=case["ids"][int(o[cut]):], offs=o[cut:] - o[cut])
            s_ids, s_offs, _, s_mode, s_cuts, _ = _twin(shard, first_row=case["first_row"] + cut)
            assert np.array_equal(s_ids, ids[int(offs[cut]):]) and np.array_equal(s_offs, offs[cut:] - offs[cut]), (k, cut)
            assert np.array_equal(s_mode, mode[cut:]) and np.array_equal(s_cuts, cuts[cut:]), (k, cut)


def test_no_rows_and_one_row():
    got = _lib.fim_host(np.zeros(0, np.uint32), np.zeros(1, np.uint64), 10, 10, 11, 12)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2] == 13 and got[3].size == 0 and got[5] == 0
    for n in (0, 1, 2, 5):
        ids, offs = np.arange(n, dtype=np.uint32), np.array([0, n], np.uint64)
        for seed in range(20):
            got = _lib.fim_host(ids, offs, 10, 20, 11, 12, rate=1.0, spm_rate=0.5, seed=seed)
            _same(got, fc.fim(ids, offs, 10, 20, 11, 12, 1.0, 0.5, seed), (n, seed))
            assert got[2] == 21 and got[5] == (n > 0) and got[0].size == n + 3 * (n > 0)
    # a vocabulary that already holds the sentinels keeps its size
    assert _lib.fim_host(np.array([3], np.uint32), np.array([0, 1], np.uint64), 100, 5, 6, 7)[2] == 100


def test_invalid_arguments_are_refused():
    ids, offs = np.arange(6, dtype=np.uint32), np.array([0, 2, 2, 6], np.uint64)

    def refused(*a, **kw):
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.fim_host(*a, **kw)
        assert e.value.status == _lib.ERR_INVALID, e.value
        return str(e.value)

    for bad in (float("nan"), -0.01, 1.01, float("inf")):
        assert "rate" in refused(ids, offs, 10, 10, 11, 12, rate=bad)
        assert "spm_rate" in refused(ids, offs, 10, 10, 11, 12, spm_rate=bad)
    for sent in ((_lib.NO_ID, 11, 12), (10, _lib.NO_ID, 12), (10, 11, _lib.NO_ID)):
        assert "TGX_NO_ID" in refused(ids, offs, 10, *sent)
    for sent in ((10, 10, 12), (10, 11, 10), (10, 11, 11)):
        assert "distinct" in refused(ids, offs, 10, *sent)
    assert "offs[0]" in refused(ids, np.array([1, 2, 2, 6], np.uint64), 10, 10, 11, 12)
    assert "monotone" in refused(ids, np.array([0, 3, 2, 6], np.uint64), 10, 10, 11, 12)
    assert "room" in refused(ids, offs, 10, 10, 11, 12, rate=1.0, ids_cap=11)      # T' = 6 + 3·2
    assert _lib.fim_host(ids, offs, 10, 10, 11, 12, rate=1.0, ids_cap=12)[0].size == 12
    assert "vocab_size" in refused(ids, offs, 5, 10, 11, 12)                        # id 5 is not below 5
    assert "vocab_size" in refused(ids, offs, 0xFFFFFFFF, 10, 11, 12)
    # NULL arguments, at the ABI itself; the device entry points refuse theirs before they look for a device
    na = C.c_uint64()
    st = _lib.lib.tgx_fim_host(_lib.ptr(ids), _lib.ptr(offs), 3, 10, 10, 11, 12, 1.0, 0.5, 0, 0, None, 0, None, None, None, C.byref(na))
    assert st == _lib.ERR_INVALID
    out_offs = np.zeros(4, np.uint64)
    st = _lib.lib.tgx_fim_host(_lib.ptr(ids), _lib.ptr(offs), 3, 10, 10, 11, 12, 1.0, 0.5, 0, 0, None, 100, _lib.ptr(out_offs), None, None, None)
    assert st == _lib.ERR_INVALID and "out_ids" in _lib.lib.tgx_last_error().decode()
    h = C.c_void_p()
    assert _lib.lib.tgx_result_fim(None, 10, 11, 12, 1.0, 0.5, 0, 0, None, None, None, None, C.byref(h)) == _lib.ERR_INVALID
    for bad_offs, bad_v in ((np.array([1, 2, 2, 6], np.uint64), 10), (np.array([0, 3, 2, 6], np.uint64), 10), (offs, 5), (offs, 0xFFFFFFFF)):
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.NativeResult.from_ids(ids, bad_offs, bad_v)
        assert e.value.status == _lib.ERR_INVALID, e.value


@functools.lru_cache(maxsize=None)
def _statistics_run():
    N = 20_000
    ids = (np.arange(8 * N) % 50).astype(np.uint32)
    offs = (np.arange(N + 1) * 8).astype(np.uint64)
    seed = 2022
    return N, seed, _lib.fim_host(ids, offs, 50, 50, 51, 52, rate=0.5, spm_rate=0.5, seed=seed)


def test_statistics_of_the_draws():
    """Bounds from the binomial distribution, not from what the code gives: a count of N trials of probability p lies
    within 5 sigma = 5·sqrt(N·p·(1 - p)) of N·p except with probability below 1e-6."""
    N, seed, (_, _, _, mode, cuts, n_applied) = _statistics_run()
    assert abs(n_applied - N / 2) <= 5 * math.sqrt(N / 4)
    n_spm = int((mode == 2).sum())
    assert abs(n_spm - n_applied / 2) <= 5 * math.sqrt(n_applied / 4)
    rows = np.flatnonzero(mode != 0)
    c2 = np.array([min(8, int(_lib.fim_u01(seed, int(g), 2) * 9.0)) for g in rows])
    c3 = np.array([min(8, int(_lib.fim_u01(seed, int(g), 3) * 9.0)) for g in rows])
    assert np.array_equal(np.minimum(c2, c3), cuts[rows, 0]) and np.array_equal(np.maximum(c2, c3), cuts[rows, 1])
    sigma = math.sqrt(rows.size * (1 / 9) * (8 / 9))
    counts = np.bincount(c2, minlength=9)
    assert counts.size == 9 and (np.abs(counts - rows.size / 9) <= 5 * sigma).all(), counts
