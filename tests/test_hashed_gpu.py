"""Hashed n-gram features on the GPU (tgx_*_hashed_counts_device, tgx_*_hashed_scores_device; csrc/hashed.hip) against
the numpy reference of tests/hashed_cases.py, for ids and text, on its batch of rows at the chunk's edges, on either side
of the LDS threshold, past the grid's cap and at the accumulators' width.  Everything is compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import hashed_cases as hc


def _obj(kind, data, offs):
    return _lib.NativeResult.from_ids(data, offs, 2**31) if kind == "ids" else _lib.NativeCorpus(data, offs)


def _np(t):
    return t.cpu().numpy()


def _check(kind, data, offs, widths, B, q):
    import torch
    counts, scores = hc.reference(data, offs, widths, B, hc.SEED, q)
    src = _obj(kind, data, offs)
    try:
        got = tgx.hashed_counts(src, B, widths, hc.SEED)
        assert got.dtype == torch.int64 and got.shape == (B,) and np.array_equal(_np(got), counts)
        got = tgx.hashed_scores(src, torch.from_numpy(q.copy()), widths, hc.SEED, raw=True)
        assert got.dtype == torch.int64 and got.shape == scores.shape and np.array_equal(_np(got), scores)
        times = _lib.hashed_last_times()
        assert list(times) == ["hashed_counts_kernel", "hashed_scores_kernel"] and all(t > 0 for t in times.values())
    finally:
        src.free()


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 2, 10000, "lds", "lds+1"])
@pytest.mark.parametrize("kind,widths", [("ids", (1,)), ("ids", (1, 2)), ("ids", (2, 3, 5)), ("bytes", (1,)), ("bytes", (1, 2)), ("bytes", (2, 3, 5)),
                                         ("bytes", (3, 50))])
def test_batch_matches_the_reference(kind, widths, B, K):
    if isinstance(B, str):
        B = _lib.hashed_info(K)["lds_max_buckets"] + (B == "lds+1")
    _check(kind, *hc.batch(kind), widths, B, hc.weights(B, K))


@pytest.mark.parametrize("kind", hc.KINDS)
def test_past_the_cap(kind):
    """600 000 elements: past 512 blocks of 16 chunks a wave walks two chunks, so it gallops from its first chunk's
    owner and carries a row over both; the row of 300 000 lies in many waves' runs and every one adds to it"""
    lengths = (5, 300_000) + tuple(int(n) for n in np.random.default_rng(3).integers(0, 200, 2900))
    data, offs = hc.batch(kind, lengths + (600_000 - sum(lengths),), 8)
    _check(kind, data, offs, (1, 2), 10000, hc.weights(10000, 3))


def test_accumulator_width():
    """70 000 equal ids: one bucket takes every add of a width, and the row's score under Q = 2^31 - 1 passes 2^32"""
    data, offs = np.full(70_000, 11, np.uint32), np.asarray([0, 70_000], np.uint64)
    q = np.full((1, 2), 2**31 - 1, np.int32)
    _check("ids", data, offs, (1, 2), 2, q)
    _check("ids", data, offs, (1, 2), 10000, np.full((1, 10000), 2**31 - 1, np.int32))
    assert hc.reference(data, offs, (1, 2), 2, hc.SEED, q)[1][0, 0] == 139_999 * (2**31 - 1) > 2**32


@pytest.mark.parametrize("kind", hc.KINDS)
def test_prefilled_outputs_and_no_rows(kind):
    import torch
    data, offs = hc.batch(kind)
    B, K, widths = 300, 3, (1, 2)
    q = hc.weights(B, K)
    counts, scores = hc.reference(data, offs, widths, B, 0, q)
    src, none = _obj(kind, data, offs), _obj(kind, np.zeros(0, hc.DTYPE[kind]), np.zeros(1, np.uint64))
    try:
        d_q = torch.from_numpy(q.copy()).cuda()
        d_counts = torch.full((B,), -5, dtype=torch.int64, device="cuda")
        d_scores = torch.full(scores.shape, -5, dtype=torch.int64, device="cuda")
        for obj in (none, src):  # S = 0 writes nothing; then every entry is written
            _lib.hashed_counts_device(obj, widths, B, 0, d_counts.data_ptr())
            _lib.hashed_scores_device(obj, widths, B, K, 0, d_q.data_ptr(), d_scores.data_ptr())
            if obj is none:
                assert (_np(d_counts) == -5).all() and (_np(d_scores) == -5).all()
        assert np.array_equal(_np(d_counts), counts) and np.array_equal(_np(d_scores), scores)
        assert not _np(tgx.hashed_counts(none, B)).any() and tgx.hashed_scores(none, d_q).shape == (0, K)
        for bad in ((3, 1), (0,), (65,)):
            with pytest.raises(_lib.TokenGeeXError, match="width"):
                tgx.hashed_counts(src, B, bad)
        assert np.array_equal(_np(d_counts), counts)
    finally:
        src.free()
        none.free()


def test_float_weights_and_dsir():
    import torch
    data, offs = hc.batch("ids")
    B, widths = 1000, (1, 2)
    q = np.random.default_rng(5).integers(-2**20, 2**20, (2, B)).astype(np.int32)
    src = _obj("ids", data, offs)
    try:
        got = tgx.hashed_scores(src, torch.from_numpy(q.astype(np.float64) * 2.0**-24), widths)  # multiples of 2^-24: exact
        assert got.dtype == torch.float64 and np.array_equal(_np(got), hc.reference(data, offs, widths, B, 0, q)[1].astype(np.float64) * 2.0**-24)
        raw = tgx.hashed_counts(src, B, widths)
        assert not _np(tgx.dsir_weights(raw, raw)).any(), "a target equal to the raw source weighs every bucket 0"
        target = torch.roll(raw, 1)
        w = tgx.dsir_weights(target, raw, alpha=0.5)
        assert np.allclose(_np(w), _np(tgx.nb_weights(target, 0.5) - tgx.nb_weights(raw, 0.5))) and abs(float(tgx.nb_weights(raw).exp().sum()) - 1) < 1e-9
        rows = tgx.dsir_rows(src, target, raw, 20, seed=9)
        again, other = tgx.dsir_rows(src, target, raw, 20, seed=9), tgx.dsir_rows(src, target, raw, 20, seed=10)
        assert rows.dtype == torch.int64 and rows.shape == (20,) and bool((rows[1:] > rows[:-1]).all()) and int(rows[-1]) < len(offs) - 1
        assert torch.equal(rows, again) and not torch.equal(rows, other)
        kept = tgx.select(src, rows)
        assert kept.num_samples == 20
        kept.free()
    finally:
        src.free()
