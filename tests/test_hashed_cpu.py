"""Hashed n-gram features without a device (include/tgx_hashed.h): the host twins, which walk the kernels' chunks, form
the keys of all widths from one window and follow the store / add rule through csrc/hashed.h, against the numpy reference
of tests/hashed_cases.py on its batch; the bucket at its edges; the refusals; the header against the symbol table."""
import os
import re

import numpy as np
import pytest

from tokengeex_amd import _lib, tensors

import hashed_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,K", [(1, 1), (2, 16), (10000, 3), (16385, 1)])
@pytest.mark.parametrize("kind,widths", [("ids", (1,)), ("ids", (1, 2)), ("ids", (2, 3, 5)), ("ids", (1, 4, 15, 16)), ("bytes", (1, 2)),
                                         ("bytes", (2, 3, 5)), ("bytes", (3, 50)), ("bytes", (7, 8, 9, 64))])
def test_twins_match_the_reference(kind, widths, B, K):
    data, offs = hc.batch(kind)
    q = hc.weights(B, K)
    counts, scores = hc.reference(data, offs, widths, B, hc.SEED, q)
    assert counts.sum() == sum(np.maximum(0, np.diff(offs.astype(np.int64)) - w + 1).sum() for w in widths)
    assert np.array_equal(_lib.hashed_counts_host(data, offs, widths, B, hc.SEED), counts)
    assert np.array_equal(_lib.hashed_scores_host(data, offs, widths, q, hc.SEED), scores)


@pytest.mark.parametrize("kind", hc.KINDS)
def test_no_rows_and_no_grams(kind):
    dt = hc.DTYPE[kind]
    assert (_lib.hashed_counts_host(np.zeros(0, dt), np.zeros(1, np.uint64), (1, 2), 5) == -7).all(), "S = 0 writes nothing"
    short = np.arange(3).astype(dt), np.asarray([0, 0, 2, 3, 3], np.uint64)
    assert not _lib.hashed_counts_host(*short, (3, 4), 5).any()
    assert not _lib.hashed_scores_host(*short, (3, 4), hc.weights(5, 2)).any() and not _lib.hashed_scores_host(np.zeros(0, dt), np.zeros(4, np.uint64), (1,), hc.weights(5, 2)).any()


def test_bucket_edges():
    top = 2**64 - 1
    for B in (1, 2, 3, 10000, 2**24):
        assert _lib.hashed_bucket(0, B) == 0 and _lib.hashed_bucket(top, B) == B - 1
        for b in range(1, min(B, 4)):
            first = -(-(b << 64) // B)  # the smallest key of bucket b
            assert _lib.hashed_bucket(first - 1, B) == b - 1 and _lib.hashed_bucket(first, B) == b and _lib.hashed_bucket(first + 1, B) == ((first + 1) * B) >> 64


def test_refusals():
    import torch
    data, offs = hc.batch("ids")
    for widths, B, K, word in (((), 5, 1, "n_widths 0"), ((1, 2, 3, 4, 5), 5, 1, "n_widths 5"), ((0,), 5, 1, "width 0"), ((17,), 5, 1, "width 17"),
                               ((2, 2), 5, 1, "width 2 after width 2"), ((3, 1), 5, 1, "ascend"), ((1,), 0, 1, "buckets 0"),
                               ((1,), 2**24 + 1, 1, "buckets 16777217"), ((1,), 2**20 + 1, 16, "buckets 1048577"), ((1,), 1, 17, "n_vectors 17")):
        with pytest.raises(_lib.TokenGeeXError) as e:
            if K == 1:
                _lib.hashed_counts_host(data, offs, widths, B)
            else:
                _lib.hashed_scores_host(data, offs, widths, np.zeros((K, B), np.int32))
        assert e.value.status == _lib.ERR_INVALID and word in str(e.value), (widths, B, K, str(e.value))
    with pytest.raises(_lib.TokenGeeXError, match="width 65"):
        _lib.hashed_counts_host(*hc.batch("bytes"), (65,), 5)
    for bad in (float("nan"), float("inf"), 128.0, -128.0):
        with pytest.raises(ValueError):
            tensors.quantize_weights(torch.tensor([0.5, bad]))
    q = tensors.quantize_weights(torch.tensor([127.99999994, -127.9999999999, 2.0**-24, 0.0], dtype=torch.float64))
    assert q.dtype == torch.int32 and q.tolist() == [2**31 - 1, -(2**31 - 1), 1, 0]


def test_header_and_symbol_table_agree():
    """every function the header declares is in HASHED_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_hashed.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int|uint64_t) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    assert declared == set(_lib.HASHED_SYMBOLS) and len(declared) == 9 and not declared & set(_lib.SYMBOLS)
    assert all(hasattr(_lib.lib, n) for n in declared)
    import tokengeex_amd as tgx
    assert all(getattr(tgx, n) is getattr(tensors, n) for n in ("hashed_counts", "hashed_scores", "quantize_weights", "nb_weights", "dsir_weights", "dsir_rows"))
    assert _lib.hashed_info(1) == {"lds_max_entries": 16384, "lds_max_buckets": 16384} and _lib.hashed_info(3)["lds_max_buckets"] == 4096
