"""Leftmost-first matches and the mine on the GPU (tgx_corpus_find_device, tgx_corpus_mine_device; csrc/find.hip) against
Python's re on the batch of tests/find_cases.py: matches that end on the last byte of a chunk, of a segment and of a row,
a 64-byte match from byte 63 of a chunk, matches back to back across a segment boundary, rows of length 0 and 1, forty
rows in one chunk, a row longer than a block's span, a row cut at max_len and a last row that ends mid-chunk.  Everything
is compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from find_cases import FLAT, MINE_RS_SAMPLES, OFFS, PATTERNS, mined, pattern, want

STAGES = ["find_walk_kernel", "find_scan", "find_replay_kernel", "find_keys", "find_sort_runs", "find_order"]


@pytest.fixture(scope="module")
def corpus():
    c = _lib.NativeCorpus(FLAT, OFFS)
    yield c
    c.free()


@pytest.mark.parametrize("outputs", [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)], ids=["all", "count", "lens", "truncated"])
@pytest.mark.parametrize("src", PATTERNS)
def test_find_equals_re(corpus, src, outputs):
    """every byte of an asked output is written, over sentinels, and the others are left alone"""
    import torch
    S, N = len(OFFS) - 1, FLAT.size
    bufs = [torch.full((S + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((N + 1,), 7, dtype=torch.uint8, device="cuda"),
            torch.full((S + 1,), -7, dtype=torch.int64, device="cuda")]
    corpus.find(pattern(src), *(b.data_ptr() if on else 0 for b, on in zip(bufs, outputs)))
    torch.cuda.synchronize()
    for buf, on, expect, fill in zip(bufs, outputs, want(src)[:3], (-7, 7, -7)):
        got = buf.cpu().numpy()
        assert np.array_equal(got[:-1], expect) if on else (got[:-1] == fill).all(), (src, outputs)
        assert got[-1] == fill
    times = _lib.find_last_times()
    assert list(times) == STAGES and all(times[s] > 0 for s in STAGES[:3]), times


@pytest.mark.parametrize("src", PATTERNS)
def test_public_calls_equal_re(corpus, src):
    import torch
    want_count, want_lens, want_truncated, want_top = want(src)
    count, lens, truncated = tgx.find_matches(corpus, src, return_lens=True, return_truncated=True)
    assert count.dtype == torch.int64 and count.device.type == "cuda" and lens.dtype == torch.uint8 and truncated.shape == count.shape
    assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(lens.cpu().numpy(), want_lens) and np.array_equal(truncated.cpu().numpy(), want_truncated)
    assert np.array_equal(tgx.find_matches(corpus, pattern(src)).cpu().numpy(), want_count)
    for top in (1, 3, len(want_top) + 5):
        got, n_distinct, n_matches = mined(FLAT, corpus.mine(pattern(src), top))
        assert got == want_top[:top] and n_distinct == len(want_top) and n_matches == want_count.sum(), top
        assert tgx.mine_idioms(corpus, src, top) == want_top[:top]
    assert np.array_equal(corpus.bytes(), FLAT) and np.array_equal(corpus.offsets(), OFFS), "the inputs are only read"


def test_idiom_miner_mirrors_the_reference(corpus):
    miner = tgx.IdiomMiner(2, r"std::\w+")
    assert miner.mine([s.decode() for s in MINE_RS_SAMPLES]) == miner.mine(MINE_RS_SAMPLES) == [(b"std::string", 3), (b"std::vector", 2)]
    assert tgx.IdiomMiner(3, r"std::\w+").mine(corpus) == want(r"std::\w+")[3][:3]
    with pytest.raises(ValueError, match="max_len=64"):
        tgx.IdiomMiner(3, r"\s+").mine(corpus)
    assert tgx.IdiomMiner(3, r"\s+").mine(corpus, allow_truncated=True) == want(r"\s+")[3][:3]
    with pytest.raises(tgx.TokenGeeXError, match="max_len"):
        tgx.find_matches(corpus, "a+", max_len=65)
