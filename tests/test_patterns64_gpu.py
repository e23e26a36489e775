"""Byte patterns of up to 64 states on the GPU (tgx_corpus_dfa64_hits_device; csrc/dfa64.hip) against the host twin and
the header's definition, on the case table of tests/patterns64_cases.py: automata of 3, 7, 17, 21, 33 and 64 states,
matches on the edges of chunks and segments, rows that begin on bytes 0, 1 and 63 of a chunk and in chunks 0 and 63 of
a segment, a match cut by a row boundary, empty rows, no rows and no bytes, one row of 66 000 bytes, every byte value, two
tag bits on one byte, and a corpus in which a wave takes several segments.  Everything is compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from patterns64_cases import CASE_IDS, CASES, PHONE_17, pattern, text, want

STAGES = ["dfa64_map_kernel", "dfa64_scan", "dfa64_replay_kernel", "dfa64_count_kernel"]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_matches_twin_and_reference(case):
    import torch
    pat, (flat, offs), (want_count, want_ends) = pattern(case[0]), text(case), want(case)
    S, N = len(offs) - 1, flat.size
    corpus = _lib.NativeCorpus(flat, offs)
    try:
        twin_count, twin_ends = _lib.dfa64_hits_host(flat, offs, pat)
        assert np.array_equal(twin_count, want_count) and np.array_equal(twin_ends, want_ends)
        # every byte of an output is written and the other is left alone: over sentinels, each alone and both
        for with_count, with_ends in ((True, False), (False, True), (True, True)):
            d_count = torch.full((max(S, 1),), -7, dtype=torch.int64, device="cuda")
            d_ends = torch.full((max(N, 1),), 7, dtype=torch.uint8, device="cuda")
            corpus.dfa64_hits(pat, d_count.data_ptr() if with_count else 0, d_ends.data_ptr() if with_ends else 0)
            assert np.array_equal(_np(d_count)[:S], want_count) if with_count else (_np(d_count) == -7).all(), (with_count, with_ends)
            assert np.array_equal(_np(d_ends)[:N], want_ends) if with_ends else (_np(d_ends) == 7).all(), (with_count, with_ends)
            assert (_np(d_count)[S:] == -7).all() and (_np(d_ends)[N:] == 7).all()
        times = _lib.dfa64_last_times()
        assert list(times) == STAGES and (not N or all(t > 0 for t in times.values())), times
        # the public call: the new kernels above 16 states, and below them the old ones, which answer the same
        count, ends = tgx.pattern_hits(corpus, pat, return_ends=True)
        assert count.dtype == torch.int64 and count.shape == (S,) and count.device.type == "cuda" and ends.dtype == torch.uint8 and ends.shape == (N,)
        assert np.array_equal(_np(count), want_count) and np.array_equal(_np(ends), want_ends)
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), "the inputs are only read"
    finally:
        corpus.free()


def test_bad_arguments_are_refused_before_anything_is_queued():
    import ctypes
    import torch
    flat, offs = text(("ab", "rows"))
    corpus = _lib.NativeCorpus(flat, offs)
    count = torch.full((len(offs) - 1,), -7, dtype=torch.int64, device="cuda")
    ends = torch.full((flat.size,), 7, dtype=torch.uint8, device="cuda")
    h_count = np.full(len(offs) - 1, 9, np.int64)
    hits, good = _lib.lib.tgx_corpus_dfa64_hits_device, _lib.dfa64_struct(pattern("phone17"))
    empty, over = _lib.dfa64_struct(pattern("phone17")), _lib.dfa64_struct(pattern("phone17"))
    empty.tag[empty.start], over.n_states = 1, 65
    try:
        for d in (empty, over):
            assert hits(corpus._h, ctypes.byref(d), count.data_ptr(), ends.data_ptr(), None) == _lib.ERR_INVALID
        assert hits(corpus._h, ctypes.byref(good), None, None, None) == _lib.ERR_INVALID                       # no output
        assert hits(corpus._h, None, count.data_ptr(), ends.data_ptr(), None) == _lib.ERR_INVALID
        assert hits(None, ctypes.byref(good), count.data_ptr(), ends.data_ptr(), None) == _lib.ERR_INVALID
        assert hits(corpus._h, ctypes.byref(good), _lib.ptr(h_count), ends.data_ptr(), None) == _lib.ERR_INVALID  # host memory
        assert "not device memory" in _lib.lib.tgx_last_error().decode()
        torch.cuda.synchronize()
        assert (_np(count) == -7).all() and (_np(ends) == 7).all() and (h_count == 9).all()   # nothing was written
    finally:
        corpus.free()


def test_pattern_rows_and_select_keep_corpus_and_result_aligned():
    from tokengeex_amd import synth
    flat, offs = synth.make_corpus(48 << 10, "mixed", max_len=2048, seed_offset=3)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    phone = tgx.compile_pattern(PHONE_17, max_states=64)
    planted = {2: b"call +12 345 678 9012\n", len(rows) // 2: b"x" * 5000 + b" +49 030 123 4567 ", len(rows) - 1: b"at the end: +31 020 555 0199"}
    for at, row in planted.items():
        rows[at] = row
    flat, offs = tgx.pack(rows)
    want_count, _ = _lib.dfa64_hits_host(flat, offs, phone)
    want_keep = np.flatnonzero(want_count == 0)
    assert set(planted) <= set(np.flatnonzero(want_count).tolist()) and want_keep.size > 0
    toks, scores = synth.build_vocab(flat, 2000, 16)
    nat = tgx.NativeModel(toks, scores, device=0)
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    try:
        keep = tgx.pattern_rows(corpus, phone)
        assert np.array_equal(_np(keep), want_keep)
        k_corpus, k_res = tgx.select(corpus, keep), tgx.select(res, keep)
        assert np.array_equal(k_corpus.bytes(), tgx.pack([rows[int(k)] for k in want_keep])[0])
        enc = nat.encode_corpus(k_corpus)
        assert np.array_equal(k_res.ids(), enc.ids()) and np.array_equal(k_res.offsets(), enc.offsets())
        for o in (enc, k_res, k_corpus):
            o.free()
    finally:
        res.free()
        corpus.free()
