"""Cover and redaction on the GPU (tgx_corpus_dfa_cover_device, tgx_corpus_redact; csrc/cover.hip, csrc/redact.hip)
against the host twins and the header's definitions restated in Python, on the case tables of tests/test_cover_cpu.py:
matches across chunk and tile edges so that both carries are used, rows that end on lanes 0, 62 and 63, a match cut by a
row boundary, the case a one-sided backward pass gets wrong, two patterns on the same bytes, empty rows, one row of
66 001 bytes, a corpus past the cap of the grid, all four pairs of map widths; runs at the edges of rows and chunks,
deleted, 64-byte and missing replacements, and an output that outgrows its input.  Compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from test_cover_cpu import CASE_IDS, CASES, EMAIL, REDACT_CASES, pattern, redact_case, text, want

STAGES = ["cover_summary_kernel", "cover_scan", "cover_kernel", "redact_length_kernel", "redact_scan", "redact_offsets_kernel", "redact_fill_kernel"]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cover_device_matches_twin_and_reference(case):
    import torch
    pat, (flat, offs), (want_covered, want_mask) = pattern(case[0]), text(case[1]), want(case)
    S, N = len(offs) - 1, flat.size
    corpus = _lib.NativeCorpus(flat, offs)
    try:
        covered, mask = tgx.pattern_cover(corpus, pat, return_mask=True)
        assert covered.dtype == torch.int64 and covered.shape == (S,) and covered.device.type == "cuda" and mask.dtype == torch.uint8 and mask.shape == (N,)
        times = _lib.redact_last_times()
        assert list(times) == STAGES and (not N or all(times[k] > 0 for k in STAGES[:3])), times
        twin_covered, twin_mask = _lib.dfa_cover_host(flat, offs, pat)
        assert np.array_equal(_np(covered), want_covered) and np.array_equal(twin_covered, want_covered)
        assert np.array_equal(_np(mask), want_mask) and np.array_equal(twin_mask, want_mask)
        assert np.array_equal(_np(tgx.pattern_cover(corpus, pat)), want_covered)
        # every byte of an output is written and the other is left alone: over sentinels, each alone and both
        for with_covered, with_mask in ((True, False), (False, True), (True, True)):
            d_covered = torch.full((max(S, 1),), -7, dtype=torch.int64, device="cuda")
            d_mask = torch.full((max(N, 1),), 7, dtype=torch.uint8, device="cuda")
            corpus.dfa_cover(pat, d_covered.data_ptr() if with_covered else 0, d_mask.data_ptr() if with_mask else 0)
            assert np.array_equal(_np(d_covered)[:S], want_covered) if with_covered else (_np(d_covered) == -7).all(), (with_covered, with_mask)
            assert np.array_equal(_np(d_mask)[:N], want_mask) if with_mask else (_np(d_mask) == 7).all(), (with_covered, with_mask)
            assert (_np(d_covered)[S:] == -7).all() and (_np(d_mask)[N:] == 7).all()
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), "the inputs are only read"
    finally:
        corpus.free()


@pytest.mark.parametrize("name", list(REDACT_CASES))
def test_redact_device_matches_the_reference(name):
    import torch
    flat, offs, mask, repl, want_text, want_offs = redact_case(name)
    corpus = _lib.NativeCorpus(flat, offs)
    try:
        out = tgx.redact(corpus, torch.from_numpy(mask.copy()).cuda(), repl)
        try:
            assert out.num_samples == len(offs) - 1 and out.num_bytes == want_text.size
            assert np.array_equal(out.offsets(), want_offs) and np.array_equal(out.bytes(), want_text)
        finally:
            out.free()
        times = _lib.redact_last_times()
        assert list(times) == STAGES and (not flat.size or all(times[k] > 0 for k in STAGES[3:6])), times
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), "the input is only read"
    finally:
        corpus.free()


def test_bad_arguments_are_refused_before_anything_is_queued():
    import ctypes
    import torch
    flat, offs = text("row_cut")
    corpus = _lib.NativeCorpus(flat, offs)
    covered = torch.full((len(offs) - 1,), -7, dtype=torch.int64, device="cuda")
    mask = torch.full((flat.size,), 7, dtype=torch.uint8, device="cuda")
    h_mask = np.full(flat.size, 9, np.uint8)
    cover, good, seventeen = _lib.lib.tgx_corpus_dfa_cover_device, _lib.dfa_cover_struct(pattern("ab")), _lib.dfa_cover_struct(pattern("ab"))
    seventeen.bwd.n_states = 17
    try:
        assert cover(corpus._h, ctypes.byref(seventeen), covered.data_ptr(), mask.data_ptr(), None) == _lib.ERR_INVALID
        assert cover(corpus._h, ctypes.byref(good), None, None, None) == _lib.ERR_INVALID                          # no output
        assert cover(corpus._h, None, covered.data_ptr(), mask.data_ptr(), None) == _lib.ERR_INVALID
        assert cover(None, ctypes.byref(good), covered.data_ptr(), mask.data_ptr(), None) == _lib.ERR_INVALID
        assert cover(corpus._h, ctypes.byref(good), covered.data_ptr(), _lib.ptr(h_mask), None) == _lib.ERR_INVALID  # host memory
        assert "not device memory" in _lib.lib.tgx_last_error().decode()
        torch.cuda.synchronize()
        assert (_np(covered) == -7).all() and (_np(mask) == 7).all() and (h_mask == 9).all()   # nothing was written
        redact, x, made = _lib.lib.tgx_corpus_redact, np.frombuffer(b"x" * 65, np.uint8), ctypes.c_void_p(7)
        for roffs, n_repl, flags, d_mask in (([0, 1], 1, 1, mask.data_ptr()), ([0, 1], 0, 0, mask.data_ptr()), (list(range(10)), 9, 0, mask.data_ptr()),
                                             ([0, 65], 1, 0, mask.data_ptr()), ([0, 2, 1], 2, 0, mask.data_ptr()), ([0, 1], 1, 0, None),
                                             ([0, 1], 1, 0, _lib.ptr(h_mask))):
            made.value = 7
            st = redact(corpus._h, d_mask, _lib.ptr(x), _lib.ptr(np.array(roffs, np.uint64)), n_repl, flags, None, ctypes.byref(made))
            assert st == _lib.ERR_INVALID and made.value is None, (roffs, n_repl, flags)
        with pytest.raises(ValueError, match="2 patterns and 1 replacements"):
            tgx.redact_patterns(corpus, ["a", "b"], ["x"])
    finally:
        corpus.free()


def test_redact_patterns_then_encode_equals_the_encode_of_host_redacted_texts():
    import re
    from tokengeex_amd import synth
    flat, offs = synth.make_corpus(48 << 10, "mixed", max_len=2048, seed_offset=3)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    ipv4 = r"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}"
    rows[2], rows[len(rows) // 2], rows[-1] = b"mail ada@example.org\n", b"x" * 3000 + b" bob@mail.example.com from 10.0.12.255 ", b"host 192.168.0.1"
    flat, offs = tgx.pack(rows)
    # matches of the two patterns neither touch nor overlap here, so re.sub's leftmost matches cover the same bytes
    host = [re.sub(ipv4.encode(), b"<IP_ADDRESS>", re.sub(EMAIL.encode(), b"<EMAIL>", row)) for row in rows]
    assert host[2] == b"mail <EMAIL>\n" and host[-1] == b"host <IP_ADDRESS>" and b"<EMAIL> from <IP_ADDRESS> " in host[len(rows) // 2]
    toks, scores, _ = synth.load_spec_vocab(32000)
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], ["<EMAIL>", "<IP_ADDRESS>"])  # the placeholders are special tokens
    want_ids, want_offs = tk.encode_batch_flat(*tgx.pack(host), 0.0)
    corpus = _lib.NativeCorpus(flat, offs)
    red = tgx.redact_patterns(corpus, [EMAIL, ipv4], ["<EMAIL>", "<IP_ADDRESS>"])
    try:
        assert np.array_equal(red.bytes(), tgx.pack(host)[0]) and np.array_equal(red.offsets(), tgx.pack(host)[1])
        res = tk.encode_corpus_result(red)
        assert np.array_equal(res.ids(), want_ids) and np.array_equal(res.offsets(), want_offs) and (want_ids >= tk.base_vocab_size()).sum() >= 4
        res.free()
    finally:
        red.free()
        corpus.free()
