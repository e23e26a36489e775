"""Shapes on the GPU (tgx_corpus_shape_hits_device, tgx_corpus_shape_cover_device; csrc/shape.hip) against the host twins
and the header's definition in plain Python, on the case table of tests/shape_cases.py: matches that end on lanes 63, 0
and 62 so that the halo is unused, used from its lane 1 and from its lane 63, the tile edge, rows that begin at and one
byte after a match's start, guards across rows, chunks and the corpus's end, the cover's window into the next chunk and
without one, packed patterns that straddle bit 64, and a corpus in which a block takes two tiles.  Compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from shape_cases import AKIA, CASE_IDS, CASES, HEX, HEX32, shapes, text, want

STAGES = ["shape_ends_kernel", "shape_cover_kernel"]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_matches_twin_and_reference(case):
    import torch
    shp, (flat, offs), (want_count, want_ends, want_covered, want_mask) = shapes(case[0]), text(case[1]), want(case)
    S, N = len(offs) - 1, flat.size
    corpus = _lib.NativeCorpus(flat, offs)
    try:
        for fn, method, twin, want_rows, want_bytes, used in ((tgx.shape_hits, corpus.shape_hits, _lib.shape_hits_host, want_count, want_ends, STAGES[:1]),
                                                              (tgx.shape_cover, corpus.shape_cover, _lib.shape_cover_host, want_covered, want_mask, STAGES)):
            rows, byts = fn(corpus, shp, True)
            assert rows.dtype == torch.int64 and rows.shape == (S,) and rows.device.type == "cuda" and byts.dtype == torch.uint8 and byts.shape == (N,)
            times = _lib.shapes_last_times()
            assert list(times) == STAGES and (not N or all(times[k] > 0 for k in used)), times
            twin_rows, twin_bytes = twin(flat, offs, shp)
            assert np.array_equal(_np(rows), want_rows) and np.array_equal(twin_rows, want_rows)
            assert np.array_equal(_np(byts), want_bytes) and np.array_equal(twin_bytes, want_bytes)
            assert np.array_equal(_np(fn(corpus, shp)), want_rows)
            # every byte of an output is written and the other is left alone: over sentinels, each alone and both
            for with_rows, with_bytes in ((True, False), (False, True), (True, True)):
                d_rows = torch.full((max(S, 1),), -7, dtype=torch.int64, device="cuda")
                d_bytes = torch.full((max(N, 1),), 7, dtype=torch.uint8, device="cuda")
                method(shp, d_rows.data_ptr() if with_rows else 0, d_bytes.data_ptr() if with_bytes else 0)
                assert np.array_equal(_np(d_rows)[:S], want_rows) if with_rows else (_np(d_rows) == -7).all(), (with_rows, with_bytes)
                assert np.array_equal(_np(d_bytes)[:N], want_bytes) if with_bytes else (_np(d_bytes) == 7).all(), (with_rows, with_bytes)
                assert (_np(d_rows)[S:] == -7).all() and (_np(d_bytes)[N:] == 7).all()
        assert np.array_equal(_np(tgx.shape_rows(corpus, shp)), np.flatnonzero(want_count == 0))
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), "the inputs are only read"
    finally:
        corpus.free()


def test_bad_arguments_are_refused_before_anything_is_queued():
    import ctypes
    import torch
    flat, offs = text("empties")
    corpus = _lib.NativeCorpus(flat, offs)
    rows = torch.full((len(offs) - 1,), -7, dtype=torch.int64, device="cuda")
    byts = torch.full((flat.size,), 7, dtype=torch.uint8, device="cuda")
    h_rows = np.full(len(offs) - 1, 9, np.int64)
    good, nine, long_len, empty_class = (_lib.shapes_struct(shapes("adjacent")) for _ in range(4))
    nine.n_patterns, long_len.len[0] = 9, 65
    ctypes.memset(empty_class.cls[0], 0, 32)
    try:
        for fn in (_lib.lib.tgx_corpus_shape_hits_device, _lib.lib.tgx_corpus_shape_cover_device):
            for d in (nine, long_len, empty_class):
                assert fn(corpus._h, ctypes.byref(d), rows.data_ptr(), byts.data_ptr(), None) == _lib.ERR_INVALID
            assert fn(corpus._h, ctypes.byref(good), None, None, None) == _lib.ERR_INVALID                        # no output
            assert fn(corpus._h, None, rows.data_ptr(), byts.data_ptr(), None) == _lib.ERR_INVALID
            assert fn(None, ctypes.byref(good), rows.data_ptr(), byts.data_ptr(), None) == _lib.ERR_INVALID
            assert fn(corpus._h, ctypes.byref(good), _lib.ptr(h_rows), byts.data_ptr(), None) == _lib.ERR_INVALID  # host memory
            assert "not device memory" in _lib.lib.tgx_last_error().decode()
        with pytest.raises(ValueError, match="alternation"):
            tgx.shape_hits(corpus, "a|b")
        torch.cuda.synchronize()
        assert (_np(rows) == -7).all() and (_np(byts) == 7).all() and (h_rows == 9).all()   # nothing was written
    finally:
        corpus.free()


def test_redact_with_shapes_then_encode_equals_the_encode_of_host_redacted_texts():
    import re
    from tokengeex_amd import synth
    email = r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}"
    flat, offs = synth.make_corpus(48 << 10, "mixed", max_len=2048, seed_offset=3)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    rows[2], rows[-1] = b"mail ada@example.org key " + HEX32 + b"\n", AKIA + b" is the id, not " + HEX32 + b"0"
    rows[len(rows) // 2] = b"x" * 3000 + b" bob@mail.example.com id=" + AKIA + b" md5 " + HEX32
    flat, offs = tgx.pack(rows)
    # the matches neither overlap nor touch here, so re.sub's leftmost matches cover the same bytes
    host = [re.sub(b"AKIA[0-9A-Z]{16}", b"<KEY>", re.sub(f"(?<!{HEX}){HEX}{{32}}(?!{HEX})".encode(), b"<KEY>", re.sub(email.encode(), b"<EMAIL>", row))) for row in rows]
    assert host[2] == b"mail <EMAIL> key <KEY>\n" and host[-1] == b"<KEY> is the id, not " + HEX32 + b"0" and host[len(rows) // 2].endswith(b" <EMAIL> id=<KEY> md5 <KEY>")
    toks, scores, _ = synth.load_spec_vocab(32000)
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], ["<EMAIL>", "<KEY>"])  # the placeholders are special tokens
    want_ids, want_offs = tk.encode_batch_flat(*tgx.pack(host), 0.0)
    corpus = _lib.NativeCorpus(flat, offs)
    patterns, repl = [email, (HEX + "{32}", HEX, HEX), "AKIA[0-9A-Z]{16}"], ["<EMAIL>", "<KEY>", "<KEY>"]
    try:
        with pytest.raises(ValueError):  # without shapes=True the call is what it was
            tgx.redact_patterns(corpus, patterns[::2], repl[::2])
        red = tgx.redact_patterns(corpus, patterns, repl, shapes=True)
        try:
            assert np.array_equal(red.bytes(), tgx.pack(host)[0]) and np.array_equal(red.offsets(), tgx.pack(host)[1])
            res = tk.encode_corpus_result(red)
            assert np.array_equal(res.ids(), want_ids) and np.array_equal(res.offsets(), want_offs) and (want_ids >= tk.base_vocab_size()).sum() >= 6
            res.free()
        finally:
            red.free()
    finally:
        corpus.free()
