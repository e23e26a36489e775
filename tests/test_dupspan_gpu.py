"""Duplicate spans across rows on the GPU (csrc/dupspan.hip) against the plain checker of tests/dupspan_cases.py and the
host twin: its batches for both kinds, every width and key_bits (4 and 1 force the walk back; one batch lies past the
grid's cap), over sentinels, with the mask alone, the table alone and both; then dup_spans, dedup_spans and span_rows on
test_dedup_gpu.py's corpus with a slice of one row pasted into three later rows.  All integers, compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dedup_checker as dc
import dupspan_cases as dsc
from gram_cases import V


def _obj(kind, data, offs):
    return _lib.NativeResult.from_ids(data, offs, V) if kind == "ids" else _lib.NativeCorpus(data, offs)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name,kind,w", dsc.ALL)
def test_device_matches_twin_and_checker(name, kind, w):
    import torch
    c = dsc.checked_case(name, kind, w)
    S, N = len(c["offs"]) - 1, c["data"].size
    want_table, want_mask = c["want"]
    grams, elems = int(want_table[0].sum()), np.diff(c["offs"].astype(np.int64))
    src = _obj(kind, c["data"], c["offs"])
    try:
        for key_bits in dsc.key_bits_of(N) if S else ():   # (no row: no table to point at; dup_spans below takes that case)
            twin = _lib.dup_spans_host(c["data"], c["offs"], w, key_bits, seed=key_bits)
            assert np.array_equal(twin[0], want_table) and np.array_equal(twin[1], want_mask), key_bits
            for with_table, with_mask in ((True, True), (True, False), (False, True)):   # each over a sentinel
                if not with_table and N == 0:
                    continue   # (no element: there is no mask to ask for)
                table = torch.full((3, S), -7, dtype=torch.int64, device="cuda")
                mask = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
                src.dup_spans(w, key_bits, key_bits, table.data_ptr() if with_table else 0, mask.data_ptr() if with_mask and N else 0,
                              stream=torch.cuda.current_stream().cuda_stream)
                assert np.array_equal(_np(table), want_table) if with_table else (_np(table) == -7).all(), (key_bits, with_mask)
                assert np.array_equal(_np(mask), want_mask) if with_mask else (_np(mask) == 7).all(), (key_bits, with_table)
                times = _lib.dupspan_last_times()
                assert list(times) == dsc.STAGES and times["dupspan_keys_kernel"] > 0
                assert all((times[s] > 0) == (grams > 0) for s in dsc.STAGES[1:]), times
        s = tgx.dup_spans(src, w, seed=5, return_mask=True)
        assert s.table.dtype == torch.int64 and s.table.shape == (3, S) and s.mask.dtype == torch.uint8 and s.mask.shape == (N,) and s.width == w
        assert np.array_equal(_np(s.table), want_table) and np.array_equal(_np(s.mask), want_mask)
        assert np.array_equal(_np(s.elems), elems) and np.array_equal(_np(s.covered_frac), want_table[2] / np.maximum(elems, 1))
        assert np.array_equal(_np(s.grams), want_table[0]) and np.array_equal(_np(s.dup), want_table[1]) and tgx.dup_spans(src, w).mask is None
        got = (src.ids() if kind == "ids" else src.bytes()), src.offsets()
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
    finally:
        src.free()


def test_pasted_spans_on_real_text():
    """test_dedup_gpu.py's corpus (no 50 bytes of it occur twice) with bytes [1000, 1300) of row 13 pasted into rows 19,
    50 (the 70 000-byte row) and 67, at the first place past the middle where the bytes on either side differ from the
    slice's neighbours, so that no match runs on past the paste: the checker confirms exactly the pasted bytes."""
    from test_dedup_gpu import _texts, _tokenizer
    clean, donor, targets, w = list(_texts()), 13, (19, 50, 67), 50
    piece, before, after = clean[donor][1000:1300], clean[donor][999], clean[donor][1300]
    texts, at = list(clean), {}
    for r in targets:
        row = clean[r]
        at[r] = next(p for p in range(len(row) // 2, len(row)) if row[p - 1] != before and row[p] != after)
        texts[r] = row[:at[r]] + piece + row[at[r]:]
    assert len(clean[50]) == 70_000 and len(piece) == 300
    flat, offs = tgx.pack(texts)
    want_table, want_mask = dsc.check(flat, offs, w)
    pasted = np.concatenate([np.arange(int(offs[r]) + at[r], int(offs[r]) + at[r] + 300) for r in targets])
    assert np.array_equal(np.flatnonzero(want_mask & 2), pasted), "the checker: exactly the pasted bytes"
    corpus = _lib.NativeCorpus(flat, offs)
    nat = _tokenizer().native_model()
    res = nat.encode_corpus(corpus)
    try:
        host = np.full((3, len(texts)), 9, np.int64)   # an output in host memory is refused, and nothing is written
        assert _lib.lib.tgx_corpus_dup_spans_device(corpus._h, w, 64, 0, 0, None, _lib.ptr(host), None) == _lib.ERR_INVALID and (host == 9).all()
        s = tgx.dup_spans(corpus, w, return_mask=True)
        assert np.array_equal(_np(s.table), want_table) and np.array_equal(_np(s.mask), want_mask)
        out = tgx.dedup_spans(corpus, w)
        assert dc.row_bytes(out.bytes(), out.offsets()) == clean, "the three rows have lost exactly the pasted bytes"
        out.free()
        assert np.array_equal(_np(tgx.dup_spans(res, 13, key_bits=32).table), dsc.check(res.ids(), res.offsets(), 13)[0])
        rows = tgx.span_rows(corpus, w, 0.05)   # 300 of 70 300 bytes pass, 300 of about 4 000 do not
        keep = [k for k in range(len(texts)) if want_table[2, k] <= 0.05 * len(texts[k])]
        assert _np(rows).tolist() == keep and 50 in keep and 19 not in keep and 67 not in keep
        k_corpus, k_res = tgx.select(corpus, rows), tgx.select(res, rows)
        enc = nat.encode_corpus(k_corpus)
        assert dc.row_bytes(k_corpus.bytes(), k_corpus.offsets()) == [texts[k] for k in keep]
        assert np.array_equal(k_res.ids(), enc.ids()) and np.array_equal(k_res.offsets(), enc.offsets())
        for x in (enc, k_res, k_corpus):
            x.free()
    finally:
        res.free()
        corpus.free()
