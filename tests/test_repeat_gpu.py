"""Repeated n-grams within a row on the GPU (tgx_result_repeat_stats_device, tgx_corpus_repeat_stats_device;
csrc/repeat.hip) against the independent checker (tests/repeat_checker.py: tuples in dicts, no hashing) and the host
twin, on the batches of tests/repeat_cases.py for both kinds and every width (one batch past the cap of the kernels'
grid), written over a sentinel so that every byte of both outputs is seen to be written, with the mask alone, the table
alone and both; then repetition_rows and line_repetition_rows on real text: test_dedup_gpu.py's corpus under the spec
32 000 vocabulary with three planted rows.  Everything is compared exactly: this is integer work."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import dedup_checker as dc
import repeat_cases
import repeat_checker as rc
from gram_cases import V

STAGES = ["repeat_keys_kernel", "repeat_sort", "repeat_runs_kernel", "repeat_cover_kernel"]
SEED = 0xC0FFEE1234567890
PAST = [(kind, w) for kind in repeat_cases.KINDS for w in repeat_cases.widths(kind)]


@functools.lru_cache(maxsize=None)
def _case(name, kind, w):
    """a case with the checker's answer: computed once, never changed"""
    c = repeat_cases.past_cap_case(kind, w) if name == "past_cap" else repeat_cases.case(name, kind, w)
    c["want"] = rc.stats(c["data"], c["offs"], w)
    for a in (c["data"], c["offs"]) + c["want"]:
        a.setflags(write=False)
    return c


def _obj(kind, data, offs):
    return _lib.NativeResult.from_ids(data, offs, V) if kind == "ids" else _lib.NativeCorpus(data, offs)


def _read(obj, kind):
    return (obj.ids(), obj.offsets()) if kind == "ids" else (obj.bytes(), obj.offsets())


def _np(t):
    return t.cpu().numpy()


def _check_case(c, seeds=(0, SEED)):
    import torch
    kind, w = c["kind"], c["width"]
    S, N = len(c["offs"]) - 1, c["data"].size
    want_stats, want_mask = c["want"]
    src = _obj(kind, c["data"], c["offs"])
    try:
        for seed in seeds:
            twin_stats, twin_mask = _lib.repeat_stats_host(c["data"], c["offs"], w, seed)
            assert np.array_equal(twin_stats, want_stats) and np.array_equal(twin_mask, want_mask), seed
            # both, the table alone, the mask alone: each over a sentinel
            for with_stats, with_mask in ((True, True), (True, False), (False, True)):
                if not with_stats and N == 0:
                    continue   # (no element: there is no mask to ask for)
                stats = torch.full((6, S), -7, dtype=torch.int64, device="cuda")
                mask = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
                src.repeat_stats(w, seed, stats.data_ptr() if with_stats else 0, mask.data_ptr() if with_mask and N else 0,
                                 stream=torch.cuda.current_stream().cuda_stream)
                if with_stats:
                    assert np.array_equal(_np(stats), want_stats), (seed, with_mask)
                else:
                    assert (_np(stats) == -7).all()
                if with_mask:
                    assert np.array_equal(_np(mask), want_mask), (seed, with_stats)
                else:
                    assert (_np(mask) == 7).all()
                times = _lib.repeat_last_times()
                assert list(times) == STAGES and all(t >= 0 for t in times.values())
                grams = int(want_stats[0].sum())
                assert times["repeat_keys_kernel"] > 0 and (times["repeat_sort"] > 0) == (times["repeat_runs_kernel"] > 0) == (grams > 0)
                assert (times["repeat_cover_kernel"] > 0) == (with_stats and grams > 0)
        s = tgx.repeat_stats(src, w, SEED, return_mask=True)
        assert s.table.dtype == torch.int64 and s.table.shape == (6, S) and s.table.device.type == "cuda" and s.width == w
        assert s.mask.dtype == torch.uint8 and s.mask.shape == (N,)
        assert np.array_equal(_np(s.table), want_stats) and np.array_equal(_np(s.mask), want_mask)
        assert np.array_equal(_np(s.elems), np.diff(c["offs"].astype(np.int64)))
        for k, name in enumerate(rc.NAMES):
            assert np.array_equal(_np(getattr(s, name)), want_stats[k]), name
        top, cov, cov_all = rc.fracs(want_stats, np.diff(c["offs"].astype(np.int64)), w)
        assert np.array_equal(_np(s.top_frac), top) and np.array_equal(_np(s.covered_frac), cov) and np.array_equal(_np(s.covered_all_frac), cov_all)
        assert np.array_equal(_np(s.repeated_frac), want_stats[1] / np.maximum(want_stats[0], 1))
        assert tgx.repeat_stats(src, w).mask is None
        assert (_np(s.mask)[c["repeat_at"]] & 1).all()
        got = _read(src, kind)
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
    finally:
        src.free()


@pytest.mark.parametrize("name,kind,w", repeat_cases.all_cases())
def test_device_matches_twin_and_checker(name, kind, w):
    _check_case(_case(name, kind, w))


@pytest.mark.parametrize("kind,w", PAST)
def test_past_the_cap(kind, w):
    """2048·256 + 2·256 + 70 elements: a block takes two tiles; one row with repeats goes from a run's first tile into its
    second, one from one block's run into the next, so that two blocks add to one row's sums (tests/test_repeat_cpu.py
    holds the batch to this)"""
    _check_case(_case("past_cap", kind, w), seeds=(SEED,))


@pytest.mark.parametrize("kind", repeat_cases.KINDS)
def test_no_rows_and_no_elements(kind):
    import torch
    dt = repeat_cases.DTYPE[kind]
    nothing = _obj(kind, np.zeros(0, dt), np.zeros(1, np.uint64))
    empties = _obj(kind, np.zeros(0, dt), np.zeros(6, np.uint64))
    try:
        s = tgx.repeat_stats(nothing, 3, return_mask=True)
        assert s.table.shape == (6, 0) and s.mask.shape == (0,) and s.elems.shape == (0,)
        assert tgx.repetition_rows(nothing).shape == (0,)
        stats = torch.full((6, 5), -7, dtype=torch.int64, device="cuda")
        empties.repeat_stats(3, 0, stats.data_ptr(), 0)
        assert not _np(stats).any(), "rows without elements are never visited: the pre-set is their answer"
        assert _np(tgx.repetition_rows(empties)).tolist() == [0, 1, 2, 3, 4]
    finally:
        nothing.free()
        empties.free()


@pytest.mark.parametrize("kind", repeat_cases.KINDS)
def test_bad_arguments_are_refused_before_anything_is_queued(kind):
    import torch
    lib = _lib.lib
    w_max = repeat_cases.W_MAX[kind]
    c = _case("edges_chunk", kind, 5)
    src = _obj(kind, c["data"], c["offs"])
    S, N = src.num_samples, c["data"].size
    call = lib.tgx_result_repeat_stats_device if kind == "ids" else lib.tgx_corpus_repeat_stats_device
    stats = torch.full((6, S), -7, dtype=torch.int64, device="cuda")
    mask = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    h_stats, h_mask = np.full((6, S), 9, np.int64), np.full(N, 9, np.uint8)
    p = lambda t: t.data_ptr()
    try:
        for bad_w in (0, w_max + 1):
            assert call(src._h, bad_w, 0, 0, None, p(stats), p(mask)) == _lib.ERR_INVALID, bad_w
            assert "width" in lib.tgx_last_error().decode()
            with pytest.raises(ValueError):
                tgx.repeat_stats(src, bad_w)
        with pytest.raises(ValueError):
            tgx.repetition_rows(src, top=((2, .2),), dup=((w_max + 1, .1),))
        assert call(src._h, 5, 0, 1, None, p(stats), p(mask)) == _lib.ERR_INVALID                                # flags
        assert call(None, 5, 0, 0, None, p(stats), p(mask)) == _lib.ERR_INVALID
        assert call(src._h, 5, 0, 0, None, None, None) == _lib.ERR_INVALID                                       # no output
        assert call(src._h, 5, 0, 0, None, _lib.ptr(h_stats), p(mask)) == _lib.ERR_INVALID                       # host memory
        assert "not device memory" in lib.tgx_last_error().decode()
        assert call(src._h, 5, 0, 0, None, p(stats), _lib.ptr(h_mask)) == _lib.ERR_INVALID
        if torch.cuda.device_count() >= 2:
            there = torch.full((6, S), -7, dtype=torch.int64, device="cuda:1")
            assert call(src._h, 5, 0, 0, None, p(there), p(mask)) == _lib.ERR_INVALID                            # an output on another device
        torch.cuda.synchronize()
        assert (_np(stats) == -7).all() and (_np(mask) == 7).all() and (h_stats == 9).all() and (h_mask == 9).all()   # nothing was written
        assert call(src._h, w_max, 0, 0, None, p(stats), p(mask)) == 0                                           # the widest is accepted
        want = rc.stats(c["data"], c["offs"], w_max)
        assert np.array_equal(_np(stats), want[0]) and np.array_equal(_np(mask), want[1])
    finally:
        src.free()


def test_on_torchs_current_stream_and_from_another_device():
    import torch
    c = _case("edges_tile", "ids", 5)
    src = _obj("ids", c["data"], c["offs"])
    stream = torch.cuda.Stream(device=0)
    other = 1 if torch.cuda.device_count() >= 2 else 0
    try:
        torch.cuda.synchronize()
        with torch.cuda.device(other):     # the object lives on device 0
            stats = torch.full((6, len(c["offs"]) - 1), -7, dtype=torch.int64, device="cuda:0")
            src.repeat_stats(5, 0, stats.data_ptr(), 0, stream=stream.cuda_stream)
            assert torch.cuda.current_device() == other
            assert np.array_equal(_np(stats), c["want"][0])
        with torch.cuda.stream(stream):    # tensors.* pick up torch's current stream
            s = tgx.repeat_stats(src, 5, return_mask=True)
            keep = tgx.repetition_rows(src)
        assert np.array_equal(_np(s.table), c["want"][0]) and np.array_equal(_np(s.mask), c["want"][1])
        assert np.array_equal(_np(keep), rc.keep_rows(c["data"], c["offs"]))
    finally:
        src.free()


# ---- real text --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], [])


@functools.lru_cache(maxsize=None)
def _texts():
    """test_dedup_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end.  Planted into it: a short row with a slice of about 40
    tokens pasted six times, a row of one token's text 300 times, a row of 30 identical lines."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    texts = [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]
    # the slice: 40 tokens of the longest ordinary row, decoded to their text
    tk = _tokenizer()
    donor = max(rows, key=len)
    donor_corpus = _lib.NativeCorpus(*tgx.pack([donor]))
    res = tk.native_model().encode_corpus(donor_corpus)
    ids = res.ids()
    res.free()
    donor_corpus.free()
    as_result = _lib.NativeResult.from_ids(ids[100:140], np.asarray([0, 40], np.uint64), 32000)
    dec, dec_offs = tk.decode_result_flat(as_result, False)
    as_result.free()
    piece = bytes(np.asarray(dec, np.uint8)[int(dec_offs[0]):int(dec_offs[1])])
    pasted = b"# notes\n" + piece * 6 + b"\nend\n"
    one_token = b" the" * 300
    same_lines = b"    return None\n" * 30
    planted = {5: pasted, len(texts) // 2: one_token, len(texts) - 3: same_lines}
    for at, row in sorted(planted.items(), reverse=True):
        texts.insert(at, row)
    return texts, [texts.index(row) for row in (pasted, one_token, same_lines)]


def test_repetition_filters_on_real_text():
    texts, (r_pasted, r_token, r_lines) = _texts()
    assert max(len(t) for t in texts) == 70_000, "the 70 000-byte row is present"
    S = len(texts)
    flat, offs = tgx.pack(texts)
    nat = _tokenizer().native_model()
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    try:
        ids, id_offs = res.ids(), res.offsets()
        lens = np.diff(id_offs.astype(np.int64))
        print("planted rows: tokens", lens[[r_pasted, r_token, r_lines]].tolist())
        assert lens[r_pasted] >= 100 and lens[r_token] >= 100
        for literal in (False, True):
            keep = _np(tgx.repetition_rows(res, literal=literal))
            want = rc.keep_rows(ids, id_offs, literal=literal)
            assert np.array_equal(keep, want), literal
            assert not {r_pasted, r_token} & set(keep.tolist()), "the two planted n-gram rows are dropped"
            print(f"repetition_rows(literal={literal}): {S - keep.size} of {S} rows dropped")
        s = tgx.repeat_stats(res, 2)
        assert float(s.top_frac[r_token]) > 0.9
        # byte n-grams of the text, at widths the ids could not take
        top, dup = ((20, .2),), ((50, .15), (64, .1))
        keep_b = _np(tgx.repetition_rows(corpus, top=top, dup=dup))
        assert np.array_equal(keep_b, rc.keep_rows(flat, offs, top=top, dup=dup)) and not {r_pasted, r_token, r_lines} & set(keep_b.tolist())
        # duplicate lines
        want_l, want_dl, want_db, want_nl = rc.line_keep_rows(texts)
        keep_l, (dup_lines, dup_bytes, n_lines, n_bytes) = tgx.line_repetition_rows(corpus, return_stats=True)
        assert np.array_equal(_np(dup_lines), want_dl) and np.array_equal(_np(dup_bytes), want_db) and np.array_equal(_np(n_lines), want_nl)
        assert np.array_equal(_np(n_bytes), [len(t) for t in texts])
        assert np.array_equal(_np(keep_l), want_l) and r_lines not in want_l.tolist() and want_dl[r_lines] == 29
        assert np.array_equal(_np(tgx.line_repetition_rows(corpus, 1.0, 1.0)), np.arange(S)), "without limits every row is kept"
        strict = rc.line_keep_rows(texts, 0.0, 0.0)[0]
        assert np.array_equal(_np(tgx.line_repetition_rows(corpus, 0.0, 0.0)), strict) and 0 in strict.tolist(), "an empty row is kept"
        print(f"line_repetition_rows: {S - want_l.size} of {S} rows dropped")
        # select by either keeps corpus and result aligned
        for rows, want_rows in ((tgx.repetition_rows(res), rc.keep_rows(ids, id_offs)), (tgx.line_repetition_rows(corpus), want_l)):
            k_corpus, k_res = tgx.select(corpus, rows), tgx.select(res, rows)
            assert dc.row_bytes(k_corpus.bytes(), k_corpus.offsets()) == [texts[int(k)] for k in want_rows]
            enc = nat.encode_corpus(k_corpus)
            assert np.array_equal(k_res.ids(), enc.ids()) and np.array_equal(k_res.offsets(), enc.offsets())
            for o in (enc, k_res, k_corpus):
                o.free()
    finally:
        res.free()
        corpus.free()
