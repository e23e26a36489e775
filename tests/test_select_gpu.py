"""Row selection on the GPU (tgx_result_select, tgx_corpus_select, tgx_result_lengths_device, tgx_shuffled_rows_device;
csrc/select.hip) against the host twins and the independent checker (tests/select_checker.py), through the host-index and
the device-index path; a selected corpus and a selected result stay aligned on real text; the layouts and the decode of a
selected result against the host route over the checker's output.  Everything is compared exactly: this is integer data
movement.

The shapes are tests/select_cases.py's (rows around a slot and around one and four tiles, runs of empty rows, T' one to
three positions on either side of a tile, six index patterns) and one row of 70 000 elements selected three times; the
real text is test_assemble_gpu.py's corpus, 96 KiB of mixed text with a 70 000-byte sample and empty samples, under the
spec 32 000 vocabulary."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import layout_checker as lc
import past_cap
import select_cases
import select_checker as sc

TWIN = {"ids": _lib.select_host, "bytes": _lib.select_text_host}


def _source(case, kind):
    if kind == "ids":
        return _lib.NativeResult.from_ids(case["data"], case["offs"], case["vocab_size"])
    return _lib.NativeCorpus(case["data"], case["offs"])


def _read(obj, kind):
    return (obj.ids(), obj.offsets()) if kind == "ids" else (obj.bytes(), obj.offsets())


def _same(got, want, key):
    assert got[0].dtype == want[0].dtype, key
    assert np.array_equal(got[1], want[1]), (key, "offsets")
    assert np.array_equal(got[0], want[0]), (key, "data")


def _check_case(case, kind, key):
    import torch
    want = sc.select(case["data"], case["offs"], case["rows"])
    _same(TWIN[kind](case["data"], case["offs"], case["rows"]), want, (key, "twin"))
    src = _source(case, kind)
    try:
        d_rows = torch.from_numpy(case["rows"]).cuda()
        for name, rows in (("host", case["rows"]), ("device", d_rows)):
            out = src.select(rows)
            try:
                _same(_read(out, kind), want, (key, kind, name))
                assert out.num_samples == case["rows"].size
                if kind == "ids":
                    assert out.vocab_size == src.vocab_size and out.device == src.device and out.num_tokens == case["want_total"]
                else:
                    assert out.num_bytes == case["want_total"]
            finally:
                out.free()
        _same(_read(src, kind), (case["data"], case["offs"]), (key, "the input is only read"))
        assert np.array_equal(d_rows.cpu().numpy(), case["rows"])
    finally:
        src.free()


@pytest.mark.parametrize("part", range(6))
def test_device_matches_twin_and_checker_on_the_shapes(part):
    for kind in ("ids", "bytes"):
        for k in range(part, select_cases.N_BATCHES, 6):
            _check_case(select_cases.batch(k, kind), kind, k)


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_a_row_of_70000_elements_selected_three_times(kind):
    _check_case(select_cases.long_row(kind), kind, "long")


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_nothing_selected_and_nothing_to_select_from(kind):
    import torch
    dt = np.uint32 if kind == "ids" else np.uint8
    for data, offs in ((np.arange(7, dtype=dt), np.array([0, 3, 3, 7], np.uint64)), (np.zeros(0, dt), np.zeros(1, np.uint64))):
        src = _source(dict(data=data, offs=offs, vocab_size=10), kind)
        for rows in ([], np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int64, device="cuda"), np.zeros(offs.size - 1, bool)):
            out = src.select(rows)
            got = _read(out, kind)
            assert out.num_samples == 0 and got[0].size == 0 and got[1].tolist() == [0]
            out.free()
        src.free()


def test_a_stream_of_the_caller_and_stream_0():
    import torch
    case = select_cases.batch(5, "ids")
    want = sc.select(case["data"], case["offs"], case["rows"])
    text = select_cases.batch(5, "bytes")
    want_text = sc.select(text["data"], text["offs"], text["rows"])
    res, corpus = _source(case, "ids"), _source(text, "bytes")
    stream = torch.cuda.Stream(device=res.device)
    for st in (0, stream.cuda_stream):
        for rows, trows in ((case["rows"], text["rows"]), (torch.from_numpy(case["rows"]).cuda(), torch.from_numpy(text["rows"]).cuda())):
            torch.cuda.synchronize()
            out = res.select(rows, stream=st)
            _same(_read(out, "ids"), want, st)
            out.free()
            out = corpus.select(trows, stream=st)
            _same(_read(out, "bytes"), want_text, st)
            out.free()
    with torch.cuda.stream(stream):   # the device path picks up torch's current stream
        rows = torch.from_numpy(case["rows"]).cuda()
        out = res.select(rows)
    _same(_read(out, "ids"), want, "current stream")
    out.free()
    res.free()
    corpus.free()


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_invalid_arguments_are_refused_on_both_index_paths(kind):
    import torch
    dt = np.uint32 if kind == "ids" else np.uint8
    data, offs = np.arange(10, dtype=dt), np.array([0, 3, 3, 10], np.uint64)
    src = _source(dict(data=data, offs=offs, vocab_size=10), kind)
    empty = _source(dict(data=np.zeros(0, dt), offs=np.zeros(1, np.uint64), vocab_size=10), kind)
    fn = _lib.lib.tgx_result_select if kind == "ids" else _lib.lib.tgx_corpus_select

    def refused(obj, rows):
        with pytest.raises(tgx.TokenGeeXError) as e:
            obj.select(rows)
        assert e.value.status == _lib.ERR_INVALID, e.value
        return str(e.value)

    for dev in (False, True):
        mk = (lambda r: torch.tensor(r, dtype=torch.int64, device="cuda")) if dev else (lambda r: np.asarray(r, np.int64))
        assert "rows[0] = 0 is not a row of 0" in refused(empty, mk([0]))               # S = 0 with M = 1
        assert "rows[2] = -1 " in refused(src, mk([0, 1, -1, 7, -3]))                   # the smallest bad k
        assert "rows[1] = 3 " in refused(src, mk([2, 3, 1]))                            # index = S
        assert "rows[3] = 4611686018427387904 " in refused(src, mk([0, 1, 2, 2**62]))
        many = np.zeros(5000, np.int64)                                                 # more than one block of the check
        many[[4097, 4999]] = (3, -1)
        assert "rows[4097] = 3 " in refused(src, mk(many))
        out = src.select(mk([2, 0]))   # and the stage still works
        assert _read(out, kind)[0].tolist() == list(range(3, 10)) + [0, 1, 2]
        out.free()
    # the device flag with a host pointer; unknown flags; NULL arguments
    rows = np.array([0, 1], np.int64)
    h = C.c_void_p(1)
    assert fn(src._h, _lib.ptr(rows), 2, _lib.SELECT_ROWS_DEVICE, None, C.byref(h)) == _lib.ERR_INVALID and not h.value
    assert "device memory" in _lib.lib.tgx_last_error().decode()
    assert fn(src._h, _lib.ptr(rows), 2, 2, None, C.byref(h)) == _lib.ERR_INVALID
    assert fn(None, _lib.ptr(rows), 2, 0, None, C.byref(h)) == _lib.ERR_INVALID
    assert fn(src._h, None, 2, 0, None, C.byref(h)) == _lib.ERR_INVALID
    assert fn(src._h, _lib.ptr(rows), 2, 0, None, None) == _lib.ERR_INVALID
    if kind == "ids":
        assert _lib.lib.tgx_result_lengths_device(None, None, None) == _lib.ERR_INVALID
        assert _lib.lib.tgx_result_lengths_device(src._h, None, None) == _lib.ERR_INVALID
        assert _lib.lib.tgx_result_lengths_device(src._h, None, _lib.ptr(np.zeros(3, np.int64))) == _lib.ERR_INVALID   # host memory
        assert _lib.lib.tgx_shuffled_rows_device(0, 4, 1, None, _lib.ptr(np.zeros(4, np.int64))) == _lib.ERR_INVALID
        assert _lib.lib.tgx_shuffled_rows_device(0, 4, 1, None, None) == _lib.ERR_INVALID
        assert _lib.lib.tgx_shuffled_rows_device(-1, 4, 1, None, None) == _lib.ERR_INVALID
        assert _lib.lib.tgx_shuffled_rows_device(0, 2**31, 1, None, None) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        src.select(torch.zeros(2, dtype=torch.bool, device="cuda"))   # a mask of another length
    if torch.cuda.device_count() >= 2:
        with pytest.raises(ValueError):
            src.select(torch.zeros(2, dtype=torch.int64, device="cuda:1"))
    out = src.select(rows)   # and the stage still works
    assert out.num_samples == 2
    out.free()
    src.free()
    empty.free()


def test_selecting_twice_is_selecting_through_the_composed_index():
    import torch
    case = select_cases.batch(3, "ids")   # one row repeated: M > S
    S = case["offs"].size - 1
    rng = np.random.default_rng(3)
    a = rng.integers(0, S, 2 * S).astype(np.int64)
    b = rng.integers(0, a.size, 3 * S).astype(np.int64)
    src = _source(case, "ids")
    first = src.select(torch.from_numpy(a).cuda())
    twice, once = first.select(b), src.select(a[b])
    _same(_read(twice, "ids"), _read(once, "ids"), "composition")
    _same(_read(once, "ids"), sc.select(case["data"], case["offs"], a[b]), "checker")
    for r in (first, twice, once, src):
        r.free()


# ---- real text: a selected corpus and a selected result stay aligned --------------------------------------------------

@functools.lru_cache(maxsize=None)
def _texts():
    """test_assemble_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    return [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], [])


@functools.lru_cache(maxsize=None)
def _encoded():
    """-> (the packed text, the ids and offsets of its encode); computed once, never changed"""
    flat, offs = tgx.pack(_texts())
    nat = _tokenizer().native_model()
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    ids, oo = res.ids(), res.offsets()
    res.free()
    corpus.free()
    n = np.diff(oo.astype(np.int64))
    assert n.max() > 16 * 1024 and n[0] == n[1] == n[-1] == 0 and (n == 0).sum() >= 6
    return (flat, offs), (ids, oo)


def _index_forms(offs):
    lens = np.diff(offs.astype(np.int64))
    S, long_row = lens.size, int(np.argmax(lens))
    rng = np.random.default_rng(11)
    mask = rng.random(S) < 0.5
    mask[[0, long_row]] = True     # an empty sample and the long one
    multi = rng.integers(0, S, S + S // 2).astype(np.int64)
    multi[[3, 40, 41]] = (long_row, S - 1, long_row)
    return {"reversal": np.arange(S, dtype=np.int64)[::-1].copy(), "subset mask": mask, "multiset": multi}


@pytest.mark.parametrize("form", ["reversal", "subset mask", "multiset"])
def test_corpus_and_result_stay_aligned_on_real_text(form):
    import torch
    (flat, offs), (ids, oo) = _encoded()
    nat = _tokenizer().native_model()
    S = offs.size - 1
    rows = _index_forms(offs)[form]
    idx = np.flatnonzero(rows) if rows.dtype == bool else rows
    lens = np.diff(offs.astype(np.int64))
    assert lens[idx].max() == 70_000 and (lens[idx] == 0).any()
    want_ids, want_offs = sc.select(ids, oo, idx)
    corpus = _lib.NativeCorpus(flat, offs)
    whole = nat.encode_corpus(corpus)
    for dev in (False, True):
        r = torch.from_numpy(rows).cuda() if dev else rows
        sel_corpus = tgx.select(corpus, r)
        _same((sel_corpus.bytes(), sel_corpus.offsets()), sc.select(flat, offs, idx), (form, dev, "text"))
        sel_res = tgx.select(whole, r)
        _same((sel_res.ids(), sel_res.offsets()), (want_ids, want_offs), (form, dev, "select of the encode"))
        enc = nat.encode_corpus(sel_corpus)
        _same((enc.ids(), enc.offsets()), (want_ids, want_offs), (form, dev, "encode of the select"))
        counts = nat.count_tokens(sel_corpus)
        assert np.array_equal(counts, np.bincount(want_ids, minlength=nat.vocab_size).astype(counts.dtype)), (form, dev)
        for o in (enc, sel_res, sel_corpus):
            o.free()
    whole.free()
    corpus.free()


def test_a_selected_corpus_goes_through_every_pass():
    """A selected corpus against an uploaded corpus of the same bytes and offsets (the checker's): every pass sees the same
    input, so what a pass computes per sample is compared exactly; the E-step's counts are sums of f64 atomics whose order
    differs from run to run, some 10^5 terms of relative error 2^-53 each, and are compared to 1e-9."""
    import torch
    (flat, offs), _ = _encoded()
    nat = _tokenizer().native_model()
    rows = _index_forms(offs)["multiset"][:48]
    want_flat, want_offs = sc.select(flat, offs, rows)
    corpus = _lib.NativeCorpus(flat, offs)
    sel = corpus.select(torch.from_numpy(rows).cuda())
    ref = _lib.NativeCorpus(want_flat, want_offs)
    corpus.free()
    assert sel.num_samples == ref.num_samples == 48 and sel.num_bytes == ref.num_bytes == want_flat.size

    def both(fn):
        return fn(sel), fn(ref)

    def ids_of(res):
        out = (res.ids(), res.offsets())
        res.free()
        return out
    a, b = both(lambda c: ids_of(nat.encode_corpus_sample(c, 0.5, 3)))
    _same(a, b, "sampling")
    a, b = both(lambda c: nat.encode_corpus_nbest(c, 2))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    _same(ids_of(a[0]), ids_of(b[0]), "n-best")
    a, b = both(lambda c: nat.lattice_stats_corpus(c, 1.0))
    assert np.array_equal(a.logz, b.logz) and np.array_equal(a.expected_tokens, b.expected_tokens)
    a, b = both(lambda c: nat.count_pairs(c))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].size > 1000
    a, b = both(lambda c: nat.estep(c))
    assert np.allclose(a[0], b[0], rtol=1e-9, atol=1e-9) and np.isclose(a[1], b[1], rtol=1e-12) and a[0].sum() > 0
    (sa, pa), (sb, pb) = both(lambda c: c.split_specials([b"the", b" a"], True))
    _same((sa.bytes(), sa.offsets()), (sb.bytes(), sb.offsets()), "split_specials")
    assert np.array_equal(pa.seg_offs(), pb.seg_offs()) and np.array_equal(pa.seg_special(), pb.seg_special()) and pa.num_segments > 48
    a, b = both(lambda c: c.normalize("nfkd"))
    _same((a.bytes(), a.offsets()), (b.bytes(), b.offsets()), "normalize")
    for o in (sa, sb, pa, pb, a, b, sel, ref):
        o.free()


def test_a_selected_result_through_the_layouts_and_the_decode():
    import torch
    tk = _tokenizer()
    (flat, offs), (ids, oo) = _encoded()
    S = oo.size - 1
    rows = _lib.shuffled_rows_host(S, 7)
    w_ids, w_offs = sc.select(ids, oo, rows)
    src = _lib.NativeResult.from_ids(ids, oo, tk.vocab_size())
    res = tgx.select(src, tgx.shuffled_rows(S, 7, src.device))
    _same((res.ids(), res.offsets()), (w_ids, w_offs), "shuffled")
    src.free()
    pad, eos = 1, 2
    for dt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        got = tensors.to_packed(res, 1000, pad_id=pad, eos_id=eos, dtype=tdt, return_doc=True)
        w = lc.packed_fast(w_ids, w_offs, 1000, pad, None, eos, dt)
        assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(("input_ids", "doc_ids", "positions"), w)), dt
        got = tensors.to_padded(res, max_length=129, pad_id=pad, eos_id=eos, dtype=tdt, return_lengths=True)
        w = lc.padded(w_ids, w_offs, 129, pad, None, eos, dtype=dt)
        assert np.array_equal(got["input_ids"].cpu().numpy(), w[0]) and np.array_equal(got["attention_mask"].cpu().numpy(), w[1])
        assert np.array_equal(got["lengths"].cpu().numpy(), w[2])
    text, to = tk.decode_result_flat(res, True)
    want_text, want_to = tk.decode_batch_flat(w_ids, w_offs, True)
    assert np.array_equal(to, want_to) and np.array_equal(text, want_text)
    # length-grouped rows: a stable argsort of the lengths on the device
    order = torch.argsort(tgx.row_lengths(res), stable=True)
    grouped = tgx.select(res, order)
    want_order = np.argsort(np.diff(w_offs.astype(np.int64)), kind="stable")
    _same((grouped.ids(), grouped.offsets()), sc.select(w_ids, w_offs, want_order), "length-grouped")
    assert (np.diff(np.diff(grouped.offsets().astype(np.int64))) >= 0).all()
    grouped.free()
    res.free()


def test_shuffled_rows_on_the_device_match_the_twin():
    import torch
    for n in (0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 65_537, 1_000_003):
        for seed in (0, 2**64 - 1, 0x1234_5678_9ABC_DEF1, 987_654_321)[: 4 if n < 100_000 else 2]:
            got = tgx.shuffled_rows(n, seed, 0)
            assert got.dtype == torch.int64 and got.device == torch.device("cuda", 0) and got.shape == (n,)
            assert np.array_equal(got.cpu().numpy(), _lib.shuffled_rows_host(n, seed)), (n, seed)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = tgx.shuffled_rows(1025, 5, torch.device("cuda"))
    assert np.array_equal(got.cpu().numpy(), sc.shuffled_rows(1025, 5))


def test_row_lengths():
    import torch
    for k in (0, 4, 9):
        case = select_cases.batch(k, "ids")
        src = _source(case, "ids")
        got = tgx.row_lengths(src)
        assert got.dtype == torch.int64 and got.device == torch.device("cuda", src.device)
        assert np.array_equal(got.cpu().numpy(), np.diff(case["offs"].astype(np.int64)))
        src.free()
    many = np.arange(5001, dtype=np.uint64) * 2   # more than one block of rows
    src = _lib.NativeResult.from_ids(np.zeros(10_000, np.uint32), many, 10)
    assert np.array_equal(tgx.row_lengths(src).cpu().numpy(), np.full(5000, 2))
    src.free()
    src = _lib.NativeResult.from_ids(np.zeros(0, np.uint32), np.zeros(1, np.uint64), 10)
    assert tgx.row_lengths(src).shape == (0,)   # S = 0
    src.free()


def test_stage_times_name_the_three_stages():
    import torch
    case = select_cases.batch(0, "ids")
    src = _source(case, "ids")
    for rows in (case["rows"], torch.from_numpy(case["rows"]).cuda()):
        out = src.select(rows)
        times = _lib.select_last_times()
        assert list(times) == ["select_check", "select_offsets_scan", "select_fill_kernel"], times
        assert all(np.isfinite(v) and v >= 0 for v in times.values()), times
        out.free()
    src.free()


def _pattern_rows_against_the_twin(kind, offs):
    """Rows of tests/past_cap.py's pattern, selected in their order, so that the output's rows are the pattern's; against
    the host twin"""
    n = int(offs[-1])
    data = (np.arange(n, dtype=np.uint64) * 7 % 251 + 1).astype(np.uint32 if kind == "ids" else np.uint8)
    rows = np.arange(offs.size - 1, dtype=np.int64)
    want = TWIN[kind](data, offs, rows)
    assert want[0].size == n
    src = _source(dict(data=data, offs=offs, vocab_size=1000), kind)
    try:
        out = src.select(rows)
        try:
            _same(_read(out, kind), want, (kind, n))
        finally:
            out.free()
    finally:
        src.free()


@pytest.mark.parametrize("kind", ["ids", "bytes"])
def test_the_second_trip_of_the_strided_tile_loop(kind):
    """T' = 2048 tiles + one tile + 1: blocks 0 and 1 of select_fill_kernel take a second tile"""
    tile = 1024 if kind == "ids" else 4096
    offs = past_cap.offsets(2048, tile)
    assert int(offs[-1]) == past_cap.n_out(2048, tile)
    _pattern_rows_against_the_twin(kind, offs)


@pytest.mark.parametrize("kind,n_out", [("ids", n) for n in past_cap.edge_sizes(4, 1024)] + [("bytes", n) for n in past_cap.edge_sizes(16, 4096)])
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(kind, n_out):
    """T' = 0, 1, a thread's slot (4 ids, 16 bytes) and the tile (1024 ids, 4096 bytes), each less one, full and one over"""
    _pattern_rows_against_the_twin(kind, past_cap.edge_offsets(n_out))
