"""A sample-level result with the special tokens' ids, put together on the GPU (tgx_assemble_result, csrc/assemble.hip)
against tgx_assemble_ids over the same arrays on the host; the layouts of such a result against the plain-numpy layout
checker (tests/layout_checker.py); and the Tokenizer methods over it against encode_batch_flat.  Everything is compared
exactly: this is integer data movement.

The segment-level results are real: encode and sampling over a corpus with empty rows at the start, in the middle and at
the end (encoded segments without ids) and one row of 70 000 bytes (a segment that spans about 17 of the kernel's
1024-position tiles)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import layout_checker as lc
import past_cap

N_SPECIALS = 6
PAD = 7


@functools.lru_cache(maxsize=None)
def _texts():
    """test_layout_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    return [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]


@functools.lru_cache(maxsize=None)
def _native():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.NativeModel(list(toks), np.asarray(scores, np.float64))


@functools.lru_cache(maxsize=None)
def _segs(name):
    """-> (NativeResult over the corpus' rows as segments, its ids, its offsets); computed once, never changed"""
    flat, offs = tgx.pack(_texts())
    res = _native().encode_batch_flat(flat, offs) if name == "encode" else _native().encode_batch_sample_flat(flat, offs, 0.5, 3)
    ids, oo = res.ids(), res.offsets()
    n = np.diff(oo.astype(np.int64))
    assert n.max() > 16 * 1024 and n[0] == n[1] == n[-1] == 0 and (n == 0).sum() >= 6
    return res, ids, oo


def _empty_rows(oo):
    return set(np.flatnonzero(np.diff(oo.astype(np.int64)) == 0).tolist())


def _plan(items, sample_sizes):
    """items: -1 (the next encoded segment) or a special's index; sample_sizes: segments per sample -> (seg_offs, seg_special)"""
    assert sum(sample_sizes) == len(items)
    seg_offs = np.zeros(len(sample_sizes) + 1, np.uint64)
    np.cumsum(sample_sizes, out=seg_offs[1:])
    return seg_offs, np.asarray(items, np.int32).reshape(-1)


def _spread(K, S):
    """K segments over S samples of uneven sizes"""
    cuts = np.linspace(0, K, S + 1).astype(np.int64)
    return np.diff(cuts).tolist()


def _plans(E, empty_rows):
    sp = lambda i: int(i) % N_SPECIALS   # noqa: E731
    plans = {}
    plans["no_specials_regrouped"] = _plan([-1] * E, [0, 3, 0, 0] + _spread(E - 3, 9) + [0])
    alt = [x for k in range(E) for x in (sp(k), -1)]
    plans["alternating"] = _plan(alt, _spread(2 * E, 11))
    run = [sp(k) for k in range(3000)]
    mid = E // 2
    runs = run + [-1] * mid + run[::-1] + [-1] * (E - mid) + run
    plans["runs_of_3000_specials"] = _plan(runs, _spread(len(runs), 13))
    beside = []
    for k in range(E):   # a special on both sides of every run of segments without ids (rows 0, 1 and E - 1 are such: both ends)
        if k in empty_rows and k - 1 not in empty_rows and k > 0:
            beside.append(sp(k))
        beside.append(-1)
        if k in empty_rows and k + 1 not in empty_rows and k + 1 < E:
            beside.append(sp(k + 1))
    assert beside[0] == beside[1] == beside[-1] == -1 and beside[2] >= 0 and beside[-2] >= 0
    plans["empty_segments_beside_specials"] = _plan(beside, _spread(len(beside), 7))
    plans["segmentless_samples"] = _plan(alt, [0, 0] + _spread(E, 3) + [0, 0, 0] + _spread(E, 4) + [0])
    plans["one_sample"] = _plan(alt, [2 * E])
    return plans


PLAN_NAMES = ["no_specials_regrouped", "alternating", "runs_of_3000_specials", "empty_segments_beside_specials",
              "segmentless_samples", "one_sample"]


def _assemble_and_compare(segs, ids, oo, seg_offs, ss, key):
    nat = _native()
    V = nat.vocab_size
    want_ids, want_offs = _lib.assemble_ids(seg_offs, ss, ids, oo, V)
    res = nat.assemble(segs, seg_offs, ss, N_SPECIALS)
    try:
        assert res.num_samples == seg_offs.size - 1 and res.num_tokens == want_ids.size, key
        assert res.vocab_size == V + N_SPECIALS and res.device == nat.device, key
        got_ids, got_offs = res.ids(), res.offsets()
        assert np.array_equal(got_offs, want_offs), key
        assert np.array_equal(got_ids, want_ids), key
    finally:
        res.free()
    return want_ids, want_offs


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_assemble_over_an_encode_result(name):
    segs, ids, oo = _segs("encode")
    E = segs.num_samples
    seg_offs, ss = _plans(E, _empty_rows(oo))[name]
    want_ids, want_offs = _assemble_and_compare(segs, ids, oo, seg_offs, ss, name)
    if name == "no_specials_regrouped":
        assert np.array_equal(want_ids, ids) and np.array_equal(want_offs, oo[seg_offs.astype(np.int64)])
    if name == "runs_of_3000_specials":
        assert want_ids.size > ids.size + 8000 and (want_ids[:3000] >= _native().vocab_size).all()
    # the segment-level result is only read: it is the same afterwards, and usable again
    assert np.array_equal(segs.ids(), ids) and np.array_equal(segs.offsets(), oo)
    times = _native().last_kernel_times()
    assert {"assemble_starts_kernel", "assemble_fill_kernel"} <= set(times), times


def test_assemble_over_a_sampling_result():
    segs, ids, oo = _segs("sample")
    assert not np.array_equal(ids, _segs("encode")[1])
    E = segs.num_samples
    seg_offs, ss = _plans(E, _empty_rows(oo))["runs_of_3000_specials"]
    _assemble_and_compare(segs, ids, oo, seg_offs, ss, "sample")


def test_all_special_and_no_sample():
    nat = _native()
    V = nat.vocab_size
    sp = (np.arange(2500) * 5 % N_SPECIALS).astype(np.int32)
    seg_offs = np.array([0, 0, 1, 1024, 1024, 2049, 2500, 2500], np.uint64)
    res = nat.assemble(None, seg_offs, sp, N_SPECIALS)     # K = 2500, E = 0: no result over encoded segments
    assert res.num_samples == 7 and res.num_tokens == 2500 and res.vocab_size == V + N_SPECIALS
    assert np.array_equal(res.ids(), V + sp.astype(np.uint32)) and np.array_equal(res.offsets(), seg_offs)
    res.free()
    res = nat.assemble(None, np.zeros(1, np.uint64), np.zeros(0, np.int32), N_SPECIALS)   # S = 0
    assert res.num_samples == 0 and res.num_tokens == 0 and res.offsets().tolist() == [0] and res.ids().size == 0
    res.free()
    res = nat.assemble(None, np.zeros(4, np.uint64), np.zeros(0, np.int32), 0)   # samples, none with a segment
    assert res.num_samples == 3 and res.num_tokens == 0 and res.offsets().tolist() == [0, 0, 0, 0] and res.vocab_size == V
    res.free()


def test_layouts_of_an_assembled_result():
    import torch
    segs, ids, oo = _segs("encode")
    nat = _native()
    V = nat.vocab_size
    E = segs.num_samples
    seg_offs, ss = _plans(E, _empty_rows(oo))["runs_of_3000_specials"]
    h_ids, h_offs = _lib.assemble_ids(seg_offs, ss, ids, oo, V)
    res = nat.assemble(segs, seg_offs, ss, N_SPECIALS)
    bos, eos = V + 1, V + 2
    n = np.diff(h_offs.astype(np.int64))
    for dt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        for L in (129, int(n.max()) + 2):
            got = tensors.to_padded(res, max_length=L, pad_id=V, bos_id=bos, eos_id=eos, dtype=tdt, return_lengths=True)
            w = lc.padded(h_ids, h_offs, L, V, bos, eos, dtype=dt)
            assert np.array_equal(got["input_ids"].cpu().numpy(), w[0]) and np.array_equal(got["attention_mask"].cpu().numpy(), w[1])
            assert np.array_equal(got["lengths"].cpu().numpy(), w[2])
        got = tensors.to_padded(res, max_length=300, pad_id=V, eos_id=eos, dtype=tdt, padding_side="left", truncation_side="left")
        assert np.array_equal(got["input_ids"].cpu().numpy(), lc.padded(h_ids, h_offs, 300, V, None, eos, True, True, dt)[0])
        for L, b, e in ((512, bos, eos), (1000, None, eos), (4096, None, None)):
            got = tensors.to_packed(res, L, pad_id=V, bos_id=b, eos_id=e, dtype=tdt, return_doc=True)
            w = lc.packed_fast(h_ids, h_offs, L, V, b, e, dt)
            assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(("input_ids", "doc_ids", "positions"), w)), (dt, L)
    # pad_into / pack_into and the host accessors take it as any result
    out = torch.full((res.num_samples, 64), -77, dtype=torch.int32, device=torch.device("cuda", res.device))
    tensors.pad_into(res, out, row_len=64, pad_id=PAD)
    assert np.array_equal(out.cpu().numpy(), lc.padded(h_ids, h_offs, 64, PAD)[0])
    n_stream = res.layout_info(None, eos)[1]
    assert n_stream == h_ids.size + res.num_samples
    B = -(-n_stream // 777)
    out = torch.full((B, 777), -77, dtype=torch.int64, device=torch.device("cuda", res.device))
    assert tensors.pack_into(res, out, block_len=777, pad_id=PAD, eos_id=eos) == B
    assert np.array_equal(out.cpu().numpy(), lc.packed_fast(h_ids, h_offs, 777, PAD, None, eos, np.int64)[0])
    res.free()


def test_invalid_plans_are_refused_before_any_launch():
    nat = _native()
    segs, ids, oo = _segs("encode")
    E = segs.num_samples
    ok_offs, ok_ss = _plan([-1] * E, _spread(E, 5))

    def refused(segs_, seg_offs, ss, n_specials=N_SPECIALS, model=nat):
        with pytest.raises(tgx.TokenGeeXError) as e:
            model.assemble(segs_, np.asarray(seg_offs, np.uint64), np.asarray(ss, np.int32), n_specials)
        assert e.value.status == _lib.ERR_INVALID, e.value
        return str(e.value)

    bad = ok_offs.copy()
    bad[0] = 1
    assert "seg_offs[0]" in refused(segs, bad, ok_ss)
    bad = ok_offs.copy()
    bad[2], bad[3] = ok_offs[3], ok_offs[2]
    assert "monotone" in refused(segs, bad, ok_ss)
    assert "special token" in refused(segs, [0, E + 1], [N_SPECIALS] + [-1] * E)
    assert "special token" in refused(segs, [0, E + 1], [0] + [-1] * E, n_specials=0)
    assert "rows" in refused(segs, [0, E - 1], [-1] * (E - 1))
    assert "rows" in refused(segs, [0, E + 1], [-1] * (E + 1))
    assert "no result" in refused(None, [0, 2], [-1, 0])
    assert "no room" in refused(segs, ok_offs, ok_ss, n_specials=0xFFFFFFFE - nat.vocab_size + 1)
    # an n-best result has n_samples * nbest rows: its rows are not the plan's segments
    flat, offs = tgx.pack(_texts()[:12])
    nb, _, _ = nat.encode_batch_nbest_flat(flat, offs, 3)
    assert "rows" in refused(nb, [0, 12], [-1] * 12)
    nb.free()
    # a result written by a model with another vocabulary size
    toks, scores, _ = synth.load_spec_vocab(32000)
    other = tgx.NativeModel(list(toks)[:-5], np.asarray(scores, np.float64)[:-5])
    assert "tokens" in refused(segs, ok_offs, ok_ss, model=other)
    if tgx.device_count() >= 2:
        far = tgx.NativeModel(list(toks), np.asarray(scores, np.float64), device=1)
        assert "device" in refused(segs, ok_offs, ok_ss, model=far)
    # and the stage still works
    _assemble_and_compare(segs, ids, oo, ok_offs, ok_ss, "after the refusals")


# ---- Tokenizer level ---------------------------------------------------------------------------------------------

SPECIALS = ["<|endoftext|>", "<|fim", "<|fim|>", "<pad>", "<s>", "</s>"]   # "<|fim" is a prefix of "<|fim|>" and listed first: it wins


def _tokenizer(procs=(), specials=SPECIALS):
    toks, scores, _ = synth.load_spec_vocab(32000)
    processors = [tgx.CrlfProcessor() if p == "crlf" else tgx.UnicodeProcessor(p) for p in procs]
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors, list(specials))


def _str_texts():
    body = [t.decode("utf-8", "ignore") for t in _texts()[2:40]]
    texts = ["", "<|endoftext|>", "<s></s><pad><|fim|><|fim", "no special token in here", "a\r\n<s>\r\nb\r\n", "\r\n</s>",
             "é Å<|endoftext|>é", "<|fim|>prefix<|fim>suffix<|fim|middle", ""]
    for k, t in enumerate(body):
        cut = len(t) // 3
        texts.append(t[:cut] + "<|fim|>" + t[cut:2 * cut] + "<s>" * (k % 3) + t[2 * cut:] + ("<|endoftext|>" if k % 2 else ""))
    return texts + ["<pad>", ""]


@pytest.mark.parametrize("procs", [("crlf",), ("nfc",)])
def test_tokenizer_result_and_layouts(procs):
    import torch
    tk = _tokenizer(procs)
    tk.seed = 4321
    texts = _str_texts()
    flat, offs = tgx.pack([t.encode("utf-8") for t in texts])
    base = tk.base_vocab_size()
    for dropout in (0.0, 0.1):
        want_ids, want_offs = tk.encode_batch_flat(flat, offs, dropout)
        res = tk.encode_batch_result_flat(flat, offs, dropout)
        assert res.vocab_size == tk.vocab_size() and res.num_samples == len(texts)
        assert np.array_equal(res.offsets(), want_offs) and np.array_equal(res.ids(), want_ids), (procs, dropout)
        res.free()
    assert not np.array_equal(tk.encode_batch_flat(flat, offs, 0.1)[0], tk.encode_batch_flat(flat, offs, 0.0)[0])
    ids, o = tk.encode_batch_flat(flat, offs, 0.0)
    rows = [ids[int(o[i]):int(o[i + 1])].tolist() for i in range(len(texts))]
    assert rows[1] == [base] and rows[2] == [base + 4, base + 5, base + 3, base + 1] + rows[2][4:] and rows[2][4:] == tk.encode_ordinary("|>", 0.0) + [base + 1]
    assert rows[0] == [] and max(rows[3]) < base
    assert rows == tk.encode_batch(texts, 0.0)
    pad, bos, eos = base + 3, base + 4, base + 5
    got = tk.encode_batch_padded(texts, pad="<pad>", bos="<s>", eos="</s>", max_length=200, return_lengths=True)
    w = lc.padded(ids, o, 200, pad, bos, eos, dtype=np.int64)
    assert got["input_ids"].dtype == torch.int64 and got["input_ids"].device == torch.device("cuda", 0)
    assert np.array_equal(got["input_ids"].cpu().numpy(), w[0]) and np.array_equal(got["attention_mask"].cpu().numpy(), w[1])
    assert np.array_equal(got["lengths"].cpu().numpy(), w[2])
    got = tk.encode_batch_padded_flat(flat, offs, pad_id=pad, eos="</s>", padding_side="left", dtype=torch.int32)
    mx = int(np.diff(o.astype(np.int64)).max()) + 1
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.padded(ids, o, mx, pad, None, eos, pad_left=True)[0])
    got = tk.encode_batch_packed(texts, 512, pad="<pad>", eos="<|endoftext|>", return_doc=True)
    w = lc.packed(ids, o, 512, pad, None, base, np.int64)
    assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(("input_ids", "doc_ids", "positions"), w))
    got = tk.encode_batch_packed_flat(flat, offs, 100, pad=pad, bos="<s>", drop_last=True, dtype=torch.int32)
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.packed(ids, o, 100, pad, bos, None)[0][:-1])
    # with dropout the layouts are those of encode_batch_flat under the same seed
    d_ids, d_o = tk.encode_batch_flat(flat, offs, 0.1)
    got = tk.encode_batch_packed(texts, 256, 0.1, pad=pad, eos="</s>")
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.packed(d_ids, d_o, 256, pad, None, eos, np.int64)[0])
    # a batch of special tokens only (no segment is encoded), and batches without samples
    only = ["<s></s>", "", "<pad>"]
    r = tk.encode_batch_result_flat(*tgx.pack([t.encode() for t in only]))
    assert r.ids().tolist() == [bos, eos, pad] and r.offsets().tolist() == [0, 2, 2, 3]
    r.free()
    assert tk.encode_batch_result_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64)) is None
    assert tk.encode_batch_padded([], pad=pad, bos=bos)["input_ids"].shape == (0, 1)
    assert tk.encode_batch_packed([], 16, pad=pad, return_doc=True)["doc_ids"].shape == (0, 16)


@pytest.mark.parametrize("procs", [("crlf",), ("nfc",)])
def test_tokenizer_sampling_result(procs):
    tk = _tokenizer(procs)
    texts = _str_texts()
    flat, offs = tgx.pack([t.encode("utf-8") for t in texts])
    want_ids, want_offs, want_logz = tk.encode_batch_sample_flat(flat, offs, 0.7, seed=99, return_logz=True)
    res, logz = tk.encode_batch_sample_result_flat(flat, offs, 0.7, seed=99, return_logz=True)
    assert np.array_equal(res.ids(), want_ids) and np.array_equal(res.offsets(), want_offs)
    assert logz.dtype == np.float64 and np.array_equal(logz, want_logz)
    assert res.vocab_size == tk.vocab_size()
    res.free()
    assert not np.array_equal(want_ids, tk.encode_batch_flat(flat, offs, 0.0)[0])
    res = tk.encode_batch_sample_result_flat(flat, offs, 0.7, seed=99)
    assert np.array_equal(res.ids(), want_ids)
    res.free()
    assert tk.encode_batch_sample_result_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 0.7, seed=1) is None


def test_tokenizer_without_special_tokens():
    tk = _tokenizer(("crlf",), specials=[])
    texts = [t for t in _str_texts() if t][:30]
    base = tk.base_vocab_size()
    a = tk.encode_batch_padded(texts, pad=base - 1, max_length=128, return_lengths=True)
    b = tk.encode_ordinary_batch_padded(texts, pad=base - 1, max_length=128, return_lengths=True)
    assert set(a) == set(b) and all(np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    a = tk.encode_batch_packed(texts, 256, pad=base - 1, return_doc=True)
    b = tk.encode_ordinary_batch_packed(texts, 256, pad=base - 1, return_doc=True)
    assert set(a) == set(b) and all(np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    flat, offs = tgx.pack([t.encode("utf-8") for t in texts])
    res = tk.encode_batch_result_flat(flat, offs)
    want = tk.encode_batch_flat(flat, offs)
    assert np.array_equal(res.ids(), want[0]) and np.array_equal(res.offsets(), want[1]) and res.vocab_size == base
    res.free()
    res, logz = tk.encode_batch_sample_result_flat(flat, offs, 0.3, seed=5, return_logz=True)
    want = tk.encode_batch_sample_flat(flat, offs, 0.3, seed=5, return_logz=True)
    assert np.array_equal(res.ids(), want[0]) and np.array_equal(res.offsets(), want[1]) and np.array_equal(logz, want[2])
    res.free()


def test_a_byte_without_a_token_fails_as_encode_batch_flat_does():
    tk = tgx.Tokenizer([(b"a", -1.0, False), (b"b", -2.0, False), (b"ab", -2.5, False)], [], ["<s>"])
    bad = tgx.pack([b"ab<s>a", b"a<s>abc<s>b", b"<s>"])
    good = tgx.pack([b"ab<s>a", b"<s>", b"", b"b<s><s>ab"])
    with pytest.raises(tgx.TokenGeeXError) as want:
        tk.encode_batch_flat(*bad)
    for call in (lambda: tk.encode_batch_result_flat(*bad), lambda: tk.encode_batch_padded_flat(*bad, pad="<s>"),
                 lambda: tk.encode_batch_packed_flat(*bad, 8, pad="<s>")):
        with pytest.raises(tgx.TokenGeeXError) as got:
            call()
        assert got.value.status == want.value.status == _lib.ERR_NO_PATH and str(got.value) == str(want.value)
        assert (got.value.sample, got.value.pos, got.value.length) == (want.value.sample, want.value.pos, want.value.length)
    res = tk.encode_batch_result_flat(*good)
    w_ids, w_offs = tk.encode_batch_flat(*good)
    assert np.array_equal(res.ids(), w_ids) and np.array_equal(res.offsets(), w_offs)
    assert w_ids.tolist() == [2, 3, 0, 3, 1, 3, 3, 2]
    res.free()


def _pattern_rows_against_the_twin(lens):
    """A row of the pattern (tests/past_cap.py) is a segment: every third one-id row a special token, the others encoded
    segments of as many ids; five segments to a sample; against the host twin"""
    nat = _native()
    V = nat.vocab_size
    ones = np.flatnonzero(lens == 1)
    ss = np.full(lens.size, -1, np.int32)
    ss[ones[::3]] = np.arange(ones[::3].size) % N_SPECIALS
    enc = lens[ss < 0]
    oo = np.concatenate([np.zeros(1, np.uint64), np.cumsum(enc, dtype=np.uint64)])
    ids = (np.arange(int(oo[-1]), dtype=np.uint64) * 7 % V).astype(np.uint32)
    seg_offs = np.unique(np.append(np.arange(0, lens.size, 5), lens.size)).astype(np.uint64)
    want_ids, want_offs = _lib.assemble_host(seg_offs, ss, ids, oo, V, N_SPECIALS)
    assert want_ids.size == int(lens.sum())
    segs = _lib.NativeResult.from_ids(ids, oo, V)
    res = nat.assemble(segs, seg_offs, ss, N_SPECIALS)
    try:
        assert np.array_equal(res.offsets(), want_offs)
        assert np.array_equal(res.ids(), want_ids)
    finally:
        res.free()
        segs.free()


def test_the_second_trip_of_the_strided_tile_loop():
    """T' = 2048 tiles + one tile + 1: blocks 0 and 1 of assemble_fill_kernel take a second tile; segments of 0, 1 and
    (once) more than a tile of ids"""
    lens = past_cap.lengths(2048, 1024)
    assert int(lens.sum()) == past_cap.n_out(2048, 1024)
    _pattern_rows_against_the_twin(lens)


@pytest.mark.parametrize("n_out", past_cap.edge_sizes(4, 1024))
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_out):
    """T' = 0, 1, a thread's slot of 4 ids and the tile of 1024, each less one, full and one over"""
    _pattern_rows_against_the_twin(past_cap.edge_lengths(n_out))
