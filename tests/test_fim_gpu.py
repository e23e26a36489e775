"""Fill-in-the-middle on the GPU (tgx_result_fim, csrc/fim.hip) against its host twin (tgx_fim_host) and the independent
checker (tests/fim_checker.py); the layouts and the decode of such a result against the host route over the twin's output;
and the Tokenizer methods with fim= against encode_batch_flat, then fim_host, then the layout checker.  Everything is
compared exactly: this is integer data movement.

The shapes are tests/fim_cases.py's (rows around one and four tiles, runs of empty rows, T' one to three positions on
either side of a tile) and one row of 70 000 tokens; the real result is test_assemble_gpu.py's corpus, 96 KiB of mixed
text with a 70 000-byte sample and empty samples, encoded with the reference's seven special tokens in it."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import fim_cases
import fim_checker as fc
import layout_checker as lc
import past_cap

SPECIALS = ["<|eos|>", "<|pad|>", "<|lang|>", "<|filename|>", "<|suffix|>", "<|prefix|>", "<|middle|>"]
FIM = dict(prefix="<|prefix|>", suffix="<|suffix|>", middle="<|middle|>", rate=0.5, spm_rate=0.5, seed=1)


def _device_and_twin(case):
    """-> (what the device gives, what the twin gives), each (ids, offsets, vocab_size, mode, cuts, n_applied)"""
    src = _lib.NativeResult.from_ids(case["ids"], case["offs"], case["vocab_size"])
    try:
        assert np.array_equal(src.ids(), case["ids"]) and np.array_equal(src.offsets(), case["offs"])   # from_ids round-trips
        assert src.vocab_size == case["vocab_size"] and src.num_samples == case["offs"].size - 1
        res, mode, cuts = src.fim(case["pre"], case["suf"], case["mid"], return_info=True, **fim_cases.args(case))
        try:
            got = (res.ids(), res.offsets(), res.vocab_size, mode, cuts, (res.num_tokens - src.num_tokens) // 3)
            assert res.num_samples == src.num_samples and res.device == src.device
        finally:
            res.free()
        assert np.array_equal(src.ids(), case["ids"]) and np.array_equal(src.offsets(), case["offs"])   # the input is only read
    finally:
        src.free()
    want = _lib.fim_host(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case))
    return got, want


def _same(got, want, key):
    for g, w, name in zip(got, want, ("ids", "offsets", "vocab_size", "mode", "cuts", "n_applied")):
        assert np.array_equal(g, w), (key, name)


@pytest.mark.parametrize("part", range(6))
def test_device_matches_twin_and_checker_on_the_shapes(part):
    for k in range(part, fim_cases.N_BATCHES, 6):
        case = fim_cases.batch(k)
        got, want = _device_and_twin(case)
        _same(got, want, k)
        _same(got, fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case)), k)
        assert int(got[1][-1]) == case["want_total"]


def test_a_row_of_70000_tokens():
    case = fim_cases.long_row()
    got, want = _device_and_twin(case)
    _same(got, want, "long")
    _same(got, fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case)), "long")
    assert got[3].tolist()[2] in (1, 2) and got[0].size == case["ids"].size + 9


def test_no_rows_one_row_and_the_optional_outputs():
    src = _lib.NativeResult.from_ids(np.zeros(0, np.uint32), np.zeros(1, np.uint64), 10)
    res, mode, cuts = src.fim(10, 11, 12, return_info=True)
    assert res.num_samples == 0 and res.num_tokens == 0 and res.offsets().tolist() == [0] and res.ids().size == 0 and res.vocab_size == 13
    assert mode.size == 0 and cuts.shape == (0, 2)
    res.free()
    src.free()
    ids, offs = np.arange(5, dtype=np.uint32), np.array([0, 5], np.uint64)
    src = _lib.NativeResult.from_ids(ids, offs, 10)
    for seed in range(8):
        res = src.fim(20, 11, 12, seed=seed)   # no info asked for: fim_info_kernel is not launched
        want = fc.fim(ids, offs, 10, 20, 11, 12, 1.0, 0.5, seed)
        assert np.array_equal(res.ids(), want[0]) and np.array_equal(res.offsets(), want[1]) and res.vocab_size == 21
        res.free()
    # n_applied at the ABI, with mode alone and with cuts alone
    h, na = C.c_void_p(), C.c_uint64(77)
    mode = np.full(1, 9, np.uint8)
    _lib.check(_lib.lib.tgx_result_fim(src._h, 20, 11, 12, 1.0, 1.0, 3, 0, None, _lib.ptr(mode), None, C.byref(na), C.byref(h)))
    assert na.value == 1 and mode.tolist() == [2]
    _lib.NativeResult(h).free()
    h, cuts = C.c_void_p(), np.full(2, 99, np.uint64)
    _lib.check(_lib.lib.tgx_result_fim(src._h, 20, 11, 12, 0.0, 1.0, 3, 0, None, None, _lib.ptr(cuts), C.byref(na), C.byref(h)))
    assert na.value == 0 and cuts.tolist() == [0, 0]
    _lib.NativeResult(h).free()
    src.free()


def test_stage_times_name_the_three_stages():
    """fim_last_times after a call that asks for the mode, so that fim_info_kernel runs too: the three stages in order,
    every time finite and not negative"""
    src = _lib.NativeResult.from_ids(np.arange(5, dtype=np.uint32), np.array([0, 5], np.uint64), 10)
    res, mode, _ = src.fim(20, 11, 12, seed=3, return_info=True)
    assert mode.size == 1
    times = _lib.fim_last_times()
    assert list(times) == ["fim_offsets_scan", "fim_fill_kernel", "fim_info_kernel"], times
    assert all(np.isfinite(v) and v >= 0 for v in times.values()), times
    res.free()
    src.free()


def test_invalid_arguments_are_refused():
    src = _lib.NativeResult.from_ids(np.arange(6, dtype=np.uint32), np.array([0, 2, 2, 6], np.uint64), 10)

    def refused(*a, **kw):
        with pytest.raises(tgx.TokenGeeXError) as e:
            src.fim(*a, **kw)
        assert e.value.status == _lib.ERR_INVALID, e.value
        return str(e.value)

    for bad in (float("nan"), -0.01, 1.01):
        assert "rate" in refused(10, 11, 12, rate=bad)
        assert "spm_rate" in refused(10, 11, 12, spm_rate=bad)
    assert "TGX_NO_ID" in refused(10, _lib.NO_ID, 12)
    assert "distinct" in refused(10, 11, 10)
    assert _lib.lib.tgx_result_fim(src._h, 10, 11, 12, 1.0, 0.5, 0, 0, None, None, None, None, None) == _lib.ERR_INVALID
    res = src.fim(10, 11, 12)   # and the stage still works
    assert res.num_tokens == 12
    res.free()
    src.free()


# ---- a real result: rows that already hold special ids ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _texts():
    """test_assemble_gpu.py's corpus as strings, with special tokens in most samples"""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]).decode("utf-8", "ignore") for i in range(offs.size - 1)]
    for k, t in enumerate(rows):
        cut = len(t) // 3
        rows[k] = ("<|lang|>" if k % 2 else "") + t[:cut] + "<|filename|>" * (k % 3) + t[cut:] + ("<|eos|>" if k % 4 else "")
    half = len(rows) // 2
    return ["", ""] + rows[:half] + ["", "", ""] + [bytes(big[:70_000]).decode("utf-8", "ignore")] + rows[half:] + ["<|pad|>", ""]


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [tgx.CrlfProcessor()], list(SPECIALS))


@functools.lru_cache(maxsize=None)
def _host_route(ordinary=False):
    """-> (the packed batch, encode_batch_flat's ids and offsets, the twin's output over them under FIM); computed once"""
    tk = _tokenizer()
    flat, offs = tgx.pack([t.encode("utf-8") for t in _texts()])
    ids, oo = tk.encode_batch_flat(flat, offs, 0.0, ordinary=ordinary)
    base = tk.base_vocab_size()
    twin = _lib.fim_host(ids, oo, tk.vocab_size(), base + 5, base + 4, base + 6, rate=0.5, spm_rate=0.5, seed=1)
    n = np.diff(oo.astype(np.int64))
    assert n.max() > 16 * 1024 and n[0] == n[1] == n[-1] == 0 and {0, 1, 2} <= set(twin[3].tolist())
    return (flat, offs), (ids, oo), twin


def test_fim_of_a_real_result_its_layouts_and_its_decode():
    import torch
    tk = _tokenizer()
    (flat, offs), (ids, oo), (w_ids, w_offs, w_vocab, w_mode, w_cuts, _) = _host_route()
    base = tk.base_vocab_size()
    assert (ids >= base).any()   # rows that already hold special ids
    src = tk.encode_batch_result_flat(flat, offs)
    res = tk.fim_result(src, **FIM)
    assert np.array_equal(res.ids(), w_ids) and np.array_equal(res.offsets(), w_offs) and res.vocab_size == w_vocab == tk.vocab_size()
    res.free()
    res, mode, cuts = src.fim(base + 5, base + 4, base + 6, rate=0.5, spm_rate=0.5, seed=1, return_info=True)
    assert np.array_equal(res.ids(), w_ids) and np.array_equal(mode, w_mode) and np.array_equal(cuts, w_cuts)
    assert np.array_equal(src.ids(), ids)
    src.free()
    # layouts
    pad, eos = base + 1, base
    for dt, tdt in ((np.int32, torch.int32), (np.int64, torch.int64)):
        got = tensors.to_packed(res, 1000, pad_id=pad, eos_id=eos, dtype=tdt, return_doc=True)
        w = lc.packed_fast(w_ids, w_offs, 1000, pad, None, eos, dt)
        assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(("input_ids", "doc_ids", "positions"), w)), dt
        got = tensors.to_padded(res, max_length=129, pad_id=pad, eos_id=eos, dtype=tdt, return_lengths=True)
        w = lc.padded(w_ids, w_offs, 129, pad, None, eos, dtype=dt)
        assert np.array_equal(got["input_ids"].cpu().numpy(), w[0]) and np.array_equal(got["attention_mask"].cpu().numpy(), w[1])
        assert np.array_equal(got["lengths"].cpu().numpy(), w[2])
    # decode, special tokens included, against the host decode of the twin's ids
    text, to = tk.decode_result_flat(res, True)
    want_text, want_to = tk.decode_batch_flat(w_ids, w_offs, True)
    assert np.array_equal(to, want_to) and np.array_equal(text, want_text)
    assert b"<|prefix|>" in bytes(text) and b"<|middle|>" in bytes(text)
    res.free()


def test_an_nbest_result_and_a_stream_of_the_caller():
    import torch
    tk = _tokenizer()
    nat = tk.native_model()
    flat, offs = tgx.pack([t.encode("utf-8") for t in _texts()[2:14]] + [b""])
    nb, _, _ = nat.encode_batch_nbest_flat(flat, offs, 3)   # 13 · 3 rows, some of them empty: its rows are rows
    ids, oo = nb.ids(), nb.offsets()
    assert nb.num_samples == 39 and (np.diff(oo.astype(np.int64)) == 0).any()
    V = nat.vocab_size
    want = _lib.fim_host(ids, oo, V, V + 2, V, V + 1, rate=0.7, spm_rate=0.3, seed=5, first_row=100)
    stream = torch.cuda.Stream(device=nb.device)
    for st in (0, stream.cuda_stream):
        res, mode, cuts = nb.fim(V + 2, V, V + 1, rate=0.7, spm_rate=0.3, seed=5, first_row=100, return_info=True, stream=st)
        _same((res.ids(), res.offsets(), res.vocab_size, mode, cuts, int((mode != 0).sum())), want, st)
        res.free()
    assert want[2] == V + 3 and {1, 2} <= set(want[3].tolist())
    nb.free()


def _eq(got: dict, want, keys):
    assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(keys, want)), keys


def test_tokenizer_layouts_with_fim():
    tk = _tokenizer()
    texts = _texts()
    base = tk.base_vocab_size()
    pad, eos = base + 1, base
    (flat, offs), (ids, oo), (w_ids, w_offs, _, _, _, _) = _host_route()
    packed_keys = ("input_ids", "doc_ids", "positions")
    got = tk.encode_batch_packed(texts, 512, pad="<|pad|>", eos="<|eos|>", return_doc=True, fim=FIM)
    _eq(got, lc.packed_fast(w_ids, w_offs, 512, pad, None, eos, np.int64), packed_keys)
    got = tk.encode_batch_padded_flat(flat, offs, pad="<|pad|>", eos="<|eos|>", max_length=200, fim=dict(FIM))
    _eq(got, lc.padded(w_ids, w_offs, 200, pad, None, eos, dtype=np.int64), ("input_ids", "attention_mask"))
    corpus = _lib.NativeCorpus(flat, offs)
    got = tk.encode_corpus_packed(corpus, 512, pad="<|pad|>", eos="<|eos|>", return_doc=True, fim=FIM)
    _eq(got, lc.packed_fast(w_ids, w_offs, 512, pad, None, eos, np.int64), packed_keys)
    got = tk.encode_corpus_padded(corpus, pad="<|pad|>", max_length=64, fim=FIM)
    _eq(got, lc.padded(w_ids, w_offs, 64, pad, dtype=np.int64), ("input_ids", "attention_mask"))
    # the ordinary path: the text is not split, the sentinels are given as ids
    _, (o_ids, o_oo), (ow_ids, ow_offs, _, _, _, _) = _host_route(True)
    assert not np.array_equal(o_ids, ids)
    fim_ids = dict(FIM, prefix=base + 5, suffix=base + 4, middle=base + 6)
    got = tk.encode_ordinary_batch_padded(texts, pad=pad, max_length=300, return_lengths=True, fim=fim_ids)
    _eq(got, lc.padded(ow_ids, ow_offs, 300, pad, dtype=np.int64), ("input_ids", "attention_mask", "lengths"))
    got = tk.encode_ordinary_batch_packed(texts, 777, pad=pad, eos=eos, fim=fim_ids)
    _eq(got, lc.packed_fast(ow_ids, ow_offs, 777, pad, None, eos, np.int64), ("input_ids",))
    # without fim= the same methods give what they give without the keyword's existence: the layouts of encode_batch_flat
    got = tk.encode_batch_packed(texts, 512, pad="<|pad|>", eos="<|eos|>", return_doc=True)
    _eq(got, lc.packed_fast(ids, oo, 512, pad, None, eos, np.int64), packed_keys)
    got = tk.encode_batch_packed(texts, 512, pad="<|pad|>", eos="<|eos|>", return_doc=True, fim=None)
    _eq(got, lc.packed_fast(ids, oo, 512, pad, None, eos, np.int64), packed_keys)
    got = tk.encode_ordinary_batch_padded(texts, pad=pad, max_length=300, return_lengths=True)
    _eq(got, lc.padded(o_ids, o_oo, 300, pad, dtype=np.int64), ("input_ids", "attention_mask", "lengths"))
    got = tk.encode_corpus_packed(corpus, 512, pad="<|pad|>", eos="<|eos|>", return_doc=True)
    _eq(got, lc.packed_fast(ids, oo, 512, pad, None, eos, np.int64), packed_keys)
    corpus.free()
    # rate 0 is the identity, a batch without samples stays one, and requests that cannot be met are refused
    got = tk.encode_batch_packed(texts, 512, pad="<|pad|>", eos="<|eos|>", fim=dict(FIM, rate=0.0))
    _eq(got, lc.packed_fast(ids, oo, 512, pad, None, eos, np.int64), ("input_ids",))
    assert tk.encode_batch_packed([], 16, pad=pad, fim=FIM)["input_ids"].shape == (0, 16)
    with pytest.raises(ValueError):
        tk.encode_batch_padded(texts[:4], pad=pad, max_length=64, return_offsets_mapping="byte", fim=FIM)
    with pytest.raises(ValueError):
        tk.encode_ordinary_batch_padded(texts[:4], pad=pad, max_length=64, return_overflowing_tokens=True, fim=FIM)
    with pytest.raises(ValueError):
        tk.encode_corpus_padded(_lib.NativeCorpus(*tgx.pack([b"ab"])), pad=pad, max_length=64, return_offsets_mapping="char", fim=FIM)
    with pytest.raises(tgx.TokenGeeXError):
        tk.encode_batch_packed(texts[:4], 64, pad=pad, fim=dict(FIM, prefix="<|nope|>"))
    with pytest.raises(TypeError):
        tk.encode_batch_packed(texts[:4], 64, pad=pad, fim=dict(prefix=1, suffix=2))


def _edge_case(target):
    """Rows of tests/past_cap.py's pattern whose T' is target.  A rearranged row grows by three sentinels, and whether a
    row is rearranged depends on the seed and its index alone, so the pattern is shortened until T' is at most the
    target, under one seed after another until it is the target."""
    V = 1000
    for seed in range(1, 200):
        fim = dict(rate=0.5, spm_rate=0.5, seed=seed, first_row=5)
        for t in range(target, -1, -1):
            offs = past_cap.edge_offsets(t)
            ids = (np.arange(t, dtype=np.uint64) * 7 % V).astype(np.uint32)
            want = _lib.fim_host(ids, offs, V, V + 2, V, V + 1, **fim)
            if int(want[1][-1]) <= target:
                break
        if int(want[1][-1]) == target and (want[5] > 0 or target < 4):
            return dict(ids=ids, offs=offs, vocab_size=V, pre=V + 2, suf=V, mid=V + 1, **fim)
    raise AssertionError(f"no seed gives T' = {target}")


@pytest.mark.parametrize("n_out", past_cap.edge_sizes(4, 1024))
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_out):
    """T' = 0, 1, a thread's slot of 4 ids and the tile of 1024, each less one, full and one over"""
    case = _edge_case(n_out)
    got, twin = _device_and_twin(case)
    assert int(twin[1][-1]) == n_out
    _same(got, twin, n_out)
    _same(got, fc.fim(case["ids"], case["offs"], case["vocab_size"], case["pre"], case["suf"], case["mid"], **fim_cases.args(case)), n_out)


def test_the_second_trip_of_the_strided_tile_loop():
    """T' = 2048 tiles + one tile + 1 (tests/past_cap.py): blocks 0 and 1 of fim_fill_kernel take a second tile"""
    V, target = 1000, past_cap.n_out(2048, 1024)
    lens = past_cap.lengths(2048, 1024)
    long_at = int(np.argmax(lens))
    fim = dict(rate=0.5, spm_rate=0.5, seed=11, first_row=5)
    for _ in range(2):  # whether a row is rearranged does not depend on its length, as long as it has a token: shorten the long row by the sentinels
        offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
        ids = (np.arange(int(offs[-1]), dtype=np.uint64) * 7 % V).astype(np.uint32)
        want = _lib.fim_host(ids, offs, V, V + 2, V, V + 1, **fim)
        lens[long_at] -= np.uint64(int(want[1][-1]) - target)
    assert int(want[1][-1]) == target and want[5] > 1000 and lens[long_at] > 1024
    case = dict(ids=ids, offs=offs, vocab_size=V, pre=V + 2, suf=V, mid=V + 1, **fim)
    got, twin = _device_and_twin(case)
    _same(got, twin, "past the cap")
