"""Token spans on the GPU (tgx_result_spans_device / tgx_result_pad_spans_device, csrc/spans.hip) against the plain
restatement in tests/spans_checker.py and against the input text.  Everything is compared exactly: integer data movement.

The source results are those of tests/test_layout_gpu.py — encode, sampling, n-best at k = 3 and a resident corpus over
~96 KiB of mixed text with empty samples and one sample of 70 000 bytes (a row far longer than a tile of 1024 elements, rows
that start and end inside tiles) — built once and shared with that file's tests."""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import past_cap
import spans_checker as sc
from test_layout_gpu import SOURCES, _native, _source, _texts

POISON = -77   # what a destination holds before the call: an element the kernel skipped shows
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]
UNITS = ["byte", "char"]
G = 1 << 30


def _torch():
    import torch
    return torch


def _tdtype(dt):
    torch = _torch()
    return torch.int64 if dt == np.int64 else torch.int32


@functools.lru_cache(maxsize=None)
def _spec_tokens():
    toks, _, _ = synth.load_spec_vocab(32000)
    return list(toks)


@functools.lru_cache(maxsize=None)
def _want_flat(source, unit):
    """the checker's flat spans of a source, computed once"""
    _, ids, offs = _source(source)
    w = sc.flat(ids, offs, sc.vocab_lookup(_spec_tokens()), unit)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("source", SOURCES)
def test_flat_against_the_checker_and_the_input_text(source):
    torch = _torch()
    res, ids, offs = _source(source)
    nat, toks = _native(), _spec_tokens()
    dev = torch.device("cuda", res.device)
    T = res.num_tokens
    assert T > 20 * 1024
    for unit, dt in itertools.product(UNITS, [np.int32, np.int64]):
        out = torch.full((T, 2), POISON, dtype=_tdtype(dt), device=dev)
        tensors.spans_into(res, nat, out, unit=unit)
        assert np.array_equal(out.cpu().numpy(), _want_flat(source, unit)), (source, unit, dt)
    got = tensors.to_spans(res, nat, unit="byte")
    assert got.dtype == torch.int64 and got.shape == (T, 2) and got.device == dev
    sp = got.cpu().numpy()
    texts = _texts()
    k = 3 if source == "nbest" else 1    # n-best rows are rows of the same sample
    for i in range(res.num_samples):
        raw = texts[i // k]
        lo, hi = int(offs[i]), int(offs[i + 1])
        for j in range(lo, hi):
            assert raw[sp[j, 0]:sp[j, 1]] == toks[ids[j]], (source, i, j)
        if hi > lo:
            assert sp[lo, 0] == 0 and sp[hi - 1, 1] == len(raw) and np.array_equal(sp[lo + 1:hi, 0], sp[lo:hi - 1, 1])


@pytest.mark.parametrize("source", SOURCES)
def test_padded_against_the_checker(source):
    """All four bos / eos combinations, both padding and both truncation sides, L in {A or 1, about half a median row, the
    longest row, the longest + 3}; unit and dtype take turns over these 64 cases, so that each of the four kinds meets every
    bos / eos combination, side and length.  The host twin runs the full product with every kind on a machine without a
    GPU (tests/test_spans_cpu.py)."""
    torch = _torch()
    res, ids, offs = _source(source)
    nat = _native()
    dev = torch.device("cuda", res.device)
    S = res.num_samples
    n = np.diff(offs.astype(np.int64))
    lookup = sc.vocab_lookup(_spec_tokens())
    kinds = list(itertools.product(UNITS, [np.int32, np.int64]))
    for q, (bos, eos) in enumerate(BOS_EOS):
        a = (bos is not None) + (eos is not None)
        mx = int(n.max()) + a
        assert res.layout_info(bos, eos)[0] == mx
        row_lens = sorted({max(1, a), max(1, a, int(np.median(n)) // 2 + a), mx, mx + 3})
        for turn, (L, pside, tside) in enumerate(itertools.product(row_lens, ["right", "left"], ["right", "left"])):
            unit, dt = kinds[(turn + turn // 4 + q) % 4]
            out = torch.full((S, L, 2), POISON, dtype=_tdtype(dt), device=dev)
            tensors.pad_spans_into(res, nat, out, row_len=L, unit=unit, bos_id=bos, eos_id=eos, padding_side=pside, truncation_side=tside)
            want = sc.padded(ids, offs, lookup, unit, L, bos, eos, pside == "left", tside == "left", dt, flat_spans=_want_flat(source, unit))
            assert np.array_equal(out.cpu().numpy(), want), (source, unit, dt, bos, eos, pside, tside, L)
    got = tensors.to_padded_spans(res, nat, unit="char", dtype=torch.int32, bos_id=1)
    assert got.shape == (S, int(n.max()) + 1, 2) and got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), sc.padded(ids, offs, lookup, "char", int(n.max()) + 1, 1, None, flat_spans=_want_flat(source, "char")))


def test_unaligned_destinations_and_the_library_stream():
    """Raw pointers (NativeModel.result_spans / result_pad_spans): destinations that are not aligned to a pair (the
    element-wide store path of the kernels), on the library's stream (stream = 0), which is ordered after torch's fills."""
    torch = _torch()
    res, ids, offs = _source("encode")
    nat = _native()
    dev = torch.device("cuda", res.device)
    S, T, L = res.num_samples, res.num_tokens, 33
    none = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    lookup = sc.vocab_lookup(_spec_tokens())
    for dt, shift in itertools.product([np.int32, np.int64], [0, 1]):
        flags = _lib.span_flags("char", dt)
        buf = torch.full((T * 2 + 8,), POISON, dtype=_tdtype(dt), device=dev)
        out = buf[shift:shift + T * 2]
        nat.result_spans(res, *none, out.data_ptr(), flags=flags)
        assert np.array_equal(out.cpu().numpy().reshape(T, 2), _want_flat("encode", "char"))
        assert (buf[:shift] == POISON).all() and (buf[shift + T * 2:] == POISON).all()   # nothing beside the destination
        buf = torch.full((S * L * 2 + 8,), POISON, dtype=_tdtype(dt), device=dev)
        out = buf[shift:shift + S * L * 2]
        nat.result_pad_spans(res, *none, L, out.data_ptr(), eos_id=2, flags=flags)
        want = sc.padded(ids, offs, lookup, "char", L, None, 2, flat_spans=_want_flat("encode", "char"))
        assert np.array_equal(out.cpu().numpy().reshape(S, L, 2), want)
        assert (buf[:shift] == POISON).all() and (buf[shift + S * L * 2:] == POISON).all()


CJK_ROWS = ["你好，世界", "a\U0001f600b\U0001f4a9", "", "日本語 text é€", "\U0001f600", "x"]


def test_single_byte_vocabulary_on_cjk_text():
    """every token is one byte, so every character of more than one byte is split: all of its tokens get that character"""
    torch = _torch()
    toks = [bytes([b]) for b in range(256)]
    nat = tgx.NativeModel(toks, np.full(256, -1.0))
    raws = [t.encode() for t in CJK_ROWS]
    res = nat.encode_batch_flat(*tgx.pack(raws))
    ids, offs = res.ids(), res.offsets()
    assert ids.tolist() == list(b"".join(raws))
    for dt in (torch.int32, torch.int64):
        got = tensors.to_spans(res, nat, unit="char", dtype=dt).cpu().numpy()
        assert np.array_equal(got, sc.flat(ids, offs, sc.vocab_lookup(toks), "char"))
    for i, s in enumerate(CJK_ROWS):
        for j in range(int(offs[i]), int(offs[i + 1])):
            cs, ce = got[j]
            assert ce == cs + 1 and bytes([ids[j]]) in s[cs:ce].encode(), (i, j)
    L = 9
    got = tensors.to_padded_spans(res, nat, unit="char", max_length=L, bos_id=7, truncation_side="left").cpu().numpy()
    assert np.array_equal(got, sc.padded(ids, offs, sc.vocab_lookup(toks), "char", L, 7, None, False, True))
    res.free()


def _tokenizer(processors=()):
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], list(processors), ["<pad>", "<s>", "</s>", "<|é|>"])


def _flatten(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.array([i for r in rows for i in r], np.uint32), offs


def test_tokenizer_offset_mapping_with_special_tokens_in_the_text():
    torch = _torch()
    tk = _tokenizer()
    texts = ["def f(x):</s>\n    return x  # 你好", "", "<s>plain text<|é|> and more<|é|></s>", "</s>", "no specials here: 世界 é"]
    rows = tk.encode_batch(texts, 0.0)
    ids, offs = _flatten(rows)
    base = tk.base_vocab_size()
    pad, bos, eos = base, base + 1, base + 2
    lookup = tk.id_to_token
    before = tk.encode_batch_padded(texts, pad="<pad>", bos="<s>", max_length=40)
    assert set(before) == {"input_ids", "attention_mask"}     # the default call returns what it returned before
    for unit, dt in itertools.product(UNITS, [torch.int32, torch.int64]):
        got = tk.encode_batch_padded(texts, pad="<pad>", bos="<s>", max_length=40, dtype=dt, return_offsets_mapping=unit)
        assert set(got) == {"input_ids", "attention_mask", "offset_mapping"}
        assert torch.equal(got["input_ids"], before["input_ids"].to(dt)) and torch.equal(got["attention_mask"], before["attention_mask"])
        om = got["offset_mapping"]
        assert om.shape == (len(texts), 40, 2) and om.dtype == dt and om.device == got["input_ids"].device
        assert np.array_equal(om.cpu().numpy(), sc.padded(ids, offs, lookup, unit, 40, bos, None))
    # the special's span is its own text and the tokens after it are shifted by its length
    got = tk.encode_batch_padded(texts, pad="<pad>", return_offsets_mapping="char", padding_side="left")
    cols = got["input_ids"].shape[1]
    om, inp, mask = got["offset_mapping"].cpu().numpy(), got["input_ids"].cpu().numpy(), got["attention_mask"].cpu().numpy()
    n_special = 0
    for i, s in enumerate(texts):
        assert mask[i].sum() == len(rows[i]) and inp[i, cols - len(rows[i]):].tolist() == rows[i]
        for c in range(cols - len(rows[i]), cols):
            cs, ce = om[i, c]
            assert s[cs:ce].encode().find(tk.id_to_token(int(inp[i, c]))) >= 0, (i, c)
            if inp[i, c] >= base:
                assert s[cs:ce] == tk.id_to_special_token(int(inp[i, c]))
                n_special += 1
        assert (om[i, :cols - len(rows[i])] == 0).all()
    assert n_special == 6
    j = rows[2].index(base + 3)     # "<|é|>" is 5 characters and 6 bytes: what follows it is shifted by that much
    byte_om = tk.encode_batch_padded(texts, pad="<pad>", return_offsets_mapping="byte")["offset_mapping"].cpu().numpy()
    assert texts[2].index("<|é|>") == 13
    assert (om[2, cols - len(rows[2]) + j] == [13, 18]).all() and (byte_om[2, j] == [13, 19]).all() and byte_om[2, j + 1, 0] == 19
    # the other three surfaces, and the flat spans of a device result
    flat, o = tgx.pack([t.encode() for t in texts])
    got = tk.encode_batch_padded_flat(flat, o, pad=pad, eos="</s>", return_offsets_mapping="byte", dtype=torch.int32)
    mx = int(np.diff(offs.astype(np.int64)).max()) + 1
    assert np.array_equal(got["offset_mapping"].cpu().numpy(), sc.padded(ids, offs, lookup, "byte", mx, None, eos, dtype=np.int32))
    o_rows = tk.encode_ordinary_batch(texts, 0.0)
    o_ids, o_offs = _flatten(o_rows)
    for got in (tk.encode_ordinary_batch_padded(texts, pad=pad, max_length=16, return_offsets_mapping="char", truncation_side="left"),
                tk.encode_ordinary_batch_padded_flat(flat, o, pad=pad, max_length=16, return_offsets_mapping="char", truncation_side="left")):
        assert np.array_equal(got["offset_mapping"].cpu().numpy(), sc.padded(o_ids, o_offs, lookup, "char", 16, trunc_left=True))
    res = tk.encode_batch_result_flat(flat, o)
    assert res.vocab_size == tk.vocab_size()
    sp = tk.result_spans(res)
    assert sp.dtype == torch.int64 and np.array_equal(sp.cpu().numpy(), sc.flat(ids, offs, lookup, "char"))
    assert np.array_equal(tk.result_spans_flat(res, "byte", torch.int32), sc.flat(ids, offs, lookup, "byte", np.int32))
    res.free()
    e = tk.encode_batch_padded([], pad=pad, bos=bos, return_offsets_mapping="char")
    assert e["offset_mapping"].shape == (0, 1, 2) and e["offset_mapping"].dtype == e["input_ids"].dtype
    with pytest.raises(ValueError):
        tk.encode_batch_padded(texts, pad=pad, return_offsets_mapping="token")


def test_spans_index_the_processed_text():
    tk = _tokenizer([tgx.CrlfProcessor()])
    texts = ["line one\r\nline two\r\n\r\nthree 你好\r\n", "a\r\n<s>b\r\n", "plain"]
    flat, o = tgx.pack([t.encode() for t in texts])
    res = tk.encode_batch_result_flat(flat, o)
    ids, offs = res.ids(), res.offsets()
    bsp, csp = tk.result_spans_flat(res, "byte"), tk.result_spans_flat(res, "char")
    res.free()
    for i, t in enumerate(texts):
        row = [int(x) for x in ids[int(offs[i]):int(offs[i + 1])]]
        processed = tk.decode(row, True)
        assert processed == t.replace("\r\n", "\n") and (i == 2 or processed != t)
        for k, x in enumerate(row):
            j = int(offs[i]) + k
            assert processed.encode()[bsp[j, 0]:bsp[j, 1]] == tk.id_to_token(x)
            assert tk.id_to_token(x) in processed[csp[j, 0]:csp[j, 1]].encode()
        assert bsp[int(offs[i + 1]) - 1, 1] == len(processed.encode()) and csp[int(offs[i + 1]) - 1, 1] == len(processed)


def test_sums_are_64_bit_and_int32_is_refused_when_a_row_does_not_fit():
    """Special tokens only, assembled on the device with no segments: three specials that special_offs declares as 2^30
    bytes each in three rows of three.  The global sum passes 2^32 and rows pass 2^31; the output is 9 x 2 elements."""
    torch = _torch()
    nat = _native()
    V = nat.vocab_size
    res = nat.assemble(None, np.array([0, 3, 6, 9], np.uint64), np.array([0, 1, 2, 2, 2, 2, 1, 0, 1], np.int32), 3)
    assert res.ids().tolist() == [V, V + 1, V + 2, V + 2, V + 2, V + 2, V + 1, V, V + 1]
    sf, so = np.zeros(0, np.uint8), np.array([0, G, 2 * G, 3 * G], np.uint64)
    dev = torch.device("cuda", res.device)
    want = [[0, G], [G, 2 * G], [2 * G, 3 * G]] * 3
    assert tensors.to_spans(res, nat, (sf, so), "byte", torch.int64).tolist() == want
    got = tensors.to_padded_spans(res, nat, (sf, so), "byte", torch.int64, max_length=3, bos_id=1, padding_side="left")
    assert got.tolist() == [[[0, 0], want[0], want[1]]] * 3
    for padded in (False, True):
        out = torch.full((3, 3, 2) if padded else (9, 2), POISON, dtype=torch.int32, device=dev)
        with pytest.raises(tgx.TokenGeeXError) as e:
            if padded:
                tensors.pad_spans_into(res, nat, out, (sf, so), row_len=3)
            else:
                tensors.spans_into(res, nat, out, (sf, so))
        assert e.value.status == _lib.ERR_UNSUPPORTED and (out == POISON).all()    # and nothing was written
    so_fit = np.array([0, G // 2, G, G + G // 2 - 1], np.uint64)     # every row is below 2^31
    got = tensors.to_spans(res, nat, (sf, so_fit), "byte", torch.int32)
    assert got[3:6].tolist() == [[0, G // 2 - 1], [G // 2 - 1, G - 2], [G - 2, G + G // 2 - 3]]
    res.free()


def test_rows_without_tokens():
    torch = _torch()
    nat = _native()
    res = nat.encode_batch_flat(*tgx.pack([b"", b"", b""]))     # T = 0: the padded form is filled with 0
    assert res.num_samples == 3 and res.num_tokens == 0
    assert tensors.to_spans(res, nat).shape == (0, 2)
    out = torch.full((3, 4, 2), POISON, dtype=torch.int32, device=torch.device("cuda", res.device))
    tensors.pad_spans_into(res, nat, out, row_len=4, bos_id=1, eos_id=2)
    assert (out == 0).all()
    res.free()
    res = nat.assemble(None, np.zeros(1, np.uint64), np.zeros(0, np.int32), 0)     # S = 0
    assert tensors.to_spans(res, nat).shape == (0, 2) and tensors.to_padded_spans(res, nat, max_length=5).shape == (0, 5, 2)
    res.free()


def test_refused_before_anything_is_queued():
    torch = _torch()
    res, ids, offs = _source("encode")
    nat = _native()
    dev = torch.device("cuda", res.device)
    T, S = res.num_tokens, res.num_samples
    none = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    good = torch.full((T, 2), POISON, dtype=torch.int32, device=dev)
    # a result from another model with a larger vocabulary
    toks, scores, _ = synth.load_spec_vocab(32000)
    bigger = tgx.NativeModel(list(toks) + [b"zzzz-extra"], np.append(np.asarray(scores, np.float64), -20.0))
    other = bigger.encode_batch_flat(*tgx.pack([b"some text"]))
    dest = torch.full((other.num_tokens, 2), POISON, dtype=torch.int32, device=dev)
    with pytest.raises(tgx.TokenGeeXError) as e:
        nat.result_spans(other, *none, dest.data_ptr())
    assert e.value.status == _lib.ERR_INVALID and (dest == POISON).all()
    bigger.result_spans(other, *none, dest.data_ptr())     # its own model takes it
    assert (dest != POISON).all()
    other.free()
    # a destination on the host, NULL, unknown flags, a side flag in the flat form, a row length below A
    host = np.empty(S * 8 * 2, np.int32)
    for call in (lambda: nat.result_spans(res, *none, host.ctypes.data), lambda: nat.result_pad_spans(res, *none, 8, host.ctypes.data),
                 lambda: nat.result_spans(res, *none, 0), lambda: nat.result_pad_spans(res, *none, 8, 0),
                 lambda: nat.result_spans(res, *none, good.data_ptr(), flags=64),
                 lambda: nat.result_spans(res, *none, good.data_ptr(), flags=_lib.LAYOUT_PAD_LEFT),
                 lambda: nat.result_pad_spans(res, *none, 0, good.data_ptr()),
                 lambda: nat.result_pad_spans(res, *none, 1, good.data_ptr(), bos_id=1, eos_id=2),
                 lambda: nat.result_pad_spans(res, *none, 8, good.data_ptr(), bos_id=2**31)):
        with pytest.raises(tgx.TokenGeeXError) as e:
            call()
        assert e.value.status == _lib.ERR_INVALID, e.value
    # the torch layer checks its destination as the layouts do
    for bad, exc in [(torch.empty((T, 2), dtype=torch.int32), ValueError), (torch.empty((T - 1, 2), dtype=torch.int32, device=dev), ValueError),
                     (torch.empty((T, 2), dtype=torch.int16, device=dev), ValueError), (torch.empty((2, T), dtype=torch.int32, device=dev).t(), ValueError),
                     (np.empty((T, 2), np.int32), TypeError)]:
        with pytest.raises(exc):
            tensors.spans_into(res, nat, bad)
    with pytest.raises(ValueError):
        tensors.pad_spans_into(res, nat, torch.empty((S, 7, 2), dtype=torch.int32, device=dev), row_len=8)
    with pytest.raises(ValueError):
        tensors.spans_into(res, nat, good, unit="word")
    assert (good == POISON).all()
    tensors.spans_into(res, nat, good)     # and the library still works
    assert np.array_equal(good.cpu().numpy(), _want_flat("encode", "byte"))


def test_on_a_side_stream_the_tensor_is_usable_at_once():
    torch = _torch()
    res, ids, offs = _source("encode")
    nat = _native()
    before = torch.cuda.current_device()
    side = torch.cuda.Stream(torch.device("cuda", res.device))
    with torch.cuda.stream(side):
        sp = tensors.to_spans(res, nat, unit="char")
        total = sp.sum()            # used at once, with no synchronisation of the caller's
        q = tensors.to_padded_spans(res, nat, unit="byte", max_length=64, eos_id=2)
        ptotal = q.sum()
    w = _want_flat("encode", "char")
    assert int(total) == int(w.sum())
    want = sc.padded(ids, offs, sc.vocab_lookup(_spec_tokens()), "byte", 64, None, 2, flat_spans=_want_flat("encode", "byte"))
    assert int(ptotal) == int(want.sum()) and torch.cuda.current_device() == before


@functools.lru_cache(maxsize=None)
def _byte_model():
    toks = [bytes([b]) for b in range(256)]
    return tgx.NativeModel(toks, np.full(256, -1.0)), _lib.pack(toks)


def _pattern_rows_against_the_twin(offs):
    """rows of tests/past_cap.py's pattern over one-byte tokens, the character unit, against the host twin"""
    torch = _torch()
    nat, (vf, vo) = _byte_model()
    ids = (np.arange(int(offs[-1]), dtype=np.uint64) * 7 % 256).astype(np.uint32)
    want = _lib.spans_host(vf, vo, 256, np.zeros(0, np.uint8), np.zeros(1, np.uint64), 0, ids, offs, unit="char", dtype=np.int32)
    assert want.shape == (int(offs[-1]), 2)
    res = _lib.NativeResult.from_ids(ids, offs, 256)
    try:
        got = tensors.to_spans(res, nat, unit="char", dtype=torch.int32).cpu().numpy()
    finally:
        res.free()
    assert np.array_equal(got, want)


def test_the_second_trip_of_the_strided_tile_loop():
    """T = 2048 tiles + one tile + 1 tokens: blocks 0 and 1 of span_flat_kernel take a second tile"""
    offs = past_cap.offsets(2048, 1024)
    assert int(offs[-1]) == past_cap.n_out(2048, 1024)
    _pattern_rows_against_the_twin(offs)


@pytest.mark.parametrize("n_tokens", past_cap.edge_sizes(4, 1024))
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_tokens):
    """T = 0, 1, a thread's slot of 4 pairs and the tile of 1024, each less one, full and one over"""
    _pattern_rows_against_the_twin(past_cap.edge_offsets(n_tokens))
