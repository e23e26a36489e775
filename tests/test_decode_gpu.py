"""Ids in HBM decoded to UTF-8 text in HBM (tgx_decode_result / tgx_decode_padded, csrc/decode.hip).  The offsets form is
compared with the existing host decode (tgx_decode_batch) over the result's ids copied to the host, the padded form with
that or with the plain restatement in tests/decode_checker.py; the number of replacement characters with the host twin,
which tests/test_decode_cpu.py checks without a device.  Everything is compared exactly.

The results are real: encode and sampling over test_assemble_gpu.py's corpus (empty rows at the start, in the middle and at
the end, one row of 70 000 bytes: about 17 of the fill kernel's 4096-byte tiles) and results assembled with special tokens."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import decode_checker as dc
import past_cap

N_SPECIALS = 6
SPECIALS = ["<|endoftext|>", "<|fim", "<|fim|>", "<pad>", "<s>", "</s>"]


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _texts():
    """test_assemble_gpu.py's corpus, built the same way"""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    return [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]


@functools.lru_cache(maxsize=None)
def _spec_vocab():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return list(toks), np.asarray(scores, np.float64)


class Model:
    """a NativeModel with its vocabulary and special tokens in the batch format"""

    def __init__(self, tokens, scores, specials):
        self.tokens, self.specials = list(tokens), list(specials)
        self.nat = tgx.NativeModel(self.tokens, scores)
        self.vf, self.vo = _lib.pack(self.tokens)
        self.sf, self.so = _lib.pack(self.specials)
        self.V, self.NS = len(self.tokens), len(self.specials)

    def host(self, ids, offs, inc):
        return _lib.decode_batch_flat(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, inc)

    def twin(self, ids, offs, inc, **kw):
        return _lib.decode_rows_host(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, include_special=inc, **kw)

    def decode(self, res, inc, stream=0):
        return self.nat.decode_result(res, self.sf, self.so, inc, stream)

    def decode_tensor(self, t, inc, **kw):
        return tensors.decode_padded(self.nat, t, special_flat=self.sf, special_offs=self.so, include_special=inc, **kw)


@functools.lru_cache(maxsize=None)
def _spec():
    toks, scores = _spec_vocab()
    return Model(toks, scores, [s.encode() for s in SPECIALS])


def _take(text):
    """-> (bytes, offsets, num_replaced) of a NativeText, which is freed"""
    try:
        assert text.num_bytes == int(text.offsets()[-1]) and text.num_rows == text.offsets().size - 1
        return text.bytes(), text.offsets(), text.num_replaced
    finally:
        text.free()


def _plan(items, sample_sizes):
    assert sum(sample_sizes) == len(items)
    seg_offs = np.zeros(len(sample_sizes) + 1, np.uint64)
    np.cumsum(sample_sizes, out=seg_offs[1:])
    return seg_offs, np.asarray(items, np.int32).reshape(-1)


def _spread(K, S):
    return np.diff(np.linspace(0, K, S + 1).astype(np.int64)).tolist()


@functools.lru_cache(maxsize=None)
def _source(name):
    """-> (NativeResult, its ids, its offsets); computed once, never changed"""
    m = _spec()
    flat, offs = tgx.pack(_texts())
    if name == "encode":
        res = m.nat.encode_batch_flat(flat, offs)
    elif name == "sample":
        res = m.nat.encode_batch_sample_flat(flat, offs, 0.5, 3)
    else:   # the encode result's rows as segments between runs of 3000 special tokens
        segs = _source("encode")[0]
        E = segs.num_samples
        run = [k % N_SPECIALS for k in range(3000)]
        runs = run + [-1] * (E // 2) + run[::-1] + [-1] * (E - E // 2) + run
        res = m.nat.assemble(segs, *_plan(runs, _spread(len(runs), 13)), N_SPECIALS)
    return res, res.ids(), res.offsets()


def _check_against_host(m, res, ids, offs, inc, key=None):
    got, got_offs, n_rep = _take(m.decode(res, inc))
    want, want_offs = m.host(ids, offs, inc)
    assert np.array_equal(got_offs, want_offs), key
    assert np.array_equal(got, want), key
    assert n_rep == m.twin(ids, offs, inc)[2], key
    return got, got_offs, n_rep


# ---- the offsets form ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("include_special", [False, True])
@pytest.mark.parametrize("name", ["encode", "sample", "assembled"])
def test_results_against_the_host_decode(name, include_special):
    m = _spec()
    res, ids, offs = _source(name)
    n = np.diff(offs.astype(np.int64))
    if name != "assembled":
        assert n.max() > 16 * 1024 and n[0] == n[1] == n[-1] == 0 and (n == 0).sum() >= 6
    else:
        assert res.vocab_size == m.V + N_SPECIALS and (ids[:3000] >= m.V).all() and ids.size > _source("encode")[1].size + 8000
    got, got_offs, n_rep = _check_against_host(m, res, ids, offs, include_special, name)
    assert got.size > 160_000 and n_rep == 0            # the corpus is UTF-8, and no row end or special token cuts a character
    assert (got >= 0x80).sum() > 1000                   # ... with multi-byte characters in it
    if name != "assembled":
        assert got.tobytes() == b"".join(_texts())
    # the source is only read: it is the same afterwards, and usable again
    assert np.array_equal(res.ids(), ids) and np.array_equal(res.offsets(), offs)
    _check_against_host(m, res, ids, offs, include_special, name)


def test_degenerate_results():
    m = _spec()
    none = m.nat.assemble(None, np.zeros(1, np.uint64), np.zeros(0, np.int32), N_SPECIALS)    # S = 0
    empty = m.nat.encode_batch_flat(*tgx.pack([b"", b"", b""]))                              # rows without ids
    for res, S in ((none, 0), (empty, 3)):
        assert res.num_samples == S and res.num_tokens == 0
        got, got_offs, n_rep = _take(m.decode(res, True))
        assert got.size == 0 and got_offs.tolist() == [0] * (S + 1) and n_rep == 0
        res.free()
    only = m.nat.assemble(None, *_plan([4, 5, 3, 0], [2, 0, 1, 1]), N_SPECIALS)     # rows of special tokens only
    assert _take(m.decode(only, True))[0].tobytes() == b"<s></s><pad><|endoftext|>"
    got, got_offs, _ = _take(m.decode(only, False))
    assert got.size == 0 and got_offs.tolist() == [0, 0, 0, 0, 0]
    only.free()


# ---- invalid UTF-8 on the device -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bytes_model():
    return Model([bytes([b]) for b in range(256)], np.full(256, -5.0), [b"<s>", b"\xff\x80<raw>", b""])


@functools.lru_cache(maxsize=None)
def _byte_rows():
    """400 rows of 0 .. 40 bytes of the boundary alphabet and two of 5000, cut into segments with special tokens between
    them -> (assembled NativeResult over a vocabulary of the 256 single bytes, its ids, its offsets)"""
    m = _bytes_model()
    rng = np.random.default_rng(21)
    segments, items, sizes = [], [], []
    for n in [int(x) for x in rng.integers(0, 41, 400)] + [5000, 5000]:
        row = bytes(dc.ALPHABET[i] for i in rng.integers(0, len(dc.ALPHABET), n))
        cuts = sorted(rng.integers(0, n + 1, int(rng.integers(0, 4)) if n < 100 else 60).tolist())
        pieces = [row[a:b] for a, b in zip([0] + cuts, cuts + [n])]
        k0 = len(items)
        for k, piece in enumerate(pieces):
            if k:
                items.append(int(rng.integers(0, m.NS)))
            segments.append(piece)
            items.append(-1)
        sizes.append(len(items) - k0)
    segs = m.nat.encode_batch_flat(*tgx.pack(segments))
    assert np.array_equal(segs.ids(), np.frombuffer(b"".join(segments), np.uint8))   # a byte's id is the byte
    res = m.nat.assemble(segs, *_plan(items, sizes), m.NS)
    segs.free()
    return res, res.ids(), res.offsets()


@pytest.mark.parametrize("include_special", [False, True])
def test_invalid_utf8_is_replaced_on_the_device(include_special):
    m = _bytes_model()
    res, ids, offs = _byte_rows()
    got, got_offs, n_rep = _check_against_host(m, res, ids, offs, include_special)
    assert n_rep > 1000
    # every run came out as UTF-8; the one special token that is not UTF-8 goes out as it is, so the text is cut at it first
    raw = b"\xff\x80<raw>"
    rows = ["".join(p.decode("utf-8") for p in got[int(got_offs[i]):int(got_offs[i + 1])].tobytes().split(raw))
            for i in range(res.num_samples)]
    assert (raw in got.tobytes()) == include_special
    # both ways through the second copy: replacement characters, and multi-byte characters that stay
    assert any(any(ord(c) > 0x7F and c != dc.REPLACEMENT for c in r) for r in rows) and any(dc.REPLACEMENT in r for r in rows)
    if include_special:
        assert b"\xff\x80<raw>" in got.tobytes()    # a special token's bytes go out as they are


# ---- the padded form -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_padded_tensors(side, dtype):
    torch = _torch()
    m = _spec()
    res, ids, offs = _source("assembled")
    pad = m.V + 3
    td = getattr(torch, dtype)
    for inc in (False, True):
        want, want_offs = m.host(ids, offs, inc)
        # nothing truncated: the decode of the result itself, whichever way the padding is told apart
        out = tensors.to_padded(res, pad_id=m.V + N_SPECIALS + 9, padding_side=side, dtype=td, return_lengths=True)
        calls = {"mask": dict(attention_mask=out["attention_mask"]), "bool mask": dict(attention_mask=out["attention_mask"].bool()),
                 "skip": dict(skip_id=m.V + N_SPECIALS + 9)}    # (an id that would be out of bounds: it is skipped, not checked)
        if side == "right":
            calls["lengths"] = dict(lengths=out["lengths"])
            calls["all three"] = dict(attention_mask=out["attention_mask"], lengths=out["lengths"], skip_id=m.V + N_SPECIALS + 9)
        for name, kw in calls.items():
            got, got_offs, n_rep = _take(m.decode_tensor(out["input_ids"], inc, **kw))
            assert np.array_equal(got_offs, want_offs) and np.array_equal(got, want) and n_rep == 0, (side, dtype, inc, name)
    # truncated rows cut characters: the checker's output over the tensor
    out = tensors.to_padded(res, max_length=61, pad_id=pad, padding_side=side, truncation_side="left" if side == "right" else "right", dtype=td)
    h_ids, h_mask = out["input_ids"].cpu().numpy(), out["attention_mask"].cpu().numpy()
    for inc in (False, True):
        want, want_offs, want_rep = dc.decode_padded(h_ids, m.tokens, m.specials, inc, mask=h_mask)
        got, got_offs, n_rep = _take(m.decode_tensor(out["input_ids"], inc, attention_mask=out["attention_mask"]))
        assert np.array_equal(got_offs, want_offs) and np.array_equal(got, want) and n_rep == want_rep, (side, dtype, inc)
        got, got_offs, n_rep = _take(m.decode_tensor(out["input_ids"], inc, skip_id=pad))   # pad is a special token here: dropped wherever it stands
        want, want_offs, want_rep = dc.decode_padded(h_ids, m.tokens, m.specials, inc, skip_id=pad)
        assert np.array_equal(got_offs, want_offs) and np.array_equal(got, want) and n_rep == want_rep, (side, dtype, inc)


@pytest.mark.parametrize("L", [1, 7, 64, 257])
def test_padded_random_ids_over_long_tokens(L):
    """ids drawn at random over a vocabulary with an empty token and tokens of up to 64 bytes (the spec vocabulary stops at 16,
    the size of a token's slot), characters cut across tokens, invalid bytes and a special token that is not UTF-8"""
    torch = _torch()
    toks = dc.mixed_tokens()
    m = _mixed_model()
    rng = np.random.default_rng(L)
    for S, dtype in ((33, np.int32), (2, np.int64), (600, np.int64)):
        ids = rng.integers(0, m.V + m.NS, (S, L)).astype(dtype)
        lengths = rng.integers(-1, L + 2, S).astype(np.int32)
        mask = (rng.random((S, L)) < 0.8)
        ids[~mask] = -3 if S % 2 else m.V + m.NS     # not live: not checked
        t = torch.from_numpy(ids).cuda()
        for inc in (False, True):
            kw = dict(mask=mask.astype(np.uint8), lengths=lengths)
            want = dc.decode_padded(ids, toks, m.specials, inc, **kw) if S < 100 else m.twin(ids, None, inc, **kw)
            got = _take(m.decode_tensor(t, inc, attention_mask=torch.from_numpy(mask).cuda(), lengths=torch.from_numpy(lengths).cuda()))
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == want[2], (L, S, inc)


@functools.lru_cache(maxsize=None)
def _mixed_model():
    toks = dc.mixed_tokens()
    return Model(toks, -np.arange(1.0, len(toks) + 1), dc.MIXED_SPECIALS)


def test_refusals_before_any_launch():
    torch = _torch()
    m = _spec()
    good = torch.ones((4, 6), dtype=torch.int64, device="cuda")
    for bad, exc in ((torch.ones((4, 12), dtype=torch.int64, device="cuda")[:, ::2], ValueError), (good.cpu(), ValueError),
                     (good.to(torch.int16), ValueError), (good.float(), ValueError), (good[0], ValueError), (good.cpu().numpy(), TypeError)):
        with pytest.raises(exc):
            m.decode_tensor(bad, True)
    for kw in (dict(attention_mask=torch.ones((4, 5), dtype=torch.uint8, device="cuda")), dict(attention_mask=torch.ones((4, 6), dtype=torch.uint8)),
               dict(attention_mask=torch.ones((4, 6), dtype=torch.int32, device="cuda")), dict(lengths=torch.ones(4, dtype=torch.int64, device="cuda")),
               dict(lengths=torch.ones(3, dtype=torch.int32, device="cuda")), dict(lengths=torch.ones(4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            m.decode_tensor(good, True, **kw)
    # the C entry itself: host memory where device memory belongs
    host = np.ones((4, 6), np.int64)
    for kw in (dict(ids_ptr=host.ctypes.data), dict(ids_ptr=good.data_ptr(), mask_ptr=host.ctypes.data), dict(ids_ptr=good.data_ptr(), lengths_ptr=host.ctypes.data)):
        with pytest.raises(tgx.TokenGeeXError) as e:
            m.nat.decode_padded(n_rows=4, row_len=6, i64=True, special_flat=m.sf, special_offs=m.so, **kw)
        assert e.value.status == _lib.ERR_INVALID and "not device memory" in str(e.value)
    with pytest.raises(tgx.TokenGeeXError) as e:    # a result of more ids than the model and its special tokens have
        m.nat.decode_result(_source("assembled")[0], m.sf[:0], m.so[:1], True)
    assert e.value.status == _lib.ERR_INVALID
    assert _take(m.decode_tensor(good, True))[0].tobytes() == m.tokens[1] * 24


# ---- out of bounds ---------------------------------------------------------------------------------------------------------

def test_out_of_bounds_on_the_device():
    torch = _torch()
    m = _spec()
    rng = np.random.default_rng(8)
    bad = m.V + m.NS
    rows = rng.integers(0, bad, (12, 30))
    rows[5, 7] = rows[5, 20] = rows[9, 0] = bad
    for dtype in (np.int32, np.int64):
        ids = rows.astype(dtype)
        with pytest.raises(tgx.TokenGeeXError) as want:
            m.host(*_flat(ids), True)
        with pytest.raises(tgx.TokenGeeXError) as got:
            m.decode_tensor(torch.from_numpy(ids).cuda(), True)
        assert got.value.status == want.value.status == _lib.ERR_TOKEN_ID_OOB and str(got.value) == str(want.value) == f"token id {bad} is out of bounds"
        assert (got.value.sample, got.value.pos) == (want.value.sample, want.value.pos) == (5, bad)
        ids[5, 7] = bad + 4      # the first of the lowest row is named, not the lowest value
        with pytest.raises(tgx.TokenGeeXError) as got:
            m.decode_tensor(torch.from_numpy(ids).cuda(), False)
        assert (got.value.sample, got.value.pos) == (5, bad + 4)
    for value in (-1, 2 ** 32 + 3):
        ids = rows.astype(np.int64)
        ids[5, 7] = value
        with pytest.raises(tgx.TokenGeeXError) as got:
            m.decode_tensor(torch.from_numpy(ids).cuda(), True)
        assert got.value.status == _lib.ERR_TOKEN_ID_OOB and str(got.value) == f"token id {value} is out of bounds"
        assert (got.value.sample, got.value.pos) == (5, value % 2 ** 64)
    # a good call afterwards still works
    rows[5, 7] = rows[5, 20] = rows[9, 0] = 11
    ids = rows.astype(np.int64)
    got, got_offs, _ = _take(m.decode_tensor(torch.from_numpy(ids).cuda(), True))
    want, want_offs = m.host(*_flat(ids), True)
    assert np.array_equal(got, want) and np.array_equal(got_offs, want_offs)


def _flat(ids2d):
    S, L = ids2d.shape
    return np.ascontiguousarray(ids2d.reshape(-1), np.uint32), np.arange(S + 1, dtype=np.uint64) * L


# ---- ordering ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["default stream", "side stream"])
def test_ordered_after_the_work_that_produces_the_ids(where):
    """The id tensor is written on torch's current stream by ops queued right before the call (a long chain of products, then
    the copy into the tensor): the decode must start after them.  The event shows that the work was still pending."""
    torch = _torch()
    m = _spec()
    res, ids, offs = _source("encode")
    dev = torch.device("cuda", res.device)
    src = tensors.to_padded(res, max_length=96, pad_id=m.V + 3, dtype=torch.int64)
    want = _take(m.decode_tensor(src["input_ids"], True, attention_mask=src["attention_mask"]))
    a = torch.ones((4096, 4096), device=dev)
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    torch.cuda.synchronize(dev)

    def run():
        t = torch.full_like(src["input_ids"], m.V + m.NS)     # out of bounds everywhere until the copy lands
        torch.cuda.current_stream(dev).synchronize()
        for _ in range(40):
            torch.mm(a, a, out=b)
        t.copy_(src["input_ids"])
        ev = torch.cuda.Event()
        ev.record()
        pending = not ev.query()
        got = _take(m.decode_tensor(t, True, attention_mask=src["attention_mask"]))
        assert pending, "the queued work had ended before the call: nothing was tested"
        assert all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2])) and got[2] == want[2]

    if where == "default stream":
        assert torch.cuda.current_stream(dev).cuda_stream == 0
        run()
    else:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream != 0
            run()
        torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)


# ---- Tokenizer level ---------------------------------------------------------------------------------------------------------

def _tokenizer(procs=()):
    toks, scores = _spec_vocab()
    processors = [tgx.CrlfProcessor() if p == "crlf" else tgx.UnicodeProcessor(p) for p in procs]
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors, list(SPECIALS))


def _str_texts():
    body = [t.decode("utf-8", "ignore") for t in _texts()[2:40]]
    texts = ["", "<|endoftext|>", "<s></s><pad><|fim|><|fim", "no special token in here", "a\r\n<s>\r\nb\r\n", "\r\n</s>",
             "é Å<|endoftext|>é", "<|fim|>prefix<|fim>suffix<|fim|middle", ""]
    for k, t in enumerate(body):
        cut = len(t) // 3
        texts.append(t[:cut] + "<|fim|>" + t[cut:2 * cut] + "<s>" * (k % 3) + t[2 * cut:] + ("<|endoftext|>" if k % 2 else ""))
    return texts + ["<pad>", ""]


@pytest.mark.parametrize("procs", [("crlf",), ("nfc",), ()])
def test_tokenizer_decodes_results_and_tensors(procs):
    tk = _tokenizer(procs)
    texts = _str_texts()
    flat, offs = tgx.pack([t.encode("utf-8") for t in texts])
    rows = tk.encode_batch(texts, 0.0)
    res = tk.encode_batch_result_flat(flat, offs, 0.0)
    for flag in (False, True):
        want = tk.decode_batch(rows, flag)
        assert tk.decode_result(res, flag) == want, (procs, flag)
        got, got_offs = tk.decode_result_flat(res, flag)
        assert got.tobytes() == "".join(want).encode("utf-8") and got_offs.size == len(texts) + 1
        text = tk.decode_result_text(res, flag)
        assert (text.num_rows, text.num_bytes, text.num_replaced, text.device) == (len(texts), got.size, 0, res.device)
        assert text.bytes_ptr and text.offsets_ptr
        text.free()
    res.free()
    if not procs:
        assert tk.decode_result(tk.encode_batch_result_flat(flat, offs, 0.0), True) == texts
    out = tk.encode_batch_padded(texts, pad="<pad>", padding_side="left")
    want = tk.decode_batch(rows, False)
    assert tk.decode_tensor(out["input_ids"], False, attention_mask=out["attention_mask"]) == want
    assert tk.decode_tensor(out["input_ids"], False, skip="<pad>") == want      # (excluded special tokens emit nothing anyway)
    assert tk.decode_tensor(out["input_ids"].int(), False, skip=tk.special_token_to_id("<pad>")) == want
    got, got_offs = tk.decode_tensor_flat(out["input_ids"], True, attention_mask=out["attention_mask"])
    assert got.tobytes() == "".join(tk.decode_batch(rows, True)).encode("utf-8")
    with pytest.raises(tgx.TokenGeeXError):
        tk.decode_tensor(out["input_ids"], False, skip="<no such token>")


# ---- retokenize --------------------------------------------------------------------------------------------------------------

def test_retokenize_without_leaving_the_device():
    m = _spec()
    toks, scores = _spec_vocab()
    small = tgx.NativeModel(toks[:-5000], scores[:-5000])
    res, ids, offs = _source("sample")
    text = m.decode(res, False)
    corpus = text.to_corpus()
    host_bytes, host_offs = m.host(ids, offs, False)
    assert (corpus.num_samples, corpus.num_bytes, corpus.device) == (res.num_samples, host_bytes.size, res.device)
    again = small.encode_corpus(corpus)
    want = small.encode_batch_flat(host_bytes, host_offs)
    assert np.array_equal(again.ids(), want.ids()) and np.array_equal(again.offsets(), want.offsets())
    assert again.ids().max() < 27000 and not np.array_equal(again.ids(), _source("encode")[1])
    # the text is still there, and the corpus outlives it
    assert np.array_equal(text.bytes(), host_bytes)
    text.free()
    assert np.array_equal(small.encode_corpus(corpus).ids(), want.ids())
    for h in (corpus, again, want):
        h.free()
    small.free()


# ---- hygiene -----------------------------------------------------------------------------------------------------------------

def test_handles_pool_and_current_device():
    torch = _torch()
    m = _spec()
    res, ids, offs = _source("encode")
    before = torch.cuda.current_device()
    text = m.decode(res, True)
    corpus = text.to_corpus()
    t = tensors.to_padded(res, max_length=8, pad_id=0)
    text2 = m.decode_tensor(t["input_ids"], True, attention_mask=t["attention_mask"])
    assert torch.cuda.current_device() == before
    assert text.bytes().size == text.num_bytes and text.offsets()[-1] == text.num_bytes
    for h in (text, text, text2, corpus, corpus):    # twice is harmless
        h.free()
    tgx.pool_trim(res.device)
    tgx.pool_trim()
    assert torch.cuda.current_device() == before
    _check_against_host(m, res, ids, offs, True)     # and everything still works on fresh buffers


def _pattern_rows_against_the_twin(lens):
    """A row of the pattern (tests/past_cap.py) is an element: a one-byte token, a special token without bytes, and a
    special token of as many bytes as the one longer row has; seven elements to a row; against the host twin"""
    long_len = int(lens.max()) if int(lens.max()) > 1 else 0
    toks = [bytes([b]) for b in range(256)]
    m = Model(toks, np.full(256, -1.0), [b"", bytes(97 + k % 26 for k in range(long_len))])
    ids = (np.arange(lens.size, dtype=np.uint64) * 7 % 26 + 97).astype(np.uint32)
    ids[lens == 0] = 256
    if long_len:
        ids[lens == long_len] = 257
    offs = np.unique(np.append(np.arange(0, lens.size, 7), lens.size)).astype(np.uint64)
    want = m.twin(ids, offs, True)
    assert want[0].size == int(lens.sum()) and want[2] == 0
    res = _lib.NativeResult.from_ids(ids, offs, 258)
    try:
        got = _take(m.decode(res, True))
    finally:
        res.free()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == 0


def test_the_second_trip_of_the_strided_tile_loop():
    """2048 tiles + one tile + 1 raw bytes: blocks 0 and 1 of decode_fill_kernel take a second tile; one special token has
    more than a tile of bytes"""
    lens = past_cap.lengths(2048, 4096)
    assert int(lens.sum()) == past_cap.n_out(2048, 4096) and int(lens.max()) > 4096
    _pattern_rows_against_the_twin(lens)


@pytest.mark.parametrize("n_raw", past_cap.edge_sizes(16, 4096))
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_raw):
    """0 and 1 raw bytes, a thread's slot of 16 bytes and the tile of 4096, each less one, full and one over"""
    _pattern_rows_against_the_twin(past_cap.edge_lengths(n_raw))
