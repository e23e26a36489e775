"""Overflow windows on the GPU (tgx_result_window_info / tgx_result_window_pad_device / tgx_result_window_spans_device,
csrc/layout.hip and csrc/spans.hip) against the plain restatement in tests/windows_checker.py.  Everything is compared
exactly: this is integer data movement.

Inputs are real results — encode, sampling, n-best at k = 3 (rows beyond n_found are empty) and a resident corpus — over
~32 KiB of mixed text in samples of up to 2 KiB, empty samples at the start, in the middle and at the end, and one sample
of 12 000 bytes whose row has more than 1024 tokens: at L = 8 it owns several tiles of the fill kernel on its own, while
other tiles hold many rows.  Then the torch layer (tokengeex_amd/tensors.py) and the Tokenizer methods."""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import layout_checker as lc
import past_cap
import spans_checker as sc
import windows_checker as wc

PAD = 7
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]
SIDES = ["right", "left"]
POISON = -77   # what a destination holds before the call: an element the kernel skipped shows
SOURCES = ["encode", "sample", "nbest", "resident"]
BIG = 12_000


def _torch():
    import torch
    return torch


def _tdtype(dt):
    torch = _torch()
    return torch.int64 if dt == np.int64 else torch.int32


@functools.lru_cache(maxsize=None)
def _texts():
    flat, offs = synth.make_corpus(32 << 10, "mixed", max_len=2048, seed_offset=3)
    big, _ = synth.make_corpus(BIG + 4096, "mixed", min_len=BIG, max_len=BIG, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    return [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:BIG])] + rows[half:] + [b""]


@functools.lru_cache(maxsize=None)
def _spec_tokens():
    toks, _, _ = synth.load_spec_vocab(32000)
    return list(toks)


@functools.lru_cache(maxsize=None)
def _native():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.NativeModel(list(toks), np.asarray(scores, np.float64))


@functools.lru_cache(maxsize=None)
def _source(name):
    """-> (NativeResult, ids, offs) of a real pass over the corpus"""
    nat = _native()
    flat, offs = tgx.pack(_texts())
    if name == "encode":
        res = nat.encode_batch_flat(flat, offs)
    elif name == "sample":
        res = nat.encode_batch_sample_flat(flat, offs, 0.5, 3)
    elif name == "nbest":
        res, _, nf = nat.encode_batch_nbest_flat(flat, offs, 3)
        assert res.num_samples == 3 * len(_texts()) and int(nf[0]) == 1
    else:
        corpus = tgx.NativeCorpus(flat, offs)
        res = nat.encode_corpus(corpus)
        res._corpus = corpus
    ids, oo = res.ids(), res.offsets()
    n = np.diff(oo.astype(np.int64))
    k = 3 if name == "nbest" else 1
    big_row = k * _texts().index(max(_texts(), key=len))
    assert n[big_row] > 1024 and (n == 0).sum() >= 6 and n[0] == 0 and n[-1] == 0
    ids.setflags(write=False)
    oo.setflags(write=False)
    return res, ids, oo


@functools.lru_cache(maxsize=None)
def _want_flat(source, unit):
    """the checker's flat spans of a source, computed once"""
    _, ids, offs = _source(source)
    w = sc.flat(ids, offs, sc.vocab_lookup(_spec_tokens()), unit)
    w.setflags(write=False)
    return w


def _dev(res):
    return _torch().device("cuda", res.device)


def _shapes(a):
    """(L, stride): room 1; L = 8 with no overlap, some, and the most (step 1); an odd L; a usual window over short rows"""
    room8 = 8 - a
    return [(a + 1, 0), (8, 0), (8, room8 // 2), (8, room8 - 1), (13, 5), (512, 64)]


def _run(res, L, stride, bos, eos, pside, tside, dt, W=None):
    """window_into over poisoned destinations -> the five outputs as numpy"""
    torch = _torch()
    dev = _dev(res)
    flags = _lib.layout_flags(pside, tside, dt)
    if W is None:
        W = res.window_info(L, stride, bos_id=bos, eos_id=eos, flags=flags)
    out = torch.full((W, L), POISON, dtype=_tdtype(dt), device=dev)
    mask = torch.full((W, L), 9, dtype=torch.uint8, device=dev)
    i32 = [torch.full((W,), POISON, dtype=torch.int32, device=dev) for _ in range(3)]
    got = tensors.window_into(res, out, mask, *i32, row_len=L, stride=stride, pad_id=PAD, n_windows=W, bos_id=bos, eos_id=eos,
                              padding_side=pside, truncation_side=tside)
    assert got == W
    return [t.cpu().numpy() for t in [out, mask] + i32]


def _same(got, want, key):
    for name, g, w in zip(("ids", "mask", "lengths", "row", "first"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (key, name)


@pytest.mark.parametrize("source", SOURCES)
def test_windows_against_the_checker(source):
    """The full product of options on the encode source; on the other three both dtypes, two bos / eos choices and the
    sides turned together."""
    res, ids, offs = _source(source)
    if source == "encode":
        options = list(itertools.product(BOS_EOS, SIDES, SIDES, [np.int32, np.int64]))
    else:
        options = [(be, s, s, dt) for be, s, dt in itertools.product([(None, None), (1, 2)], SIDES, [np.int32, np.int64])]
    for (bos, eos), pside, tside, dt in options:
        a = (bos is not None) + (eos is not None)
        shapes = _shapes(a) if source == "encode" else [(8, (8 - a) // 2), (13, 0)]
        for L, stride in shapes:
            key = (source, bos, eos, pside, tside, dt, L, stride)
            want = wc.windows(ids, offs, L, stride, PAD, bos, eos, pside == "left", tside == "left", dt)
            W = res.window_info(L, stride, bos_id=bos, eos_id=eos)
            assert W == want[0].shape[0] == wc.n_windows(offs, L, stride, bos, eos), key
            _same(_run(res, L, stride, bos, eos, pside, tside, dt, W), want, key)
    # the per-row form of the checker itself on one setting, where the long row owns several tiles
    got = _run(res, 8, 3, 1, None, "right", "right", np.int32)
    _same(got, wc.windows_by_row(ids, offs, 8, 3, PAD, 1, None), source)
    per_tile = [len(np.unique(got[3][w:w + 1024 // 8])) for w in range(0, len(got[3]), 1024 // 8)]
    assert np.bincount(got[3]).max() * 8 > 2 * 1024 and min(per_tile) == 1 and max(per_tile) >= 3   # tiles of one row, and tiles of several


@pytest.mark.parametrize("source", SOURCES)
def test_window_spans_against_the_checker_and_the_ids(source):
    """Both units; every pair lines up with the id of the same call: a kept token's cell holds that token's id and span,
    every other cell (0, 0)."""
    torch = _torch()
    res, ids, offs = _source(source)
    nat = _native()
    dev = _dev(res)
    T = int(offs[-1])
    kinds = list(itertools.product(["byte", "char"], [np.int32, np.int64]))
    if source == "encode":
        options = list(itertools.product(BOS_EOS, SIDES, SIDES))
    else:
        options = [((1, 2), "right", "left"), ((None, None), "left", "right")]
    turn = 0
    for (bos, eos), pside, tside in options:
        a = (bos is not None) + (eos is not None)
        for L, stride in [(a + 1, 0), (8, (8 - a) // 2), (13, 5)]:
            unit, dt = kinds[(turn + turn // 4) % 4]
            turn += 1
            key = (source, unit, dt, bos, eos, pside, tside, L, stride)
            W = res.window_info(L, stride, bos_id=bos, eos_id=eos)
            out = torch.full((W, L, 2), POISON, dtype=_tdtype(dt), device=dev)
            assert tensors.window_spans_into(res, nat, out, row_len=L, stride=stride, n_windows=W, unit=unit, bos_id=bos, eos_id=eos,
                                             padding_side=pside, truncation_side=tside) == W
            got = out.cpu().numpy()
            want = wc.window_spans(offs, _want_flat(source, unit), L, stride, bos, eos, pside == "left", tside == "left", dt)
            assert got.dtype == want.dtype and np.array_equal(got, want), key
            # element for element with the ids: cell -> token index through the checker's layout of the indices
            where = wc.windows(np.arange(T), offs, L, stride, T, T if bos is not None else None, T if eos is not None else None,
                               pside == "left", tside == "left", np.int64)[0]
            got_ids = _run(res, L, stride, bos, eos, pside, tside, dt, W)[0]
            tok = where < T
            assert np.array_equal(got_ids[tok], ids[where[tok]].astype(dt)), key
            assert np.array_equal(got[tok], _want_flat(source, unit)[where[tok]].astype(dt)) and not got[~tok].any(), key
    got = tensors.to_window_spans(res, nat, unit="char", dtype=torch.int32, max_length=16, stride=4, bos_id=1)
    want = wc.window_spans(offs, _want_flat(source, "char"), 16, 4, 1, None, dtype=np.int32)
    assert got.dtype == torch.int32 and got.device == dev and np.array_equal(got.cpu().numpy(), want)


def test_odd_sizes_leave_a_short_last_group():
    res, ids, offs = _source("encode")
    L = 13
    stride = next(s for s in range(L) if wc.n_windows(offs, L, s) % 2 == 1)
    W = wc.n_windows(offs, L, stride)
    assert (W * L) % 4 in (1, 3)
    for dt in (np.int32, np.int64):
        _same(_run(res, L, stride, None, None, "right", "right", dt), wc.windows(ids, offs, L, stride, PAD, dtype=dt), (dt, stride))
    L = 7
    stride = next(s for s in range(L - 2) if wc.n_windows(offs, L, s, 1, 2) % 2 == 1)
    _same(_run(res, L, stride, 1, 2, "left", "left", np.int32), wc.windows(ids, offs, L, stride, PAD, 1, 2, True, True), stride)


def test_optional_outputs_and_unaligned_destinations():
    """Raw pointers (NativeResult.window_pad_device / window_spans_device): every optional output left out; destinations
    sliced one element in, which are not 16-byte aligned (the element-wide store path of the kernels); the library's
    stream (stream = 0), which is ordered after torch's fills on the null stream."""
    torch = _torch()
    res, ids, offs = _source("encode")
    nat = _native()
    dev = _dev(res)
    none = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    L, stride = 9, 2
    W = res.window_info(L, stride, bos_id=1)
    for dt, shift in itertools.product([np.int32, np.int64], [0, 1]):
        flags = _lib.layout_flags(dtype=dt)
        want = wc.windows(ids, offs, L, stride, PAD, 1, None, dtype=dt)
        buf = torch.full((W * L + 8,), POISON, dtype=_tdtype(dt), device=dev)
        mbuf = torch.full((W * L + 8,), 9, dtype=torch.uint8, device=dev)
        ibuf = [torch.full((W + 8,), POISON, dtype=torch.int32, device=dev) for _ in range(3)]
        out, mask = buf[shift:shift + W * L], mbuf[shift:shift + W * L]
        i32 = [b[shift:shift + W] for b in ibuf]
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        res.window_pad_device(L, stride, PAD, W, out.data_ptr(), bos_id=1, flags=flags)
        assert np.array_equal(out.cpu().numpy().reshape(W, L), want[0])
        assert (buf[:shift] == POISON).all() and (buf[shift + W * L:] == POISON).all()      # nothing beside the destination
        assert (mbuf == 9).all() and all((b == POISON).all() for b in ibuf)                 # nothing that was not asked for
        buf.fill_(POISON)
        res.window_pad_device(L, stride, PAD, W, out.data_ptr(), mask_ptr=mask.data_ptr(), lengths_ptr=i32[0].data_ptr(),
                              window_row_ptr=i32[1].data_ptr(), window_first_ptr=i32[2].data_ptr(), bos_id=1, flags=flags)
        _same([out.cpu().numpy().reshape(W, L), mask.cpu().numpy().reshape(W, L)] + [t.cpu().numpy() for t in i32], want, (dt, shift))
        assert (mbuf[:shift] == 9).all() and (mbuf[shift + W * L:] == 9).all()
        assert all((b[:shift] == POISON).all() and (b[shift + W:] == POISON).all() for b in ibuf)

        sbuf = torch.full((W * L * 2 + 8,), POISON, dtype=_tdtype(dt), device=dev)
        sp = sbuf[shift:shift + W * L * 2]
        res.window_spans_device(nat, *none, L, stride, W, sp.data_ptr(), bos_id=1, flags=_lib.span_flags("char", dt))
        want_sp = wc.window_spans(offs, _want_flat("encode", "char"), L, stride, 1, None, dtype=dt)
        assert np.array_equal(sp.cpu().numpy().reshape(W, L, 2), want_sp)
        assert (sbuf[:shift] == POISON).all() and (sbuf[shift + W * L * 2:] == POISON).all()


def test_errors_leave_the_destinations_untouched():
    torch = _torch()
    res, ids, offs = _source("encode")
    nat = _native()
    dev = _dev(res)
    none = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    L, stride = 8, 2
    W = res.window_info(L, stride, bos_id=1, eos_id=2)
    assert W == wc.n_windows(offs, L, stride, 1, 2) > res.num_samples
    out = torch.full((W + 4, L), POISON, dtype=torch.int32, device=dev)
    mask = torch.full((W + 4, L), 9, dtype=torch.uint8, device=dev)
    i32 = [torch.full((W + 4,), POISON, dtype=torch.int32, device=dev) for _ in range(3)]
    spans = torch.full((W + 4, L, 2), POISON, dtype=torch.int32, device=dev)
    host = np.empty(W * L, np.int32)

    def pad(n_windows=W, L=L, stride=stride, ids_ptr=None, **kw):
        kw = {"bos_id": 1, "eos_id": 2, "mask_ptr": mask.data_ptr(), "lengths_ptr": i32[0].data_ptr(), "window_row_ptr": i32[1].data_ptr(),
              "window_first_ptr": i32[2].data_ptr(), **kw}
        res.window_pad_device(L, stride, PAD, n_windows, out.data_ptr() if ids_ptr is None else ids_ptr, **kw)

    def span(n_windows=W, L=L, stride=stride, **kw):
        kw = {"bos_id": 1, "eos_id": 2, **kw}
        res.window_spans_device(nat, *none, L, stride, n_windows, spans.data_ptr(), **kw)

    calls = [lambda: pad(W + 1), lambda: pad(W - 1), lambda: pad(res.num_samples), lambda: pad(0),    # not the W that is computed
             lambda: pad(stride=6), lambda: pad(stride=7), lambda: pad(stride=2**32 - 1),              # stride >= room = 6
             lambda: pad(L=2), lambda: pad(L=0), lambda: pad(L=1, stride=0, eos_id=None),              # no room for a token
             lambda: pad(flags=64), lambda: pad(flags=_lib.SPAN_CHARS), lambda: pad(bos_id=2**31),
             lambda: pad(ids_ptr=host.ctypes.data), lambda: pad(window_row_ptr=host.ctypes.data),      # not device memory
             lambda: span(W + 1), lambda: span(0), lambda: span(stride=6), lambda: span(L=2), lambda: span(flags=64),
             lambda: res.window_info(8, 6, bos_id=1, eos_id=2), lambda: res.window_info(2, 0, bos_id=1, eos_id=2),
             lambda: res.window_info(8, 2, flags=64)]
    for k, call in enumerate(calls):
        with pytest.raises(tgx.TokenGeeXError) as e:
            call()
        assert e.value.status == _lib.ERR_INVALID, (k, e.value)
    with pytest.raises(tgx.TokenGeeXError) as e:
        res.window_pad_device(L, stride, PAD, W, 0)          # NULL where something would be written
    assert e.value.status == _lib.ERR_INVALID
    assert (out == POISON).all() and (mask == 9).all() and all((t == POISON).all() for t in i32) and (spans == POISON).all()
    # the torch layer checks its tensors against W before anything is launched
    with pytest.raises(ValueError):
        tensors.window_into(res, out[:W - 1], row_len=L, stride=stride, pad_id=PAD, bos_id=1, eos_id=2)
    with pytest.raises(ValueError):
        tensors.window_into(res, out, window_row=i32[1][:W - 1], row_len=L, stride=stride, pad_id=PAD, bos_id=1, eos_id=2)
    with pytest.raises(ValueError):
        tensors.window_spans_into(res, nat, spans[:W - 1], row_len=L, stride=stride, bos_id=1, eos_id=2)
    with pytest.raises(TypeError):
        tensors.to_windows(res, max_length=None, pad_id=PAD)
    assert (out == POISON).all() and (spans == POISON).all()
    # and the library still works
    pad()
    span()
    want = wc.windows(ids, offs, L, stride, PAD, 1, 2)
    assert np.array_equal(out[:W].cpu().numpy(), want[0]) and (out[W:] == POISON).all()
    assert np.array_equal(i32[1][:W].cpu().numpy(), want[3]) and (i32[1][W:] == POISON).all()
    assert np.array_equal(spans[:W].cpu().numpy(), wc.window_spans(offs, _want_flat("encode", "byte"), L, stride, 1, 2, dtype=np.int32))
    assert (spans[W:] == POISON).all()


def test_no_long_row_is_the_padded_form():
    """L above the longest row: W = S and every output is that of the padded calls; and window 0 of every row is the padded
    row at a short L."""
    torch = _torch()
    res, ids, offs = _source("sample")
    nat = _native()
    S = res.num_samples
    L = res.layout_info(1, 2)[0] + 3
    for stride in (0, L - 3):
        w = tensors.to_windows(res, max_length=L, stride=stride, pad_id=PAD, bos_id=1, eos_id=2, padding_side="left", return_lengths=True)
        p = tensors.to_padded(res, max_length=L, pad_id=PAD, bos_id=1, eos_id=2, padding_side="left", return_lengths=True)
        assert w["input_ids"].shape == (S, L) and all(torch.equal(w[k], p[k]) for k in p)
        assert torch.equal(w["overflow_to_sample_mapping"], torch.arange(S, dtype=torch.int32, device=w["input_ids"].device))
        assert not w["window_first"].any()
        ws = tensors.to_window_spans(res, nat, unit="char", max_length=L, stride=stride, bos_id=1, eos_id=2, padding_side="left")
        assert torch.equal(ws, tensors.to_padded_spans(res, nat, unit="char", max_length=L, bos_id=1, eos_id=2, padding_side="left"))
    for tside in SIDES:
        w = tensors.to_windows(res, max_length=16, stride=5, pad_id=PAD, eos_id=2, truncation_side=tside, dtype=torch.int32)
        p = tensors.to_padded(res, max_length=16, pad_id=PAD, eos_id=2, truncation_side=tside, dtype=torch.int32)
        row = w["overflow_to_sample_mapping"].cpu().numpy()
        w0 = torch.as_tensor(np.flatnonzero(np.diff(row, prepend=-1)), device=w["input_ids"].device)
        assert w0.numel() == S and torch.equal(w["input_ids"][w0], p["input_ids"]) and torch.equal(w["attention_mask"][w0], p["attention_mask"])


def test_torch_layer():
    torch = _torch()
    res, ids, offs = _source("encode")
    dev = _dev(res)
    before = torch.cuda.current_device()
    want = wc.windows(ids, offs, 64, 16, PAD, 1, 2, dtype=np.int64)
    W = want[0].shape[0]
    w = tensors.to_windows(res, max_length=64, stride=16, pad_id=PAD, bos_id=1, eos_id=2, return_lengths=True)
    total = w["input_ids"].sum()      # used at once, with no synchronisation of the caller's
    assert int(total) == int(want[0].sum())
    assert set(w) == {"input_ids", "attention_mask", "overflow_to_sample_mapping", "window_first", "lengths"}
    assert w["input_ids"].shape == (W, 64) and w["input_ids"].dtype == torch.int64 and w["attention_mask"].dtype == torch.uint8
    assert all(w[k].shape == (W,) and w[k].dtype == torch.int32 for k in ("overflow_to_sample_mapping", "window_first", "lengths"))
    assert all(t.device == dev and t.is_contiguous() for t in w.values())
    _same([w[k].cpu().numpy() for k in ("input_ids", "attention_mask", "lengths", "overflow_to_sample_mapping", "window_first")], want, "torch")
    assert set(tensors.to_windows(res, max_length=64, pad_id=PAD, dtype=torch.int32)) == {"input_ids", "attention_mask", "overflow_to_sample_mapping",
                                                                                         "window_first"}
    assert torch.cuda.current_device() == before
    # the same tensors on a stream that is not the default one
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        q = tensors.to_windows(res, max_length=64, stride=16, pad_id=PAD, bos_id=1, eos_id=2, return_lengths=True)
        s = q["input_ids"].sum()
    assert int(s) == int(want[0].sum()) and all(torch.equal(q[k], w[k]) for k in w)


# ---- Tokenizer level ---------------------------------------------------------------------------------------------

def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], ["<pad>", "<s>", "</s>"])


def _flatten(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.array([i for r in rows for i in r], np.uint32), offs


def _str_texts(ascii_only):
    texts = [t.decode("utf-8", "ignore") for t in _texts()[:40]]
    if ascii_only:
        texts = [t.encode("ascii", "ignore").decode() for t in texts]
    texts[3] = "plain </s> text <pad> with <s> specials"
    texts[5] = texts[5][:700] + "<s>" + texts[5][700:1400] + "</s><pad>" + texts[5][1400:]   # special tokens inside a long sample
    texts[7] = ""
    return texts


def test_tokenizer_overflowing_tokens():
    torch = _torch()
    tk = _tokenizer()
    base = tk.base_vocab_size()
    pad, bos, eos = base, base + 1, base + 2
    texts = _str_texts(ascii_only=True)
    rows = tk.encode_batch(texts, 0.0)
    ids, offs = _flatten(rows)
    assert (ids >= base).sum() >= 6 and max(map(len, rows)) > 64
    L, stride = 32, 8
    got = tk.encode_batch_padded(texts, pad="<pad>", bos="<s>", eos="</s>", max_length=L, stride=stride, return_overflowing_tokens=True,
                                 return_offsets_mapping="char", return_lengths=True)
    want = wc.windows(ids, offs, L, stride, pad, bos, eos, dtype=np.int64)
    W = want[0].shape[0]
    assert W > len(texts) and got["input_ids"].dtype == torch.int64 and got["offset_mapping"].shape == (W, L, 2)
    _same([got[k].cpu().numpy() for k in ("input_ids", "attention_mask", "lengths", "overflow_to_sample_mapping", "window_first")], want, "tokenizer")
    out, ln, row, om = (got[k].cpu().numpy() for k in ("input_ids", "lengths", "overflow_to_sample_mapping", "offset_mapping"))
    seen = [0] * len(texts)
    for w in range(W):
        kept, spans = out[w, 1:ln[w] - 1].tolist(), om[w, 1:ln[w] - 1]
        text = texts[row[w]]
        if kept:   # decoding a window's kept ids gives the substring its offsets name
            assert tk.decode(kept, True) == text[spans[0, 0]:spans[-1, 1]], w
            assert np.array_equal(spans[1:, 0], spans[:-1, 1]) and spans[0, 0] <= seen[row[w]]
            seen[row[w]] = spans[-1, 1]
        assert not om[w, 0].any() and not om[w, ln[w] - 1:].any()      # bos, eos and padding
    assert seen == [len(t) for t in texts]                              # every sample is covered to its end
    # bytes, over text with characters of several bytes, through the ordinary path and the flat form
    texts = _str_texts(ascii_only=False)
    assert any(len(t.encode()) > len(t) for t in texts)
    rows = tk.encode_ordinary_batch(texts, 0.0)
    ids, offs = _flatten(rows)
    flat, o = tgx.pack([t.encode("utf-8") for t in texts])
    got = tk.encode_ordinary_batch_padded_flat(flat, o, pad_id=pad, max_length=24, stride=23, return_overflowing_tokens=True,
                                               return_offsets_mapping="byte", truncation_side="left", padding_side="left", dtype=torch.int32)
    want = wc.windows(ids, offs, 24, 23, pad, pad_left=True, trunc_left=True)
    assert np.array_equal(got["input_ids"].cpu().numpy(), want[0]) and np.array_equal(got["overflow_to_sample_mapping"].cpu().numpy(), want[3])
    assert "lengths" not in got
    out, msk, row, om = (got[k].cpu().numpy() for k in ("input_ids", "attention_mask", "overflow_to_sample_mapping", "offset_mapping"))
    for w in range(0, want[0].shape[0], 37):
        raw = texts[row[w]].encode()
        for c in np.flatnonzero(msk[w]):
            assert raw[om[w, c, 0]:om[w, c, 1]] == tk.id_to_token(int(out[w, c])), (w, c)
    # without the two keywords the output is what it was
    plain = tk.encode_batch_padded(_str_texts(True), pad="<pad>", bos="<s>", eos="</s>", max_length=L, return_offsets_mapping="char")
    ids, offs = _flatten(tk.encode_batch(_str_texts(True), 0.0))
    assert set(plain) == {"input_ids", "attention_mask", "offset_mapping"} and plain["offset_mapping"].shape == (len(texts), L, 2)
    assert np.array_equal(plain["input_ids"].cpu().numpy(), lc.padded(ids, offs, L, pad, bos, eos, dtype=np.int64)[0])
    want_row = wc.windows(ids, offs, L, stride, pad, bos, eos)[3]
    k0 = np.flatnonzero(np.diff(want_row, prepend=-1))      # the first window of every sample
    first = tk.encode_batch_padded(_str_texts(True), pad="<pad>", bos="<s>", eos="</s>", max_length=L, stride=stride, return_overflowing_tokens=True,
                                   return_offsets_mapping="char")
    assert torch.equal(first["offset_mapping"][torch.as_tensor(k0, device=first["input_ids"].device)], plain["offset_mapping"])
    assert len(want_row) == first["input_ids"].shape[0]
    # an empty batch, and requests that cannot be met
    e = tk.encode_batch_padded([], pad=pad, bos=bos, max_length=16, stride=2, return_overflowing_tokens=True, return_offsets_mapping="byte")
    assert e["input_ids"].shape == (0, 16) and e["attention_mask"].shape == (0, 16) and e["offset_mapping"].shape == (0, 16, 2)
    assert e["overflow_to_sample_mapping"].shape == (0,) and e["overflow_to_sample_mapping"].dtype == torch.int32
    with pytest.raises(TypeError):
        tk.encode_batch_padded(texts, pad=pad, return_overflowing_tokens=True)              # no max_length
    with pytest.raises(ValueError):
        tk.encode_ordinary_batch_padded(texts, pad=pad, max_length=16, stride=4)            # a stride without overflow
    with pytest.raises(tgx.TokenGeeXError) as err:
        tk.encode_batch_padded(texts, pad=pad, bos=bos, max_length=16, stride=15, return_overflowing_tokens=True)
    assert err.value.status == _lib.ERR_INVALID


def _pattern_rows_against_the_twin(lens, n_out):
    """Rows of tests/past_cap.py's pattern as windows of L = 1, so that a window is a token and W·L = n_out can be any
    number; an empty row has one window of padding; against the host twin"""
    offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    ids = (np.arange(int(offs[-1]), dtype=np.uint64) * 7 % 1000).astype(np.uint32)
    want = _lib.layout_windows_host(ids, offs, 1, 0, PAD)
    assert want["input_ids"].shape == (n_out, 1)
    res = _lib.NativeResult.from_ids(ids, offs, 1000)
    try:
        got = _run(res, 1, 0, None, None, "right", "right", np.int32)
    finally:
        res.free()
    for g, name in zip(got, ("input_ids", "attention_mask", "lengths", "overflow_to_sample_mapping", "window_first")):
        assert np.array_equal(g, want[name]), name


def test_the_second_trip_of_the_strided_tile_loop():
    """W·L = 2048 tiles + one tile + 1 elements (the number is prime, so L = 1): blocks 0 and 1 of layout_window_kernel take
    a second tile.  The pattern's rows of 0 and 1 tokens are all one window wide, so the rows' windows sum to the
    pattern's total when the long row gives up its empty rows' share"""
    lens = past_cap.lengths(2048, 1024)
    lens[int(np.argmax(lens))] -= np.uint64(int((lens == 0).sum()))   # every empty row adds a window of padding
    _pattern_rows_against_the_twin(lens, past_cap.n_out(2048, 1024))


@pytest.mark.parametrize("n_out", past_cap.edge_sizes(4, 1024))
def test_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_out):
    """W·L = 0 (no row), 1, a thread's slot of 4 elements and the tile of 1024, each less one, full and one over: as many
    rows of 0 and 1 tokens, one window each"""
    _pattern_rows_against_the_twin(past_cap.edge_rows(n_out), n_out)
