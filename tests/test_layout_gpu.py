"""Padded and packed layouts on the GPU (tgx_result_pad_device / tgx_result_pack_device, csrc/layout.hip) against the
plain-numpy checker (tests/layout_checker.py).  Everything is compared exactly: this is integer data movement.

Inputs are real results — encode, sampling, n-best at k = 3 (rows beyond n_found are empty) and a resident corpus — on
a corpus with empty samples and one sample of 70 000 bytes; then a packed stream of more than 2^24 elements, the torch
layer (tokengeex_amd/tensors.py) and the Tokenizer methods."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import layout_checker as lc
import past_cap

PAD = 7
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]
POISON = -77   # what a destination holds before the call: an element the kernel skipped shows


@functools.lru_cache(maxsize=None)
def _texts():
    """~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty samples: two at the start,
    a run in the middle, one at the end."""
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
        assert res.num_samples == 3 * len(_texts())
        assert int(nf[0]) == 1    # an empty sample has one (empty) row: rows 1 and 2 lie beyond n_found
    else:
        corpus = tgx.NativeCorpus(flat, offs)
        res = nat.encode_corpus(corpus)
        res._corpus = corpus
    ids, oo = res.ids(), res.offsets()
    n = np.diff(oo.astype(np.int64))
    assert n.max() > 10_000 and (n == 0).sum() >= 6 and n[0] == 0 and n[-1] == 0
    return res, ids, oo


SOURCES = ["encode", "sample", "nbest", "resident"]


def _row_lens(offs, a):
    n = np.diff(offs.astype(np.int64))
    mx = int(n.max()) + a
    return sorted({max(1, a), max(1, a, int(np.median(n)) // 2 + a), mx, mx + 3})


def _torch():
    import torch
    return torch


def _dev(res):
    return _torch().device("cuda", res.device)


def _tdtype(dt):
    torch = _torch()
    return torch.int64 if dt == np.int64 else torch.int32


@pytest.mark.parametrize("source", SOURCES)
def test_padded_against_the_checker(source):
    torch = _torch()
    res, ids, offs = _source(source)
    S = res.num_samples
    assert res.layout_info() == (int(np.diff(offs.astype(np.int64)).max()), int(offs[-1]))
    for (bos, eos), pside, tside, dt in itertools.product(BOS_EOS, ["right", "left"], ["right", "left"], [np.int32, np.int64]):
        a = (bos is not None) + (eos is not None)
        assert res.layout_info(bos, eos)[0] == int(np.diff(offs.astype(np.int64)).max()) + a
        for L in _row_lens(offs, a):
            out = torch.full((S, L), POISON, dtype=_tdtype(dt), device=_dev(res))
            mask = torch.full((S, L), 9, dtype=torch.uint8, device=_dev(res))
            lengths = torch.full((S,), POISON, dtype=torch.int32, device=_dev(res))
            nt = tensors.pad_into(res, out, mask, lengths, row_len=L, pad_id=PAD, bos_id=bos, eos_id=eos, padding_side=pside,
                                  truncation_side=tside)
            w_out, w_mask, w_len, w_nt = lc.padded(ids, offs, L, PAD, bos, eos, pside == "left", tside == "left", dt)
            key = (source, bos, eos, pside, tside, dt, L)
            assert np.array_equal(out.cpu().numpy(), w_out), key
            assert np.array_equal(mask.cpu().numpy(), w_mask), key
            assert np.array_equal(lengths.cpu().numpy(), w_len), key
            assert nt == w_nt, key


@pytest.mark.parametrize("source", SOURCES)
def test_packed_against_the_checker(source):
    torch = _torch()
    res, ids, offs = _source(source)
    S = res.num_samples
    for (bos, eos), dt in itertools.product(BOS_EOS, [np.int32, np.int64]):
        a = (bos is not None) + (eos is not None)
        n_stream = int(offs[-1]) + S * a
        assert res.layout_info(bos, eos)[1] == n_stream
        for L in [1, 7, 512, n_stream + 5]:
            B = -(-n_stream // L)
            out = torch.full((B, L), POISON, dtype=_tdtype(dt), device=_dev(res))
            doc = torch.full((B, L), POISON, dtype=torch.int32, device=_dev(res))
            pos = torch.full((B, L), POISON, dtype=torch.int32, device=_dev(res))
            assert tensors.pack_into(res, out, doc, pos, block_len=L, pad_id=PAD, bos_id=bos, eos_id=eos) == B
            w_out, w_doc, w_pos = lc.packed_fast(ids, offs, L, PAD, bos, eos, dt)
            key = (source, bos, eos, dt, L)
            assert np.array_equal(out.cpu().numpy(), w_out), key
            assert np.array_equal(doc.cpu().numpy(), w_doc), key
            assert np.array_equal(pos.cpu().numpy(), w_pos), key
    # the per-row checker itself on one setting (packed_fast is pinned to it on small cases by test_layout_cpu.py)
    w = lc.packed(ids, offs, 512, PAD, 1, 2)
    for x, y in zip(w, lc.packed_fast(ids, offs, 512, PAD, 1, 2)):
        assert np.array_equal(x, y)


def test_optional_outputs_and_unaligned_destinations():
    """Raw pointers (NativeResult.pad_device / pack_device): mask, lengths, doc and pos left out; destinations that are not
    16-byte aligned (the element-wide store path of the kernels); a library stream (stream = 0), which is ordered after
    torch's fills on the null stream."""
    torch = _torch()
    res, ids, offs = _source("encode")
    S, L = res.num_samples, 33
    dev = _dev(res)
    for dt, shift in itertools.product([np.int32, np.int64], [0, 1]):
        flags = _lib.layout_flags(dtype=dt)
        buf = torch.full((S * L + 8,), POISON, dtype=_tdtype(dt), device=dev)
        mbuf = torch.full((S * L + 8,), 9, dtype=torch.uint8, device=dev)
        out, mask = buf[shift:shift + S * L], mbuf[shift:shift + S * L]
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        nt = res.pad_device(L, PAD, out.data_ptr(), bos_id=1, flags=flags)
        w_out, w_mask, _, w_nt = lc.padded(ids, offs, L, PAD, 1, None, dtype=dt)
        assert nt == w_nt and np.array_equal(out.cpu().numpy().reshape(S, L), w_out)
        assert (buf[:shift] == POISON).all() and (buf[shift + S * L:] == POISON).all()   # nothing beside the destination
        res.pad_device(L, PAD, out.data_ptr(), mask_ptr=mask.data_ptr(), bos_id=1, flags=flags)
        assert np.array_equal(mask.cpu().numpy().reshape(S, L), w_mask)
        assert (mbuf[:shift] == 9).all() and (mbuf[shift + S * L:] == 9).all()

        n_stream = res.layout_info(1, None)[1]
        B = -(-n_stream // L)
        pbuf = torch.full((B * L + 8,), POISON, dtype=_tdtype(dt), device=dev)
        dbuf = torch.full((B * L + 8,), POISON, dtype=torch.int32, device=dev)
        pout, dout = pbuf[shift:shift + B * L], dbuf[shift:shift + B * L]
        assert res.pack_device(L, PAD, pout.data_ptr(), bos_id=1, flags=flags) == B
        w_out, w_doc, _ = lc.packed_fast(ids, offs, L, PAD, 1, None, dt)
        assert np.array_equal(pout.cpu().numpy().reshape(B, L), w_out)
        assert (pbuf[:shift] == POISON).all() and (pbuf[shift + B * L:] == POISON).all()
        assert res.pack_device(L, PAD, pout.data_ptr(), doc_ptr=dout.data_ptr(), bos_id=1, flags=flags) == B
        assert np.array_equal(dout.cpu().numpy().reshape(B, L), w_doc)
        assert (dbuf[:shift] == POISON).all() and (dbuf[shift + B * L:] == POISON).all()


def test_ordered_after_work_queued_on_the_default_stream():
    """torch's default stream is the null stream, handle 0.  A long chain of products is queued on it, then the fill of
    the destination; the layout call that follows must start after all of that, or the fill lands on top of what it
    wrote.  The event shows that the queued work was still pending when the call was made."""
    torch = _torch()
    res, ids, offs = _source("encode")
    S, L, dev = res.num_samples, 64, _dev(res)
    assert torch.cuda.current_stream(dev).cuda_stream == 0
    a = torch.ones((4096, 4096), device=dev)
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    torch.cuda.synchronize(dev)

    def busy_then_fill(*dests):
        for _ in range(40):
            torch.mm(a, a, out=b)
        for d in dests:
            d.fill_(POISON if d.dtype != torch.uint8 else 9)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    out = torch.empty((S, L), dtype=torch.int64, device=dev)
    mask = torch.empty((S, L), dtype=torch.uint8, device=dev)
    lengths = torch.empty((S,), dtype=torch.int32, device=dev)
    w_out, w_mask, w_len, w_nt = lc.padded(ids, offs, L, PAD, 1, 2, dtype=np.int64)
    ev = busy_then_fill(out, mask, lengths)
    pending = not ev.query()
    nt = tensors.pad_into(res, out, mask, lengths, row_len=L, pad_id=PAD, bos_id=1, eos_id=2)
    assert pending, "the queued work had ended before the call: nothing was tested"
    assert nt == w_nt and np.array_equal(out.cpu().numpy(), w_out)
    assert np.array_equal(mask.cpu().numpy(), w_mask) and np.array_equal(lengths.cpu().numpy(), w_len)

    ev = busy_then_fill(out)      # the raw entry point with no stream of the caller's
    pending = not ev.query()
    assert res.pad_device(L, PAD, out.data_ptr(), bos_id=1, eos_id=2, flags=_lib.LAYOUT_I64) == w_nt
    assert pending and np.array_equal(out.cpu().numpy(), w_out)

    n_stream = res.layout_info(1, 2)[1]
    B = -(-n_stream // L)
    pout = torch.empty((B, L), dtype=torch.int32, device=dev)
    doc = torch.empty((B, L), dtype=torch.int32, device=dev)
    pos = torch.empty((B, L), dtype=torch.int32, device=dev)
    w = lc.packed_fast(ids, offs, L, PAD, 1, 2, np.int32)
    ev = busy_then_fill(pout, doc, pos)
    pending = not ev.query()
    assert tensors.pack_into(res, pout, doc, pos, block_len=L, pad_id=PAD, bos_id=1, eos_id=2) == B
    assert pending
    assert all(np.array_equal(t.cpu().numpy(), x) for t, x in zip((pout, doc, pos), w))

    # to_padded: the block torch.empty hands out was just given back while work that writes it is still queued
    scratch = torch.empty((S, L), dtype=torch.int64, device=dev)
    ev = busy_then_fill(scratch)
    pending = not ev.query()
    del scratch
    got = tensors.to_padded(res, max_length=L, pad_id=PAD, bos_id=1, eos_id=2)
    assert pending and np.array_equal(got["input_ids"].cpu().numpy(), w_out)


def test_host_twins_of_a_result():
    res, ids, offs = _source("encode")
    got = res.pad_host(40, PAD, bos_id=1, eos_id=2, padding_side="left", dtype=np.int64)
    w = lc.padded(ids, offs, 40, PAD, 1, 2, True, False, np.int64)
    assert np.array_equal(got["input_ids"], w[0]) and np.array_equal(got["attention_mask"], w[1]) and got["n_truncated"] == w[3]
    got = res.pack_host(512, PAD, eos_id=2)
    w = lc.packed_fast(ids, offs, 512, PAD, None, 2)
    assert all(np.array_equal(got[k], x) for k, x in zip(("input_ids", "doc_ids", "positions"), w))


def test_packed_stream_of_more_than_2_pow_24_elements():
    torch = _torch()
    flat, offs = synth.make_corpus(64 << 20, "mixed", seed_offset=9)
    res = _native().encode_batch_flat(flat, offs)
    ids, oo = res.ids(), res.offsets()
    n_stream = res.layout_info(None, 2)[1]
    assert n_stream == ids.size + res.num_samples and n_stream > 1 << 24
    for L, dt in [(4096, torch.int64), (1000, torch.int32)]:
        got = tensors.to_packed(res, L, pad_id=PAD, eos_id=2, dtype=dt, return_doc=True)
        w_out, w_doc, w_pos = lc.packed_fast(ids, oo, L, PAD, None, 2, np.int64 if dt == torch.int64 else np.int32)
        assert np.array_equal(got["input_ids"].cpu().numpy(), w_out)
        assert np.array_equal(got["doc_ids"].cpu().numpy(), w_doc)
        assert np.array_equal(got["positions"].cpu().numpy(), w_pos)
    # and the padded layout of the same result, truncating most rows
    got = tensors.to_padded(res, max_length=128, pad_id=PAD, bos_id=1, dtype=torch.int32, return_lengths=True)
    n = np.diff(oo.astype(np.int64))
    assert np.array_equal(got["lengths"].cpu().numpy(), np.minimum(n, 127) + 1)
    first = np.minimum(n, 127)
    rows = [0, 1, res.num_samples // 2, res.num_samples - 1]
    w = lc.padded(ids, oo, 128, PAD, 1, None)[0][rows]
    assert np.array_equal(got["input_ids"][rows].cpu().numpy(), w)
    assert int(got["attention_mask"].sum()) == int((first + 1).sum())
    res.free()


@pytest.mark.parametrize("n_out", past_cap.edge_sizes(4, 1024))
def test_packed_outputs_that_end_at_the_edges_of_a_slot_and_a_tile(n_out):
    """B·L = 0, 1, a thread's slot of 4 elements and the tile of 1024, each less one, full and one over: rows of
    tests/past_cap.py's pattern packed into blocks of one element, so that B·L is the stream's length; against the host twin"""
    torch = _torch()
    offs = past_cap.edge_offsets(n_out)
    ids = (np.arange(n_out, dtype=np.uint64) * 7 % 1000).astype(np.uint32)
    want = _lib.layout_pack_host(ids, offs, 1, PAD)
    assert want["input_ids"].shape == (n_out, 1)
    res = _lib.NativeResult.from_ids(ids, offs, 1000)
    try:
        got = tensors.to_packed(res, 1, pad_id=PAD, dtype=torch.int32, return_doc=True)
        for name in ("input_ids", "doc_ids", "positions"):
            assert np.array_equal(got[name].cpu().numpy(), want[name]), name
    finally:
        res.free()


def test_torch_layer():
    torch = _torch()
    res, ids, offs = _source("encode")
    S = res.num_samples
    dev = _dev(res)
    before = torch.cuda.current_device()
    mx = int(np.diff(offs.astype(np.int64)).max())

    p = tensors.to_padded(res, pad_id=PAD, bos_id=1, eos_id=2, return_lengths=True)
    # used at once, with no synchronisation of the caller's
    total, n_pad = p["input_ids"].sum(), p["input_ids"].eq(PAD).sum()
    w_out, w_mask, w_len, _ = lc.padded(ids, offs, mx + 2, PAD, 1, 2, dtype=np.int64)
    assert int(total) == int(w_out.sum()) and int(n_pad) == int((w_out == PAD).sum())
    assert p["input_ids"].shape == (S, mx + 2) and p["input_ids"].dtype == torch.int64
    assert p["attention_mask"].shape == (S, mx + 2) and p["attention_mask"].dtype == torch.uint8
    assert p["lengths"].shape == (S,) and p["lengths"].dtype == torch.int32
    assert all(t.device == dev and t.is_contiguous() for t in p.values())
    assert np.array_equal(p["input_ids"].cpu().numpy(), w_out) and np.array_equal(p["attention_mask"].cpu().numpy(), w_mask)
    assert np.array_equal(p["lengths"].cpu().numpy(), w_len)
    assert set(tensors.to_padded(res, max_length=16, pad_id=PAD, dtype=torch.int32)) == {"input_ids", "attention_mask"}
    p32 = tensors.to_padded(res, max_length=16, pad_id=PAD, dtype=torch.int32, padding_side="left", truncation_side="left")
    assert p32["input_ids"].dtype == torch.int32 and p32["input_ids"].shape == (S, 16)
    assert np.array_equal(p32["input_ids"].cpu().numpy(), lc.padded(ids, offs, 16, PAD, pad_left=True, trunc_left=True)[0])

    k = tensors.to_packed(res, 512, pad_id=PAD, eos_id=2, return_doc=True)
    total, n_tail = k["input_ids"].sum(), k["doc_ids"].eq(-1).sum()
    w_out, w_doc, w_pos = lc.packed_fast(ids, offs, 512, PAD, None, 2, np.int64)
    assert int(total) == int(w_out.sum()) and int(n_tail) == int((w_doc == -1).sum()) > 0
    assert k["input_ids"].dtype == torch.int64 and k["doc_ids"].dtype == k["positions"].dtype == torch.int32
    assert all(t.shape == w_out.shape and t.device == dev and t.is_contiguous() for t in k.values())
    assert np.array_equal(k["positions"].cpu().numpy(), w_pos)
    kd = tensors.to_packed(res, 512, pad_id=PAD, eos_id=2, return_doc=True, drop_last=True, dtype=torch.int32)
    assert all(t.shape == (w_out.shape[0] - 1, 512) and t.is_contiguous() for t in kd.values())
    assert np.array_equal(kd["input_ids"].cpu().numpy(), w_out[:-1]) and int(kd["doc_ids"].min()) >= 0
    assert set(tensors.to_packed(res, 512, pad_id=PAD)) == {"input_ids"}
    assert torch.cuda.current_device() == before

    # the ids are usable on another stream's work too: the call has returned, so the stream has reached its end
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        q = tensors.to_padded(res, max_length=64, pad_id=PAD, eos_id=2)
        s = q["input_ids"].sum()
    assert int(s) == int(lc.padded(ids, offs, 64, PAD, None, 2, dtype=np.int64)[0].sum())


def test_destinations_are_checked_before_any_launch():
    torch = _torch()
    res, ids, offs = _source("encode")
    S, dev = res.num_samples, _dev(res)
    good = torch.full((S, 8), POISON, dtype=torch.int32, device=dev)
    for bad, exc in [(torch.empty((S, 8), dtype=torch.int32), ValueError),                    # on the host
                     (torch.empty((S, 7), dtype=torch.int32, device=dev), ValueError),        # too small
                     (torch.empty((S, 8), dtype=torch.int16, device=dev), ValueError),        # no id type
                     (torch.empty((8, S), dtype=torch.int32, device=dev).t(), ValueError),    # not contiguous
                     (np.empty((S, 8), np.int32), TypeError)]:
        with pytest.raises(exc):
            tensors.pad_into(res, bad, row_len=8, pad_id=PAD)
        with pytest.raises(exc):
            tensors.pack_into(res, bad, block_len=8, pad_id=PAD)   # (each of them is too small for the stream as well)
    with pytest.raises(ValueError):   # a mask that is too small, beside a good destination: nothing is written
        tensors.pad_into(res, good, torch.empty((S, 4), dtype=torch.uint8, device=dev), row_len=8, pad_id=PAD)
    with pytest.raises(ValueError):
        tensors.pad_into(res, good, lengths=torch.empty((S,), dtype=torch.int64, device=dev), row_len=8, pad_id=PAD)
    with pytest.raises(ValueError):
        tensors.pack_into(res, torch.empty((4, 8), dtype=torch.int32, device=dev), block_len=8, pad_id=PAD)
    assert (good == POISON).all()
    # the C ABI itself: host memory as a destination, NULL where something would be written, bad lengths and ids
    host = np.empty(S * 8, np.int32)
    for call in (lambda: res.pad_device(8, PAD, host.ctypes.data), lambda: res.pack_device(8, PAD, host.ctypes.data),
                 lambda: res.pad_device(8, PAD, good.data_ptr(), mask_ptr=host.ctypes.data),
                 lambda: res.pad_device(8, PAD, 0), lambda: res.pack_device(8, PAD, 0),
                 lambda: res.pad_device(0, PAD, good.data_ptr()), lambda: res.pad_device(1, PAD, good.data_ptr(), bos_id=1, eos_id=2),
                 lambda: res.pack_device(0, PAD, good.data_ptr()), lambda: res.pad_device(8, 2**31, good.data_ptr()),
                 lambda: res.pad_device(8, PAD, good.data_ptr(), bos_id=2**31), lambda: res.pack_device(8, PAD, good.data_ptr(), eos_id=2**31),
                 lambda: res.pad_device(8, PAD, good.data_ptr(), flags=64), lambda: res.pack_device(8, PAD, good.data_ptr(), flags=1)):
        with pytest.raises(tgx.TokenGeeXError) as e:
            call()
        assert e.value.status == _lib.ERR_INVALID, e.value
    assert (good == POISON).all()
    # and the library still works
    assert res.pad_device(8, PAD, good.data_ptr()) == lc.padded(ids, offs, 8, PAD)[3]
    assert np.array_equal(good.cpu().numpy(), lc.padded(ids, offs, 8, PAD)[0])


def test_result_on_a_second_device():
    torch = _torch()
    if tgx.device_count() < 2 or torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    toks, scores, _ = synth.load_spec_vocab(32000)
    nat1 = tgx.NativeModel(list(toks), np.asarray(scores, np.float64), device=1)
    flat, offs = tgx.pack(_texts())
    torch.cuda.set_device(0)
    res = nat1.encode_batch_flat(flat, offs)
    assert res.device == 1
    ids, oo = res.ids(), res.offsets()
    p = tensors.to_padded(res, max_length=100, pad_id=PAD, bos_id=1)
    k = tensors.to_packed(res, 512, pad_id=PAD, eos_id=2, return_doc=True)
    assert torch.cuda.current_device() == 0
    assert all(t.device == torch.device("cuda", 1) for t in list(p.values()) + list(k.values()))
    assert np.array_equal(p["input_ids"].cpu().numpy(), lc.padded(ids, oo, 100, PAD, 1, None, dtype=np.int64)[0])
    assert np.array_equal(k["doc_ids"].cpu().numpy(), lc.packed_fast(ids, oo, 512, PAD, None, 2)[1])
    with pytest.raises(ValueError):   # a destination on device 0 for a result on device 1
        tensors.pad_into(res, torch.empty((res.num_samples, 8), dtype=torch.int32, device="cuda:0"), row_len=8, pad_id=PAD)
    with pytest.raises(tgx.TokenGeeXError) as e:
        res.pad_device(8, PAD, torch.empty((res.num_samples, 8), dtype=torch.int32, device="cuda:0").data_ptr())
    assert e.value.status == _lib.ERR_INVALID
    assert torch.cuda.current_device() == 0


# ---- Tokenizer level ---------------------------------------------------------------------------------------------

def _tokenizer(processors=()):
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], list(processors), ["<pad>", "<s>", "</s>"])


def _flatten(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.array([i for r in rows for i in r], np.uint32), offs


def _str_texts():
    texts = [t.decode("utf-8", "ignore") for t in _texts()[:60]]
    texts[3] = "plain </s> text <pad> with <s> specials"   # a special token's string is ordinary text on this path
    texts[5] = "line one\r\nline two\r\ne\u0301 \u212b"   # CRLF, and two characters NFC changes
    return texts


@pytest.mark.parametrize("procs", [(), ("crlf", "nfc")])
def test_tokenizer_padded_and_packed(procs):
    torch = _torch()
    tk = _tokenizer([tgx.CrlfProcessor() if p == "crlf" else tgx.UnicodeProcessor(p) for p in procs])
    texts = _str_texts()
    rows = tk.encode_ordinary_batch(texts, 0.0)
    ids, offs = _flatten(rows)
    base = tk.base_vocab_size()
    assert max(map(max, filter(None, rows))) < base   # no special id: "</s>" inside a text was encoded as text
    if procs:
        assert rows[5] == _tokenizer().encode_ordinary("line one\nline two\n\u00e9 \u00c5", 0.0) != \
            _tokenizer().encode_ordinary(texts[5], 0.0)
    pad, bos, eos = base, base + 1, base + 2
    got = tk.encode_ordinary_batch_padded(texts, pad="<pad>", bos="<s>", eos="</s>", max_length=256, return_lengths=True)
    w = lc.padded(ids, offs, 256, pad, bos, eos, dtype=np.int64)
    assert got["input_ids"].device == torch.device("cuda", 0) and got["input_ids"].dtype == torch.int64
    assert np.array_equal(got["input_ids"].cpu().numpy(), w[0])
    assert np.array_equal(got["attention_mask"].cpu().numpy(), w[1]) and np.array_equal(got["lengths"].cpu().numpy(), w[2])
    got = tk.encode_ordinary_batch_padded(texts, 0.0, pad_id=pad, eos="</s>", padding_side="left", dtype=torch.int32)
    mx = int(np.diff(offs.astype(np.int64)).max()) + 1
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.padded(ids, offs, mx, pad, None, eos, pad_left=True)[0])
    got = tk.encode_ordinary_batch_packed(texts, 512, pad="<pad>", eos="</s>", return_doc=True)
    w = lc.packed(ids, offs, 512, pad, None, eos, np.int64)
    assert all(np.array_equal(got[k].cpu().numpy(), x) for k, x in zip(("input_ids", "doc_ids", "positions"), w))
    # the flat forms
    flat, o = tgx.pack([t.encode("utf-8") for t in texts])
    got = tk.encode_ordinary_batch_padded_flat(flat, o, pad=pad, max_length=64)
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.padded(ids, offs, 64, pad, dtype=np.int64)[0])
    got = tk.encode_ordinary_batch_packed_flat(flat, o, 100, pad=pad, bos="<s>", drop_last=True)
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.packed(ids, offs, 100, pad, bos, None, np.int64)[0][:-1])
    # an empty batch
    e = tk.encode_ordinary_batch_padded([], pad=pad, bos=bos)
    assert e["input_ids"].shape == (0, 1) and e["attention_mask"].shape == (0, 1)
    assert tk.encode_ordinary_batch_packed([], 16, pad=pad, return_doc=True)["doc_ids"].shape == (0, 16)
    with pytest.raises(tgx.TokenGeeXError):
        tk.encode_ordinary_batch_padded(texts, pad="<nope>")
    with pytest.raises(TypeError):
        tk.encode_ordinary_batch_padded(texts, bos="<s>")


def test_tokenizer_dropout_matches_the_list_surface():
    tk = _tokenizer()
    tk.seed = 1234
    texts = _str_texts()
    rows = tk.encode_ordinary_batch(texts, 0.3)
    assert rows != tk.encode_ordinary_batch(texts, 0.0)
    ids, offs = _flatten(rows)
    pad = tk.base_vocab_size()
    got = tk.encode_ordinary_batch_padded(texts, 0.3, pad=pad, max_length=300)
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.padded(ids, offs, 300, pad, dtype=np.int64)[0])
    got = tk.encode_ordinary_batch_packed(texts, 256, 0.3, pad=pad, eos="</s>")
    assert np.array_equal(got["input_ids"].cpu().numpy(), lc.packed(ids, offs, 256, pad, None, pad + 2, np.int64)[0])
