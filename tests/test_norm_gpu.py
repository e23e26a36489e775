"""Unicode normalisation on the device (tgx_corpus_normalize, csrc/norm.hip): a resident corpus against normalize_flat
(csrc/unicode_norm.cpp) and the host twin, and the Tokenizer's encode_corpus_* with device_unicode against its flat
routes.  Everything is compared exactly: this is byte and integer movement.  The inputs are those of tests/norm_cases.py
(under 1 MB each, and one of 17 MB that takes the grids past their caps)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import norm_cases as nc


def _check(form, rows, key):
    """-> the number of pieces"""
    return _check_flat(form, *tgx.pack(list(rows)), key)


def _check_flat(form, flat, offs, key):
    """_check of a packed batch"""
    want_f, want_o = _lib.normalize_flat(form, flat, offs)
    twin_f, twin_o, twin_k = _lib.normalize_host_twin(form, flat, offs)
    corpus = tgx.NativeCorpus(flat, offs)
    out = corpus.normalize(form)
    try:
        assert out.device == corpus.device and out.num_samples == offs.size - 1 and out.num_bytes == want_f.size, (form, key)
        got_f, got_o = out.bytes(), out.offsets()
        assert np.array_equal(got_o, want_o) and np.array_equal(got_f, want_f), (form, key)
        assert np.array_equal(got_o, twin_o) and np.array_equal(got_f, twin_f) and out.n_pieces == twin_k, (form, key)
        # the corpus was only read
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), (form, key)
        return out.n_pieces
    finally:
        out.free()
        corpus.free()


@pytest.mark.parametrize("form", nc.FORMS)
def test_edges_of_slots_tiles_and_rows(form):
    assert _check(form, nc.edge_batch(), "edges") > 20
    assert _check(form, [b"".join(nc.edge_batch())], "edges, one row") > 20
    _check(form, nc.INVALID, "invalid")


@pytest.mark.parametrize("form", nc.FORMS)
def test_random_sequences_with_combining_marks(form):
    assert _check(form, nc.random_rows(), "random") > 10000


@pytest.mark.parametrize("form", nc.FORMS)
def test_past_the_caps(form):
    """nc.past_cap_corpus(): over 4096·4096 + 2·4096 bytes, so norm_mark, norm_pieces (past tiles of ASCII that it skips) and
    norm_places go round twice; over 256·4096 rows and over 64·4096 pieces, so the kernels with a thread per row or per
    piece do too (tests/test_norm_cpu.py holds the corpus to this)"""
    flat, offs = nc.past_cap_corpus()
    assert _check_flat(form, flat, offs, "past the caps") > 262_144    # kPieceBlock · kNormMaxBlocks


@pytest.mark.parametrize("form", nc.FORMS)
def test_mixed_text(form):
    rows = nc.mixed_rows()
    k = _check(form, rows, "mixed")
    assert (k == 0) == (form in ("nfc", "nfd"))   # its fullwidth punctuation changes under the compatibility forms only


def test_a_corpus_without_pieces_is_copied():
    rows = list(nc.mixed_rows()) + [b"", "plain \u4e2d\u6587 and \u00e9 (composed)".encode()]
    flat, offs = tgx.pack(rows)
    corpus = tgx.NativeCorpus(flat, offs)
    out = corpus.normalize("nfc")
    assert out.n_pieces == 0 and np.array_equal(out.bytes(), flat) and np.array_equal(out.offsets(), offs)
    out.free()


def test_no_rows_and_no_bytes():
    for rows in ([], [b"", b"", b""]):
        corpus = tgx.NativeCorpus(*tgx.pack(rows))
        for form in nc.FORMS:
            out = corpus.normalize(form)
            assert out.num_samples == len(rows) and out.num_bytes == 0 and out.n_pieces == 0 and out.offsets().tolist() == [0] * (len(rows) + 1)
            out.free()


def test_window():
    marks31, marks32 = nc.descending_marks(31), nc.descending_marks(32)
    jamo = ("\uac00" + "\u1161" * 3000).encode()
    good = [b"ok", ("e" + marks31).encode(), b"", ("x" + marks31 + "y" + marks31).encode(), jamo]
    bad = [b"ok", b"", b"a" * 5000, ("e" + marks32).encode(), ("e" + marks31).encode(), ("o" + marks32 + "!").encode()]
    for form in nc.FORMS:
        assert _check(form, good, "31 marks") == 4
        with pytest.raises(tgx.TokenGeeXError) as want:
            _lib.normalize_host_twin(form, *tgx.pack(bad))
        corpus = tgx.NativeCorpus(*tgx.pack(bad))
        with pytest.raises(tgx.TokenGeeXError) as e:
            corpus.normalize(form)
        assert e.value.status == want.value.status == _lib.ERR_UNSUPPORTED and e.value.sample == want.value.sample == 3, (form, e.value)
        assert "32" in str(e.value) and str(e.value).split(":", 1)[1] == str(want.value).split(":", 1)[1]
        # a correct call straight after it
        assert _check(form, good[:2], "after the refusal") == 1
        corpus.free()


def test_arguments():
    corpus = tgx.NativeCorpus(*tgx.pack([b"abc"]))
    import ctypes as C
    h, k = C.c_void_p(), C.c_uint64()
    assert _lib.lib.tgx_corpus_normalize(corpus._h, 4, C.byref(h), C.byref(k)) == _lib.ERR_INVALID and not h.value
    assert _lib.lib.tgx_corpus_normalize(corpus._h, 1, None, C.byref(k)) == _lib.ERR_INVALID
    assert _lib.lib.tgx_corpus_normalize(None, 1, C.byref(h), C.byref(k)) == _lib.ERR_INVALID
    out = corpus.normalize("nfkc")
    assert out.bytes().tobytes() == b"abc"
    assert list(_lib.norm_last_times()) == ["norm_mark", "norm_pieces", "norm_length", "norm_places", "norm_write"]
    out.free()


# ---- Tokenizer level ---------------------------------------------------------------------------------------------

SPECIALS = ["<|endoftext|>", "<|fim", "<|fim|>", "<pad>", "<s>", "</s>"]   # test_front_gpu.py's
LISTS = [("nfc",), ("crlf", "nfc"), ("crlf", "nfkc"), ("nfd",)]


def _tokenizer(procs, specials):
    toks, scores, _ = synth.load_spec_vocab(32000)
    processors = [tgx.CrlfProcessor() if p == "crlf" else tgx.UnicodeProcessor(p) for p in procs]
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors, list(specials))
    tk.device_unicode = True
    return tk


def _batch():
    """decomposed Latin, jamo, fullwidth forms, "\\r\\n", a special token directly in front of a mark, empty samples"""
    body = [r.decode("utf-8", "ignore") for r in nc.mixed_rows()[:24]]
    texts = ["", "cafe\u0301 A\u030a<|endoftext|>\u00e9", "e<s>\u0301", "\u1100\u1161\u11a8 \uac00<s>\u1161", "\uff21\uff22\uff23\r\n\uff01<pad>\ufb01",
             "a\r\n<s>\r\nb\r\n", "\r\n</s>", "e\r\n\u0301", "", "no special token in here", "\u0301<|fim|>\u0327\u0301<|fim", "o\u0302\u0323\r", "\n<s>\r"]
    for k, t in enumerate(body):
        cut = len(t) // 3
        texts.append(t[:cut] + "e\u0301<|fim|>" + t[cut:2 * cut] + "<s>" * (k % 3) + "\r\n\uff21" + t[2 * cut:] + ("u\u0308<|endoftext|>" if k % 2 else ""))
    texts += ["<pad>", ""]
    return tgx.pack([t.encode("utf-8") for t in texts])


def _same(res, want, key):
    try:
        assert res.num_samples == want.num_samples and res.num_tokens == want.num_tokens and res.vocab_size == want.vocab_size, key
        assert np.array_equal(res.offsets(), want.offsets()) and np.array_equal(res.ids(), want.ids()), key
    finally:
        res.free()
        want.free()


@pytest.mark.parametrize("with_specials", [True, False])
@pytest.mark.parametrize("procs", LISTS)
def test_encode_corpus_result(procs, with_specials):
    tk = _tokenizer(procs, SPECIALS if with_specials else [])
    tk.seed = 4321
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)
    # Without special tokens a CRLF pass goes through the split, which drops the empty samples, so a row is hashed by its
    # index among the non-empty samples and the flat route hashes it by its index among all: dropout is not compared there
    # (test_front_gpu.py leaves it out for the same reason).  [Unicode] alone keeps every row and is compared.
    dropouts = (0.0, 0.3) if with_specials or "crlf" not in procs else (0.0,)
    for dropout in dropouts:
        want_ids, want_offs = tk.encode_batch_flat(flat, offs, dropout)
        res = tk.encode_corpus_result(corpus, dropout)
        assert res.vocab_size == tk.vocab_size() and res.num_samples == offs.size - 1
        assert np.array_equal(res.offsets(), want_offs) and np.array_equal(res.ids(), want_ids), (procs, with_specials, dropout)
        res.free()
    assert not np.array_equal(tk.encode_batch_flat(flat, offs, 0.3)[0], tk.encode_batch_flat(flat, offs, 0.0)[0])
    # the form matters on these texts
    plain = _tokenizer(tuple(p for p in procs if p == "crlf"), SPECIALS if with_specials else [])
    assert not np.array_equal(plain.encode_batch_flat(flat, offs, 0.0)[0], tk.encode_batch_flat(flat, offs, 0.0)[0])


@pytest.mark.parametrize("with_specials", [True, False])
@pytest.mark.parametrize("procs", LISTS)
def test_encode_corpus_sample_result(procs, with_specials):
    tk = _tokenizer(procs, SPECIALS if with_specials else [])
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)
    want, want_logz = tk.encode_batch_sample_result_flat(flat, offs, 0.7, seed=99, return_logz=True)
    res, logz = tk.encode_corpus_sample_result(corpus, 0.7, seed=99, return_logz=True)
    assert logz.dtype == np.float64 and np.array_equal(logz, want_logz)
    assert not np.array_equal(want.ids(), tk.encode_batch_flat(flat, offs, 0.0)[0])
    if not with_specials and "crlf" in procs:
        # the flat route hashes a sample by its index among all samples, the split by that among the non-empty ones (the
        # case test_front_gpu.py leaves out): log Z does not depend on the draws and is compared above, the ids are not
        assert res.num_samples == want.num_samples
        res.free()
        want.free()
        return
    _same(res, want, ("sample", procs, with_specials))


def test_encode_corpus_layouts():
    import torch
    tk = _tokenizer(("crlf", "nfc"), SPECIALS)
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)

    def same(a, b, key):
        assert set(a) == set(b), key
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (key, k)

    kw = dict(pad="<pad>", max_length=160, return_offsets_mapping="char")
    same(tk.encode_corpus_padded(corpus, **kw), tk.encode_batch_padded_flat(flat, offs, **kw), kw)
    kw = dict(pad="<pad>", eos="<|endoftext|>", return_doc=True)
    same(tk.encode_corpus_packed(corpus, 512, **kw), tk.encode_batch_packed_flat(flat, offs, 512, **kw), kw)


def test_processor_lists_that_are_still_refused():
    corpus = tgx.NativeCorpus(*tgx.pack([b"a\r\n<s>b"]))
    for procs in (("nfc", "crlf"), ("nfc", "nfc"), ("crlf", "crlf")):
        tk = _tokenizer(procs, SPECIALS)
        for call in (lambda: tk.encode_corpus_result(corpus), lambda: tk.encode_corpus_sample_result(corpus, 0.5, seed=1),
                     lambda: tk.encode_corpus_padded(corpus, pad="<pad>"), lambda: tk.encode_corpus_packed(corpus, 8, pad="<pad>")):
            with pytest.raises(tgx.TokenGeeXError) as e:
                call()
            assert e.value.status == _lib.ERR_UNSUPPORTED and "encode_batch_result_flat" in str(e.value), procs
    # and the opt-in is one: without it the lists with a Unicode form are refused as before
    tk = _tokenizer(("nfc",), SPECIALS)
    tk.device_unicode = False
    with pytest.raises(tgx.TokenGeeXError) as e:
        tk.encode_corpus_result(corpus)
    assert e.value.status == _lib.ERR_UNSUPPORTED
