"""The device front end (tgx_corpus_split_specials, csrc/front.hip): a resident corpus split at special tokens and packed
with the CRLF pass, against split_specials_flat + pack_segments on the host; the plan assembled where it is
(tgx_assemble_result_plan) against tgx_assemble_result from the host arrays; and the Tokenizer's encode_corpus_* against
its flat routes.  Everything is compared exactly: this is byte and integer movement.  The cases are those of
tests/front_cases.py, each with the CRLF pass on and off, and its corpus of 16.8 MB that takes the grids past their caps."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import front_cases as fc


@functools.lru_cache(maxsize=None)
def _native():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.NativeModel(list(toks), np.asarray(scores, np.float64))


def _same(res, want, key):
    """a device result against a host-route result; both are freed"""
    try:
        assert res.num_samples == want.num_samples and res.num_tokens == want.num_tokens and res.vocab_size == want.vocab_size, key
        assert np.array_equal(res.offsets(), want.offsets()) and np.array_equal(res.ids(), want.ids()), key
    finally:
        res.free()
        want.free()


def _check(samples, specials, crlf, key):
    _check_flat(*tgx.pack(samples), specials, crlf, key)


def _check_flat(flat, offs, specials, crlf, key, encode=True):
    """a packed batch through the device front end against the host route; encode=False: without the encode of the
    segments and the assembly of the plan"""
    nat = _native()
    seg_offs, ss, pflat, poffs = fc.truth_flat(flat, offs, specials, crlf)
    corpus = tgx.NativeCorpus(flat, offs)
    segs, plan = corpus.split_specials(specials, crlf)
    try:
        # the plan is the host's
        assert (plan.num_samples, plan.num_segments, plan.num_encoded) == (offs.size - 1, ss.size, poffs.size - 1), key
        assert plan.device == corpus.device == segs.device, key
        assert np.array_equal(plan.seg_offs(), seg_offs) and np.array_equal(plan.seg_special(), ss), key
        # the segments' corpus holds what the host packs, byte for byte, and encodes to the same ids
        assert segs.num_samples == poffs.size - 1 and segs.num_bytes == pflat.size, key
        assert np.array_equal(segs.offsets(), poffs) and np.array_equal(segs.bytes(), pflat), key
        got = want = None
        if encode and plan.num_encoded:
            got, want = nat.encode_corpus(segs), nat.encode_batch_flat(pflat, poffs)
            assert np.array_equal(got.offsets(), want.offsets()) and np.array_equal(got.ids(), want.ids()), key
        # the plan assembled from HBM against the host arrays uploaded
        if encode:
            _same(nat.assemble_plan(got, plan, len(specials)), nat.assemble(want, seg_offs, ss, len(specials)), key)
        for r in (got, want):
            if r is not None:
                r.free()
        # the corpus was only read
        assert np.array_equal(corpus.bytes(), flat) and np.array_equal(corpus.offsets(), offs), key
    finally:
        segs.free()
        plan.free()
        corpus.free()


CASES = {name: (samples, specials) for name, samples, specials in fc.fixed_cases()}
GROUPS = ["straddle", "prefix_across_samples", "complete", "list_order", "first_byte", "multibyte", "invalid", "overlap", "empty", "only_empty",
          "sample_is", "only_specials", "no_special", "special_every", "mixed", "crlf"]


def test_every_case_is_in_a_group():
    assert all(sum(name.startswith(g) for g in GROUPS) == 1 for name in CASES), [n for n in CASES if sum(n.startswith(g) for g in GROUPS) != 1]
    assert sum(len(b"".join(s)) for s, _ in CASES.values()) < 600 << 10 and max(len(b"".join(s)) for s, _ in CASES.values()) < 300 << 10


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_fixed_cases(group, crlf):
    names = [n for n in CASES if n.startswith(group)]
    assert names
    for name in names:
        _check(*CASES[name], crlf, name)


def test_random_batches():
    rng = np.random.default_rng(77)
    for it in range(12):
        samples, specials = fc.random_batch(rng)
        _check(samples, specials, bool(it & 1), ("random", it))


@pytest.mark.parametrize("crlf", [False, True])
def test_past_the_caps(crlf):
    """fc.past_cap_corpus(): over 4096·4096 + 2·4096 bytes, so the kernels over tiles go round twice (two of them past tiles
    they skip), and over 256·4096 samples, candidates, segments and segments to encode, so the kernels with a thread per one
    of these do too (tests/test_front_cpu.py holds the corpus to this).  The plan, the segments' corpus and the source are
    compared whole; the encode and the assembly are run on the first and the last 2 000 rows, taken with select."""
    flat, offs, specials = fc.past_cap_corpus()
    _check_flat(flat, offs, specials, crlf, "past the caps", encode=False)
    S = offs.size - 1
    corpus = tgx.NativeCorpus(flat, offs)
    ends = corpus.select(np.concatenate([np.arange(2000), np.arange(S - 2000, S)]))
    try:
        _check_flat(ends.bytes(), ends.offsets(), specials, crlf, "past the caps, both ends")
    finally:
        ends.free()
        corpus.free()


def test_no_samples_and_no_bytes():
    for samples in ([], [b"", b"", b""]):
        corpus = tgx.NativeCorpus(*tgx.pack(samples))
        segs, plan = corpus.split_specials([b"<s>"], True)
        assert (plan.num_samples, plan.num_segments, plan.num_encoded) == (len(samples), 0, 0)
        assert plan.seg_offs().tolist() == [0] * (len(samples) + 1) and plan.seg_special().size == 0
        assert segs.num_samples == 0 and segs.num_bytes == 0 and segs.offsets().tolist() == [0]
        res = _native().assemble_plan(None, plan, 1)
        assert res.num_samples == len(samples) and res.num_tokens == 0 and res.offsets().tolist() == [0] * (len(samples) + 1)
        res.free()


def test_refusals():
    nat = _native()
    corpus = tgx.NativeCorpus(*tgx.pack([b"ab<s>cd", b"<s>", b"ef"]))

    def refused(call, status=_lib.ERR_INVALID):
        with pytest.raises(tgx.TokenGeeXError) as e:
            call()
        assert e.value.status == status, e.value
        return str(e.value)

    # an empty special: the host function's message; too many specials: unsupported, as documented
    with pytest.raises(tgx.TokenGeeXError) as want:
        _lib.split_specials_flat(*tgx.pack([b"ab"]), [b"<s>", b""])
    assert refused(lambda: corpus.split_specials([b"<s>", b""], False)) == str(want.value)
    assert "special tokens" in refused(lambda: corpus.split_specials([b"<%05d>" % k for k in range(4097)], False), _lib.ERR_UNSUPPORTED)
    assert "special tokens" in refused(lambda: corpus.split_specials([b"<%d>" % k + b"y" * 700 for k in range(100)], True), _lib.ERR_UNSUPPORTED)
    # 1024 specials of 32 bytes are taken
    many = [b"<%04d|" % k + b"x" * 26 for k in range(1024)]
    _check([b"ab" + many[1023] + b"cd" + many[0] + many[512][:-1], many[7]], many, False, "1024 specials")

    segs, plan = corpus.split_specials([b"<s>", b"</s>"], False)
    assert plan.num_encoded == 3 and plan.num_segments == 5
    res = nat.encode_corpus(segs)
    assert "plan was made with" in refused(lambda: nat.assemble_plan(res, plan, 3))
    assert "plan was made with" in refused(lambda: nat.assemble_plan(res, plan, 1))
    assert "no result" in refused(lambda: nat.assemble_plan(None, plan, 2))
    short = nat.encode_batch_flat(*tgx.pack([b"ab", b"cd"]))
    assert "rows" in refused(lambda: nat.assemble_plan(short, plan, 2))
    nb, _, _ = nat.encode_batch_nbest_flat(*tgx.pack([b"ab", b"cd", b"ef"]), 2)   # an n-best result: 6 rows for 3 segments
    assert "rows" in refused(lambda: nat.assemble_plan(nb, plan, 2))
    assert "no room" in refused(lambda: nat.assemble_plan(res, plan, 0xFFFFFFFE - nat.vocab_size + 1))
    toks, scores, _ = synth.load_spec_vocab(32000)
    other = tgx.NativeModel(list(toks)[:-5], np.asarray(scores, np.float64)[:-5])
    assert "tokens" in refused(lambda: other.assemble_plan(res, plan, 2))
    # and the stage still works
    ok = nat.assemble_plan(res, plan, 2)
    V = nat.vocab_size
    assert ok.offsets().tolist()[0] == 0 and ok.num_samples == 3 and (ok.ids() >= V).sum() == 2 and ok.vocab_size == V + 2
    for r in (ok, short, nb, res):
        r.free()


def test_stage_times_are_the_front_ends_own():
    """front_last_times after a split: the five stages in order, every time finite and not negative; a normalize on the
    same thread in between leaves them as they were (each subsystem keeps its own)."""
    corpus = tgx.NativeCorpus(*tgx.pack([b"ab<s>cd", b"<s>", b"ef"]))
    segs, plan = corpus.split_specials([b"<s>", b"</s>"], False)
    assert plan.num_encoded == 3 and segs.num_bytes == 6   # every stage ran, the pack included
    times = _lib.front_last_times()
    assert list(times) == ["front_mark", "front_resolve", "front_segments", "front_keep", "front_pack"], times
    assert all(np.isfinite(v) and v >= 0 for v in times.values()), times
    other = tgx.NativeCorpus(*tgx.pack([b"cafe\xcc\x81", b"A\xcc\x8a and \xef\xbc\xa1", b"plain"]))   # combining marks, a fullwidth letter
    out = other.normalize("nfkc")
    assert out.n_pieces > 0 and list(_lib.norm_last_times()) == ["norm_mark", "norm_pieces", "norm_length", "norm_places", "norm_write"]
    assert _lib.front_last_times() == times
    for h in (out, other, segs, plan, corpus):
        h.free()


def test_a_plan_on_another_device_is_refused():
    if tgx.device_count() < 2:
        pytest.skip("needs two visible devices")
    toks, scores, _ = synth.load_spec_vocab(32000)
    far = tgx.NativeModel(list(toks), np.asarray(scores, np.float64), device=1)
    corpus = tgx.NativeCorpus(*tgx.pack([b"<s>", b"<s><s>"]))
    segs, plan = corpus.split_specials([b"<s>"], False)
    with pytest.raises(tgx.TokenGeeXError) as e:
        far.assemble_plan(None, plan, 1)
    assert e.value.status == _lib.ERR_INVALID and "device" in str(e.value)


# ---- Tokenizer level ---------------------------------------------------------------------------------------------

SPECIALS = ["<|endoftext|>", "<|fim", "<|fim|>", "<pad>", "<s>", "</s>"]   # "<|fim" is a prefix of "<|fim|>" and listed first: it wins


def _tokenizer(procs=("crlf",), specials=SPECIALS):
    toks, scores, _ = synth.load_spec_vocab(32000)
    processors = [tgx.CrlfProcessor() if p == "crlf" else tgx.UnicodeProcessor(p) for p in procs]
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors, list(specials))


@functools.lru_cache(maxsize=None)
def _batch():
    """test_assemble_gpu.py's texts: hand-written edge cases and mixed text with special tokens written into it"""
    flat, offs = synth.make_corpus(48 << 10, "mixed", max_len=4096, seed_offset=3)
    body = [bytes(flat[int(offs[i]):int(offs[i + 1])]).decode("utf-8", "ignore") for i in range(min(38, offs.size - 1))]
    texts = ["", "<|endoftext|>", "<s></s><pad><|fim|><|fim", "no special token in here", "a\r\n<s>\r\nb\r\n", "\r\n</s>", "a\r", "\n<s>\r",
             "é Å<|endoftext|>é", "<|fim|>prefix<|fim>suffix<|fim|middle", ""]
    for k, t in enumerate(body):
        cut = len(t) // 3
        texts.append(t[:cut] + "<|fim|>" + t[cut:2 * cut] + "<s>" * (k % 3) + "\r\n" + t[2 * cut:] + ("<|endoftext|>" if k % 2 else ""))
    texts += ["<pad>", ""]
    return tgx.pack([t.encode("utf-8") for t in texts])


@pytest.mark.parametrize("procs", [("crlf",), ()])
def test_encode_corpus_result(procs):
    tk = _tokenizer(procs)
    tk.seed = 4321
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)
    for dropout in (0.0, 0.3):
        want_ids, want_offs = tk.encode_batch_flat(flat, offs, dropout)
        res = tk.encode_corpus_result(corpus, dropout)
        assert res.vocab_size == tk.vocab_size() and res.num_samples == offs.size - 1
        assert np.array_equal(res.offsets(), want_offs) and np.array_equal(res.ids(), want_ids), (procs, dropout)
        res.free()
    assert not np.array_equal(tk.encode_batch_flat(flat, offs, 0.3)[0], tk.encode_batch_flat(flat, offs, 0.0)[0])
    assert (tk.encode_batch_flat(flat, offs, 0.0)[0] >= tk.base_vocab_size()).sum() > 50


def test_encode_corpus_sample_result():
    tk = _tokenizer()
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)
    want, want_logz = tk.encode_batch_sample_result_flat(flat, offs, 0.7, seed=99, return_logz=True)
    res, logz = tk.encode_corpus_sample_result(corpus, 0.7, seed=99, return_logz=True)
    assert logz.dtype == np.float64 and np.array_equal(logz, want_logz)
    assert not np.array_equal(want.ids(), tk.encode_batch_flat(flat, offs, 0.0)[0])
    _same(res, want, "sample")
    _same(tk.encode_corpus_sample_result(corpus, 0.7, seed=99), tk.encode_batch_sample_result_flat(flat, offs, 0.7, seed=99), "sample, no logz")


def test_encode_corpus_layouts():
    import torch
    tk = _tokenizer()
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)

    def same(a, b, key):
        assert set(a) == set(b), key
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (key, k)

    for kw in (dict(pad="<pad>", bos="<s>", eos="</s>", max_length=200, return_lengths=True),
               dict(pad="<pad>", eos="</s>", padding_side="left", dtype=torch.int32),
               dict(pad="<pad>", max_length=160, return_offsets_mapping="char"),
               dict(pad="<pad>", bos="<s>", max_length=96, return_offsets_mapping="byte", truncation_side="left"),
               dict(pad="<pad>", eos="</s>", max_length=64, stride=16, return_overflowing_tokens=True, return_offsets_mapping="char")):
        same(tk.encode_corpus_padded(corpus, **kw), tk.encode_batch_padded_flat(flat, offs, **kw), kw)
    for kw in (dict(pad="<pad>", eos="<|endoftext|>", return_doc=True), dict(pad="<pad>", bos="<s>", drop_last=True, dtype=torch.int32)):
        same(tk.encode_corpus_packed(corpus, 512, **kw), tk.encode_batch_packed_flat(flat, offs, 512, **kw), kw)
    tk.seed = 7
    same(tk.encode_corpus_packed(corpus, 256, 0.3, pad="<pad>"), tk.encode_batch_packed_flat(flat, offs, 256, 0.3, pad="<pad>"), "dropout")
    empty = tgx.NativeCorpus(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    same(tk.encode_corpus_padded(empty, pad="<pad>", bos="<s>"), tk.encode_batch_padded_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64), pad="<pad>", bos="<s>"), "empty")
    same(tk.encode_corpus_packed(empty, 16, pad="<pad>", return_doc=True), tk.encode_batch_packed_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 16, pad="<pad>", return_doc=True), "empty packed")


def test_round_trip_under_a_second_tokenizer():
    """decode -> to_corpus() -> encode_corpus_result under a tokenizer with other special tokens: what the second
    tokenizer's encode_batch_flat gives for the downloaded text"""
    first = _tokenizer()
    second = _tokenizer(("crlf",), specials=["<s>", "\n\n", "<|fim|>", "prefix", "<|endoftext|"])
    flat, offs = _batch()
    res = first.encode_corpus_result(tgx.NativeCorpus(flat, offs))
    text = first.decode_result_text(res, True)
    res.free()
    t_flat, t_offs = text.bytes(), text.offsets()
    assert t_offs.size == offs.size and t_flat.size > 40_000
    corpus = text.to_corpus()
    text.free()
    want_ids, want_offs = second.encode_batch_flat(t_flat, t_offs)
    got = second.encode_corpus_result(corpus)
    assert np.array_equal(got.offsets(), want_offs) and np.array_equal(got.ids(), want_ids)
    assert got.vocab_size == second.vocab_size() and (want_ids >= second.base_vocab_size()).sum() > 50
    got.free()


def test_tokenizers_without_special_tokens_or_processors():
    flat, offs = _batch()
    corpus = tgx.NativeCorpus(flat, offs)
    for procs in (("crlf",), ()):
        tk = _tokenizer(procs, specials=[])
        want_ids, want_offs = tk.encode_batch_flat(flat, offs)
        res = tk.encode_corpus_result(corpus)
        assert np.array_equal(res.offsets(), want_offs) and np.array_equal(res.ids(), want_ids) and res.vocab_size == tk.base_vocab_size(), procs
        res.free()
        a, la = tk.encode_corpus_sample_result(corpus, 0.3, seed=5, return_logz=True)
        ids, o = a.ids(), a.offsets()
        a.free()
        if procs:
            continue   # (the flat route hashes a sample by its index among all samples, the split by that among the non-empty ones)
        w_ids, w_offs, w_logz = tk.encode_batch_sample_flat(flat, offs, 0.3, seed=5, return_logz=True)
        assert np.array_equal(ids, w_ids) and np.array_equal(o, w_offs) and np.array_equal(la, w_logz)


def test_processor_lists_the_device_front_end_does_not_take():
    corpus = tgx.NativeCorpus(*tgx.pack([b"a\r\n<s>b"]))
    for procs in (("nfc",), ("crlf", "nfkc"), ("crlf", "crlf")):
        tk = _tokenizer(procs)
        for call in (lambda: tk.encode_corpus_result(corpus), lambda: tk.encode_corpus_sample_result(corpus, 0.5, seed=1),
                     lambda: tk.encode_corpus_padded(corpus, pad="<pad>"), lambda: tk.encode_corpus_packed(corpus, 8, pad="<pad>")):
            with pytest.raises(tgx.TokenGeeXError) as e:
                call()
            assert e.value.status == _lib.ERR_UNSUPPORTED and "encode_batch_result_flat" in str(e.value), procs
