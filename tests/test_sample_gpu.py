"""Sampling a segmentation from the lattice on the GPU (tgx_encode_batch_sample / tgx_encode_corpus_sample): both kernels
against the Python checker (tests/sample_checker.py), the law of the draw, log Z, the large-alpha limit, validity at
scale and the plumbing."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, synth

import sample_checker as sc

SEED = 0x5EED5A3B1E
ALPHAS = [0.0, 0.1, 1.0]


@functools.lru_cache(maxsize=None)
def _corpus():
    """~256 KiB of mixed text in samples of up to 8 KiB, plus one sample of 70 000 bytes (longer than 64 KiB)."""
    flat, offs = synth.make_corpus(256 << 10, "mixed", max_len=8192, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    texts = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)] + [bytes(big[:70_000])]
    return texts


@functools.lru_cache(maxsize=None)
def _vocab(name):
    if name in ("vocab_32000", "vocab_65536"):
        toks, scores, _ = synth.load_spec_vocab(int(name.split("_")[1]))
        return list(toks), np.asarray(scores, np.float64)
    flat, _ = synth.make_corpus(1 << 20, "mixed", seed_offset=5)
    if name == "long24":
        toks, scores = synth.build_vocab(flat, 4000, 24)
        assert 17 <= max(map(len, toks)) <= 32
        return list(toks), np.asarray(scores, np.float64)
    # a 40-byte token (a substring the corpus holds) on top of a short-token vocabulary: only the generic kernel takes it
    toks, scores = synth.build_vocab(flat, 4000, 16)
    text = _corpus()[-1]
    toks, scores = list(toks) + [text[1000:1040]], np.append(np.asarray(scores, np.float64), -3.0)
    return toks, scores


@functools.lru_cache(maxsize=None)
def _native(name):
    toks, scores = _vocab(name)
    return tgx.NativeModel(toks, scores)


@functools.lru_cache(maxsize=None)
def _incoming(name):
    toks, scores = _vocab(name)
    om = orc.OracleModel(toks, scores)
    ml = max(map(len, toks))
    return [sc.incoming(om, t, ml) for t in _corpus()]


@functools.lru_cache(maxsize=None)
def _checked(name, alpha, viterbi=False):
    toks, scores = _vocab(name)
    return [sc.check_sample(inc, scores, len(t), alpha, SEED, i, viterbi=viterbi)
            for i, (inc, t) in enumerate(zip(_incoming(name), _corpus()))]


@functools.lru_cache(maxsize=None)
def _logz_truth(name, alpha):
    """Per-sample log Z in 80-bit extended precision: orc_marginal_ext on the model with scores alpha * scores (the
    corpus vocabularies cover every byte, so the lattice quirks do not apply)."""
    toks, scores = _vocab(name)
    om = orc.OracleModel(toks, alpha * scores)
    return np.array([om.marginal_ext(t)[1] for t in _corpus()])


def _assert_logz_truth(name, alpha, logz, kernels):
    """sample_rows_kernel (linear domain, exact power-of-two rescales): |logz - truth| <= 1e-13 max(1, |truth|) (measured:
    5e-15 relative at most).
    sample_kernel (log domain): each of the n positions adds a log-sum-exp whose rounding is ~ulp(|z_p|) at the running
    |z_p| <= |z|, and those roundings random-walk: the error is ~sqrt(n) ulp(|z|) = sqrt(n) 2^-52 |z|, the model of the
    E-step's log-domain kernels (tests/test_estep_pairs_gpu.py, rtol_for).  Several roundings per step (exp, log1p, the
    adds, a sum over the incoming tokens) make the factor in front larger than 1: measured 14 at the longest sample (2.5e-8 at the
    70 000-byte sample with alpha 0, |z| = 3.2e4; 1.2e-8 at |z| = 1.7e5), so the bound is 64 sqrt(n) 2^-52 |z| + 1e-13:
    1e-7 .. 6e-7 absolute at that sample, against today's 1e-9 |z| = 3e-5 .. 1.7e-4."""
    truth = _logz_truth(name, alpha)
    lens = np.array([len(t) for t in _corpus()], np.float64)
    if "sample_rows_kernel" in kernels:
        bound = 1e-13 * np.maximum(1.0, np.abs(truth))
    else:
        assert "sample_kernel" in kernels, kernels
        bound = 64.0 * np.sqrt(np.maximum(lens, 1.0)) * 2.0 ** -52 * np.abs(truth) + 1e-13
    err = np.abs(np.asarray(logz) - truth)
    i = int(np.argmax(err / bound))
    assert np.all(err <= bound), (i, len(_corpus()[i]), logz[i], truth[i], err[i], bound[i])


def _rows(res):
    ids, oo = res.ids(), res.offsets()
    res.free()
    return [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]


def _sample(native, texts, alpha, seed=SEED, logz=False):
    flat, offs = tgx.pack(texts)
    if logz:
        res, z = native.encode_batch_sample_flat(flat, offs, alpha, seed, return_logz=True)
        return _rows(res), z
    return _rows(native.encode_batch_sample_flat(flat, offs, alpha, seed))


@pytest.fixture
def sample_path(monkeypatch, request):
    monkeypatch.setenv("TGX_SAMPLE_PATH", request.param)
    return request.param


CASES = [("vocab_32000", "generic"), ("vocab_32000", "rows"), ("vocab_65536", "generic"), ("vocab_65536", "rows"),
         ("long24", "generic"), ("long24", "rows"), ("long40", "generic")]


@pytest.mark.parametrize("vocab,sample_path", CASES, indirect=["sample_path"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_ids_match_the_checker(vocab, sample_path, alpha):
    native = _native(vocab)
    got, logz = _sample(native, _corpus(), alpha, logz=True)
    names = native.last_kernel_times()
    if sample_path == "rows":
        assert "sample_rows_kernel" in names and "sample_kernel" not in names, names
    else:
        assert "sample_kernel" in names and "sample_rows_kernel" not in names, names
    want = _checked(vocab, alpha)
    _assert_logz_truth(vocab, alpha, logz, names)
    close = 0
    for i, w in enumerate(want):
        assert abs(logz[i] - w["logz"]) <= 1e-9 * max(1.0, abs(w["logz"])), (i, logz[i], w["logz"])
        if got[i] != w["ids"]:
            assert w["gap"] < 1e-6, (i, w["gap"])
            close += 1
    assert close < 0.01 * len(want), close


def _tiny():
    toks = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"cab"]
    scores = np.array([-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2])
    return toks, scores


@pytest.mark.parametrize("sample_path", ["generic", "rows"], indirect=True)
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_distribution(sample_path, alpha):
    toks, scores = _tiny()
    text = b"abcabca"
    inc = sc.incoming(orc.OracleModel(toks, scores), text, 3)
    probs, _ = sc.segmentation_probs(inc, scores, len(text), alpha)
    N = 50_000
    native = tgx.NativeModel(toks, scores)
    got = _sample(native, [text] * N, alpha, seed=99)
    assert ("sample_rows_kernel" in native.last_kernel_times()) == (sample_path == "rows")
    cnt = {}
    for row in got:
        cnt[tuple(row)] = cnt.get(tuple(row), 0) + 1
    assert set(cnt) <= set(probs)
    if alpha == 0.0:
        assert all(abs(p - 1.0 / len(probs)) < 1e-12 for p in probs.values())
    tv = 0.5 * sum(abs(cnt.get(s, 0) / N - p) for s, p in probs.items())
    assert tv < 0.02, tv
    for s, p in probs.items():
        if p >= 0.01:
            assert abs(cnt.get(s, 0) / N - p) <= 5 * math.sqrt(p * (1 - p) / N), (s, p, cnt.get(s, 0) / N)


@pytest.mark.parametrize("sample_path", ["generic", "rows"], indirect=True)
@pytest.mark.parametrize("alpha", [0.1, 1.0])
def test_logz_matches_the_marginal_and_the_estep(sample_path, alpha):
    toks, scores = _vocab("vocab_32000")
    native = _native("vocab_32000")
    texts = _corpus()
    _, logz = _sample(native, texts, alpha, logz=True)
    om = orc.OracleModel(toks, alpha * scores)
    _assert_logz_truth("vocab_32000", alpha, logz, native.last_kernel_times())
    for i, t in enumerate(texts):
        if len(t) <= 81920:
            _, z = om.marginal(t)
            assert abs(logz[i] - z) <= 1e-9 * max(1.0, abs(z)), (i, logz[i], z)
    if alpha == 1.0:
        flat, offs = tgx.pack(texts)
        corpus = tgx.NativeCorpus(flat, offs)
        _, zsum = native.estep(corpus, snippet_len=max(map(len, texts)) + 1)
        assert abs(logz.sum() - zsum) <= 1e-9 * max(1.0, abs(zsum)), (logz.sum(), zsum)


@pytest.mark.parametrize("sample_path", ["generic", "rows"], indirect=True)
def test_large_alpha_is_encode_and_alpha_one_is_not(sample_path):
    native = _native("vocab_32000")
    texts = _corpus()
    enc = _rows(native.encode_batch_flat(*tgx.pack(texts)))
    hot = _sample(native, texts, 1e5)
    checked = _checked("vocab_32000", 1e5, viterbi=True)
    excluded = 0
    for i, c in enumerate(checked):
        assert c["vids"] == enc[i]
        if c["vgap"] < 0.01:
            excluded += 1
        else:
            assert hot[i] == enc[i], i
    # (the spec vocabulary's scores are quantised: exact Viterbi ties — where encode's longer-token rule and the race
    # legitimately part — sit on the path of about one kilobyte sample in six; a competitor within 0.01 is a key gap of
    # 1000 at this alpha, against Gumbel noise of at most 41, so every other sample must be encode's)
    assert excluded < 0.5 * len(texts), excluded
    warm = _sample(native, texts, 1.0)
    longer = [i for i, t in enumerate(texts) if len(t) > 100]
    assert sum(warm[i] != enc[i] for i in longer) > 0.5 * len(longer)


def test_validity_at_scale():
    toks, scores = _vocab("vocab_32000")
    native = _native("vocab_32000")
    flat, offs = synth.make_corpus(64 << 20, "mixed")
    corpus = tgx.NativeCorpus(flat, offs)
    res = native.encode_corpus_sample(corpus, 0.5, SEED)
    assert "sample_rows_kernel" in native.last_kernel_times()
    ids, oo = res.ids(), res.offsets()
    res.free()
    V = len(toks)
    assert ids.size and int(ids.max()) < V
    vflat, voffs = tgx.pack(toks)
    lens = np.diff(voffs.astype(np.int64))[ids]
    starts = voffs[:-1].astype(np.int64)[ids]
    out_pos = np.concatenate([[0], np.cumsum(lens)[:-1]])
    idx = np.repeat(starts - out_pos, lens) + np.arange(int(lens.sum()))
    assert np.array_equal(vflat[idx], flat)
    per_sample = np.add.reduceat(lens, oo[:-1].astype(np.int64)) if ids.size else np.zeros(0)
    assert np.array_equal(per_sample, np.diff(offs.astype(np.int64)))


def test_plumbing():
    native = _native("vocab_32000")
    texts = _corpus()[:64]
    a = _sample(native, texts, 0.5, seed=1)
    assert _sample(native, texts, 0.5, seed=1) == a
    b = _sample(native, texts, 0.5, seed=2)
    longer = [i for i, t in enumerate(texts) if len(t) > 100]
    assert sum(a[i] != b[i] for i in longer) > 0.5 * len(longer)
    # the corpus form is the batch form
    flat, offs = tgx.pack(texts)
    corpus = tgx.NativeCorpus(flat, offs)
    res, z = native.encode_corpus_sample(corpus, 0.5, 1, return_logz=True)
    assert _rows(res) == a
    _, z2 = native.encode_batch_sample_flat(flat, offs, 0.5, 1, return_logz=True)
    assert np.array_equal(z, z2)
    # invalid temperatures
    for alpha in (-0.1, float("nan"), float("inf")):
        with pytest.raises(tgx.TokenGeeXError) as e:
            native.encode_batch_sample_flat(flat, offs, alpha, 1)
        assert e.value.status == _lib.ERR_INVALID


def test_no_path_is_reported_as_encode_does():
    toks = [b"a", b"b", b"ab"]
    native = tgx.NativeModel(toks, [-1.0, -1.0, -1.5])
    flat, offs = tgx.pack([b"abab", b"ab", b"abx", b"xa", b"b"])
    with pytest.raises(tgx.TokenGeeXError) as enc:
        native.encode_batch_flat(flat, offs)
    with pytest.raises(tgx.TokenGeeXError) as smp:
        native.encode_batch_sample_flat(flat, offs, 1.0, 3)
    assert smp.value.status == enc.value.status == _lib.ERR_NO_PATH
    assert str(smp.value) == str(enc.value)
    assert (smp.value.sample, smp.value.pos, smp.value.length) == (enc.value.sample, enc.value.pos, enc.value.length) == (2, 3, 3)


def test_tokenizer_keeps_specials():
    toks, scores = _vocab("vocab_32000")
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], special_tokens=["<|eos|>"])
    eos = tk.special_token_to_id("<|eos|>")
    texts = ["hello world<|eos|>def f(x): return x", "<|eos|>", "plain text only"]
    rows = tk.encode_batch_sample(texts, 1.0, seed=5)
    assert rows == tk.encode_batch_sample(texts, 1.0, seed=5)
    for t, r in zip(texts, rows):
        assert r.count(eos) == t.count("<|eos|>")
        assert tk.decode(r, True) == t
    flat, offs = tgx.pack([t.encode() for t in texts])
    ids, oo, logz = tk.encode_batch_sample_flat(flat, offs, 1.0, seed=5, return_logz=True)
    assert [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(len(texts))] == rows
    om = orc.OracleModel(toks, scores)
    want = [om.marginal(b"hello world")[1] + om.marginal(b"def f(x): return x")[1], 0.0, om.marginal(b"plain text only")[1]]
    for g, w in zip(logz, want):
        assert abs(g - w) <= 1e-9 * max(1.0, abs(w))
    assert tk.encode_sample(texts[0], 1.0, seed=5) == rows[0]
