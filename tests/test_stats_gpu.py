"""Per-sample lattice statistics on the GPU (tgx_lattice_stats_batch / tgx_lattice_stats_corpus): both kernels against the
80-bit truth on the shared case list (tests/stats_cases.py), the batch and corpus forms, log Z against sampling's, the
range fallback, the kernel selection at |alpha * score| = 207 / 207.5, samples without a path, and the Tokenizer level.

Bounds.  logz: tests/test_sample_gpu.py::_assert_logz_truth's (rows 1e-13 max(1, |truth|); generic 64 sqrt(n) 2^-52
|truth| + 1e-13).  escore, etokens on stats_rows_kernel: the linear-domain gate of util.assert_estep_truth, 1e-10
max(1, |truth|).  On stats_kernel, over the shared case list: 4 x the largest distance of the f64 host twin (the same
recurrences) from the truth, measured on the CPU over stats_cases.TWIN_RUNS — escore 4.89e-14, etokens 8.78e-15 relative
to max(1, |truth|), so the bounds are 1.96e-13 and 3.52e-14 max(1, |truth|).  entropy: (bound on logz) + alpha * (bound
on escore).  No sample is excused.  Largest distances observed on an MI355X: stats_rows_kernel
escore 5.7e-15, etokens 3.7e-15, log Z at 0.036 of its bound; stats_kernel escore 4.87e-14, etokens 8.78e-15 (the twin's
figures to two digits), log Z at 0.045 of its bound."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib
from tokengeex_amd.tokenizer import split_special_tokens

import hostile_cases as hc
import stats_cases as sx

STATS_KERNELS = {"sample_wslot_kernel", "stats_rows_kernel", "stats_kernel"}
RAN = {"rows": {"sample_wslot_kernel", "stats_rows_kernel"}, "generic": {"stats_kernel"},
       "fallback": {"sample_wslot_kernel", "stats_rows_kernel", "stats_kernel"}}


@functools.lru_cache(maxsize=None)
def _native(name):
    toks, scores = sx.vocab(name)
    return tgx.NativeModel(toks, scores)


@pytest.fixture
def stats_path(monkeypatch, request):
    if request.param != "auto":
        monkeypatch.setenv("TGX_STATS_PATH", request.param)
    return request.param


def _stats(native, texts, alpha, corpus=False):
    """-> (LatticeStats, the statistics kernels that ran)"""
    flat, offs = tgx.pack(texts)
    st = native.lattice_stats_corpus(tgx.NativeCorpus(flat, offs), alpha) if corpus else native.lattice_stats_flat(flat, offs, alpha)
    return st, set(native.last_kernel_times()) & STATS_KERNELS


def _bits(st):
    return [np.asarray(a).view(np.uint64) for a in (st.logz, st.expected_score, st.expected_tokens)]


def _same(a, b):
    for x, y in zip(_bits(a), _bits(b)):
        assert np.array_equal(x, y)
    assert a.n_no_path == b.n_no_path and np.array_equal(a.n_bytes, b.n_bytes)


def _assert_truth(what, st, alpha, z, es, et, n, rows, shared=True):
    """Every sample within the bounds of the module docstring; off the shared case list the generic kernel gets the
    reasoned bound of the twin's formulation (stats_cases.twin_bound)."""
    zb = sx.logz_bound(rows, n, z)
    if rows:
        eb, tb = sx.ROWS_RTOL * np.maximum(1.0, np.abs(es)), sx.ROWS_RTOL * np.maximum(1.0, np.abs(et))
    elif shared:
        eb, tb = sx.GENERIC_ESCORE_BOUND * np.maximum(1.0, np.abs(es)), sx.GENERIC_ETOKENS_BOUND * np.maximum(1.0, np.abs(et))
    else:
        eb, tb = sx.twin_bound(n, z, es), sx.twin_bound(n, z, et)
    dz, de, dt = np.abs(st.logz - z), np.abs(st.expected_score - es), np.abs(st.expected_tokens - et)
    dh = np.abs(st.entropy - (z - alpha * es))
    print(f"[stats] {what} {'rows' if rows else 'generic'} alpha {alpha}: logz err/bound {float((dz / zb).max()):.3g}, "
          f"escore dist {sx.distance(st.expected_score, es):.3g}, etokens dist {sx.distance(st.expected_tokens, et):.3g}, "
          f"entropy err/bound {float((dh / (zb + alpha * eb)).max()):.3g}")
    assert st.n_no_path == 0 and not st.no_path.any()
    assert np.all(dz <= zb), (what, int(np.argmax(dz / zb)), dz.max())
    assert np.all(de <= eb), (what, int(np.argmax(de / eb)), de.max())
    assert np.all(dt <= tb), (what, int(np.argmax(dt / tb)), dt.max())
    assert np.all(dh <= zb + alpha * eb), (what, int(np.argmax(dh)), dh.max())


CASES = [("vocab_32000", p, a) for p in ("generic", "rows") for a in sx.ALPHAS] + \
        [("long24", "rows", 0.1), ("long24", "rows", 1.0), ("long40", "auto", 1.0), ("long64", "auto", 1.0)]


@pytest.mark.parametrize("vocab,stats_path,alpha", CASES, indirect=["stats_path"])
def test_against_the_truth(vocab, stats_path, alpha):
    native = _native(vocab)
    st, ran = _stats(native, sx.texts(), alpha)
    rows = stats_path == "rows"
    assert ran == RAN["rows" if rows else "generic"], ran
    assert st.alpha == alpha and np.array_equal(st.n_bytes, sx.LENGTHS)
    assert (st.logz[0], st.expected_score[0], st.expected_tokens[0]) == (0.0, 0.0, 0.0)  # the empty sample
    z, es, et = sx.truth(vocab, alpha)
    _assert_truth(vocab, st, alpha, z, es, et, sx.lens(), rows)
    if alpha == 0.0:  # uniform: the entropy is log Z
        assert np.all(np.abs(st.entropy - st.logz) == 0.0)


@pytest.mark.parametrize("stats_path", ["generic", "rows"], indirect=True)
def test_batch_is_corpus_and_a_second_call_is_the_first(stats_path):
    native = _native("vocab_32000")
    a, ran = _stats(native, sx.texts(), 1.0)
    assert ran == RAN[stats_path]
    b, ran_b = _stats(native, sx.texts(), 1.0, corpus=True)
    assert ran_b == ran
    _same(a, b)
    flat, offs = tgx.pack(sx.texts())
    corpus = tgx.NativeCorpus(flat, offs)
    _same(native.lattice_stats_corpus(corpus, 1.0), native.lattice_stats_corpus(corpus, 1.0))
    _same(a, native.lattice_stats_corpus(corpus, 1.0))
    # a batch without samples, and outputs that are not asked for
    empty = native.lattice_stats_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 1.0)
    assert len(empty) == 0 and empty.n_no_path == 0
    lz = np.zeros(len(sx.texts()))
    bad = _lib.C.c_uint64(7)
    assert _lib.lib.tgx_lattice_stats_batch(native._h, _lib.ptr(flat), _lib.ptr(offs), len(sx.texts()), 1.0, None, None, None, _lib.C.byref(bad)) == 0
    assert bad.value == 0
    assert _lib.lib.tgx_lattice_stats_batch(native._h, _lib.ptr(flat), _lib.ptr(offs), len(sx.texts()), 1.0, _lib.ptr(lz), None, None, None) == 0
    assert np.array_equal(lz.view(np.uint64), a.logz.view(np.uint64))


@pytest.mark.parametrize("path", ["generic", "rows"])
@pytest.mark.parametrize("alpha", [0.1, 1.0])
def test_logz_is_sampling_logz_bit_for_bit(path, alpha, monkeypatch):
    """The statistics kernels take the forward value through the operations of their sampling counterparts in the same
    order, so log Z is the same double."""
    native = _native("vocab_32000")
    flat, offs = tgx.pack(sx.texts())
    monkeypatch.setenv("TGX_STATS_PATH", path)
    if path == "generic":
        monkeypatch.setenv("TGX_SAMPLE_PATH", "generic")
    st = native.lattice_stats_flat(flat, offs, alpha)
    assert set(native.last_kernel_times()) & STATS_KERNELS == RAN[path]
    res, z = native.encode_batch_sample_flat(flat, offs, alpha, 5, return_logz=True)
    res.free()
    assert ("sample_rows_kernel" in native.last_kernel_times()) == (path == "rows")
    assert np.array_equal(st.logz.view(np.uint64), np.asarray(z).view(np.uint64))


def _truth_of(toks, scores, alpha, texts):
    om = orc.OracleModel(toks, alpha * np.asarray(scores, np.float64))
    out = [om.marginal_ext(t) for t in texts]
    return (np.array([z for _, z in out]), np.array([float(np.dot(e, scores)) for e, _ in out]), np.array([float(e.sum()) for e, _ in out]),
            np.array([len(t) for t in texts], np.float64))


def test_fallback(monkeypatch):
    """The designed trigger of tests/hostile_cases.py (byte tokens at -100, 40 bytes that only they cover): the rows kernel
    raises the flag, the whole call runs again on stats_kernel and is the forced generic path's result bit for bit; an
    in-range call on the same model afterwards runs the rows kernel alone."""
    trip, stay = hc.sampling_case("designed_trip"), hc.sampling_case("designed_stay")
    native = tgx.NativeModel(trip["toks"], trip["scores"])
    got, ran = _stats(native, trip["texts"], trip["alpha"])
    assert ran == RAN["fallback"], ran
    monkeypatch.setenv("TGX_STATS_PATH", "generic")
    forced, ran_f = _stats(native, trip["texts"], trip["alpha"])
    monkeypatch.delenv("TGX_STATS_PATH")
    assert ran_f == RAN["generic"]
    _same(got, forced)
    _same(got, _stats(native, trip["texts"], trip["alpha"], corpus=True)[0])
    _assert_truth("designed_trip", got, trip["alpha"], *_truth_of(trip["toks"], trip["scores"], trip["alpha"], trip["texts"]), rows=False, shared=False)
    after, ran_a = _stats(native, stay["texts"], stay["alpha"])
    assert ran_a == RAN["rows"], ran_a
    _assert_truth("designed_stay", after, stay["alpha"], *_truth_of(stay["toks"], stay["scores"], stay["alpha"], stay["texts"]), rows=True)
    _same(got, _stats(native, trip["texts"], trip["alpha"])[0])  # and a fallback again after it


@pytest.mark.parametrize("name", ["score207", "score207_5"])
def test_the_switch_at_207(name):
    """The most negative alpha * score at -207.0: the rows kernel, unforced (w = 2^-298.6 on the path of every text with a
    z); at -207.5: the generic kernel."""
    c = hc.sampling_case(name)
    native = tgx.NativeModel(c["toks"], c["scores"])
    st, ran = _stats(native, c["texts"], c["alpha"])
    assert ran == RAN[c["expect"]], ran
    _assert_truth(name, st, c["alpha"], *_truth_of(c["toks"], c["scores"], c["alpha"], c["texts"]), rows=c["expect"] == "rows", shared=False)


@pytest.mark.parametrize("stats_path", ["generic", "rows"], indirect=True)
def test_no_path_in_the_middle_of_a_batch(stats_path):
    """A vocabulary without 0xFF and two samples that hold it, between samples that have a path: TGX_OK, the two are marked
    as the twin marks them (-inf, NaN, NaN, counted) and the other samples' values are what they are without them."""
    c = hc.sampling_case("nopath_stay")
    native = tgx.NativeModel(c["toks"], c["scores"])
    good = list(c["texts"])
    texts = good[:2] + [hc.NOPATH_BAD[0]] + good[2:9] + [hc.NOPATH_BAD[1]] + good[9:]
    bad = [2, 10]
    st, ran = _stats(native, texts, c["alpha"])
    assert ran == RAN[stats_path]
    twin = _lib.lattice_stats_host(c["toks"], c["scores"], *tgx.pack(texts), c["alpha"])
    assert st.n_no_path == twin.n_no_path == 2 and np.array_equal(st.no_path, twin.no_path) and np.nonzero(st.no_path)[0].tolist() == bad
    assert np.all(np.isneginf(st.logz[bad])) and np.all(np.isnan(st.expected_score[bad])) and np.all(np.isnan(st.expected_tokens[bad]))
    assert np.all(np.isnan(st.entropy[bad]))
    alone, _ = _stats(native, good, c["alpha"])
    keep = [i for i in range(len(texts)) if i not in bad]
    for x, y in zip(_bits(st), _bits(alone)):
        assert np.array_equal(x[keep], y)
    # (no 80-bit truth here: the oracle's marginal is kept to vocabularies with full byte cover.)  The twin and the kernel
    # are each within their bound of the truth
    tw = _lib.lattice_stats_host(c["toks"], c["scores"], *tgx.pack(good), c["alpha"])
    n, rows = np.array([len(t) for t in good], np.float64), stats_path == "rows"
    assert np.all(np.abs(alone.logz - tw.logz) <= sx.logz_bound(rows, n, tw.logz) + sx.logz_bound(False, n, tw.logz))
    for got, want in ((alone.expected_score, tw.expected_score), (alone.expected_tokens, tw.expected_tokens)):
        own = sx.ROWS_RTOL * np.maximum(1.0, np.abs(want)) if rows else sx.twin_bound(n, tw.logz, want)
        assert np.all(np.abs(got - want) <= own + sx.twin_bound(n, tw.logz, want))


def test_argument_errors_are_sampling_s():
    native = _native("vocab_32000")
    flat, offs = tgx.pack(sx.texts()[:4])
    for alpha in (-0.1, float("nan"), float("inf")):
        with pytest.raises(tgx.TokenGeeXError) as smp:
            native.encode_batch_sample_flat(flat, offs, alpha, 1)
        with pytest.raises(tgx.TokenGeeXError) as got:
            native.lattice_stats_flat(flat, offs, alpha)
        assert got.value.status == smp.value.status == _lib.ERR_INVALID
        with pytest.raises(tgx.TokenGeeXError) as got:
            native.lattice_stats_corpus(tgx.NativeCorpus(flat, offs), alpha)
        assert got.value.status == _lib.ERR_INVALID
    toks, scores = sx.tiny()
    s = scores.copy()
    s[2] = -1e308
    huge = tgx.NativeModel(toks, s)
    f2, o2 = tgx.pack([b"ab"])
    with pytest.raises(tgx.TokenGeeXError) as smp:
        huge.encode_batch_sample_flat(f2, o2, 100.0, 1)
    with pytest.raises(tgx.TokenGeeXError) as got:
        huge.lattice_stats_flat(f2, o2, 100.0)
    assert got.value.status == smp.value.status == _lib.ERR_INVALID
    s[2] = float("-inf")
    inf = tgx.NativeModel(toks, s)
    with pytest.raises(tgx.TokenGeeXError) as smp:
        inf.encode_batch_sample_flat(f2, o2, 1.0, 1)
    with pytest.raises(tgx.TokenGeeXError) as got:
        inf.lattice_stats_flat(f2, o2, 1.0)
    assert got.value.status == smp.value.status == _lib.ERR_UNSUPPORTED


SPECIALS = ["<|eos|>", "<|pad|>"]
TK_TEXTS = ["hello world<|eos|>def f(x):\r\n    return x\r\n", "<|eos|>", "plain text only", "", "a", "<|pad|><|pad|>tail\r\n<|eos|>",
            "line one\r\nline two<|eos|>line three\r\n<|pad|>", "x = [i for i in range(10)]"]


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores = sx.vocab("vocab_32000")
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors=[tgx.CrlfProcessor()], special_tokens=SPECIALS)


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_tokenizer_sums_the_segments(alpha):
    tk = _tokenizer()
    st = tk.lattice_stats(TK_TEXTS, alpha)
    assert len(st) == len(TK_TEXTS) and np.array_equal(st.n_bytes, [len(t.encode()) for t in TK_TEXTS]) and st.n_no_path == 0
    segs, owner, n_special = [], [], np.zeros(len(TK_TEXTS))
    for i, t in enumerate(TK_TEXTS):
        for piece, special in split_special_tokens(t, SPECIALS):
            if special:
                n_special[i] += 1
            else:
                segs.append(piece.replace("\r\n", "\n").encode())
                owner.append(i)
    seg = tk.native_model().lattice_stats_flat(*tgx.pack(segs), alpha)
    owner = np.array(owner)
    for got, part in ((st.logz, seg.logz), (st.expected_score, seg.expected_score), (st.expected_tokens - n_special, seg.expected_tokens)):
        want = np.bincount(owner, weights=part, minlength=len(TK_TEXTS))
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)  # (the same doubles, added in another order at most)
    assert st.expected_tokens[1] == 1.0 and st.logz[1] == 0.0 and (st.logz[3], st.expected_tokens[3]) == (0.0, 0.0)
    # the resident corpus, through the device front end
    corpus = tgx.NativeCorpus(*tgx.pack([t.encode() for t in TK_TEXTS]))
    via = tk.lattice_stats_corpus(corpus, alpha)
    for a, b in zip((st.logz, st.expected_score, st.expected_tokens), (via.logz, via.expected_score, via.expected_tokens)):
        np.testing.assert_allclose(b, a, rtol=1e-13, atol=1e-13)
    assert np.array_equal(via.n_bytes, st.n_bytes) and via.n_no_path == 0
    flat_form = tk.lattice_stats_flat(*tgx.pack([t.encode() for t in TK_TEXTS]), alpha)
    _same(st, flat_form)


def test_tokenizer_no_path_and_large_alpha():
    tk = _tokenizer()
    toks, scores = sx.vocab("vocab_32000")
    alpha = 206.0 / float(np.abs(scores).max())  # |alpha * score| <= 207 holds: the rows kernel takes it
    st = tk.lattice_stats(TK_TEXTS, alpha)
    assert "stats_rows_kernel" in tk.native_model().last_kernel_times()
    rows = tk.encode_batch(TK_TEXTS, 0.0)
    sharp = np.nonzero(st.entropy < 1e-3)[0]
    assert 1 in sharp and 3 in sharp  # a lone special token and the empty text have one segmentation
    for i in sharp:
        assert abs(st.expected_tokens[i] - len(rows[i])) < 0.5, (i, st.expected_tokens[i], len(rows[i]))
    # one unreachable segment makes its sample no_path
    part = tgx.Tokenizer([(b"a", -1.0, False), (b"b", -1.5, False), (b"ab", -1.2, False)], special_tokens=["<|eos|>"])
    got = part.lattice_stats(["ab<|eos|>abx", "ab<|eos|>ba", "x", "<|eos|>"], 1.0)
    assert got.no_path.tolist() == [True, False, True, False] and got.n_no_path == 2
    assert np.isneginf(got.logz[0]) and np.isnan(got.expected_tokens[0]) and np.isnan(got.expected_score[0])
    assert got.expected_tokens[3] == 1.0 and got.logz[3] == 0.0
