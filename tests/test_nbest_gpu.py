"""N-best segmentation on the GPU (tgx_encode_batch_nbest / tgx_encode_corpus_nbest): ids, scores and n_found against
the Python checker (tests/nbest_checker.py) on four vocabularies, against encode, the rows' own properties, the chunked
path, errors, the tokenizer level with special tokens, n-best sampling and the host A* of prune_alternatives."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, synth

import nbest_checker as nc
import sample_checker as sc

KS = [1, 3, 8, 16]


@functools.lru_cache(maxsize=None)
def _corpus():
    """~256 KiB of mixed text in samples of up to 8 KiB, plus one sample of 70 000 bytes (longer than 64 KiB)."""
    flat, offs = synth.make_corpus(256 << 10, "mixed", max_len=8192, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    return [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)] + [bytes(big[:70_000])]


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
    toks, scores = synth.build_vocab(flat, 4000, 16)  # plus one 40-byte token the corpus holds
    text = _corpus()[-1]
    return list(toks) + [text[1000:1040]], np.append(np.asarray(scores, np.float64), -3.0)


@functools.lru_cache(maxsize=None)
def _native(name):
    return tgx.NativeModel(*_vocab(name))


@functools.lru_cache(maxsize=None)
def _checked(name):
    """The checker's k = 16 lists of every sample (the rows for a smaller k are their first k: test_nbest_cpu.py)."""
    toks, scores = _vocab(name)
    om = orc.OracleModel(toks, scores)
    ml = max(map(len, toks))
    return [nc.nbest(sc.incoming(om, t, ml), scores, len(t), 16) for t in _corpus()]


def _nbest(native, texts, k):
    res, scores, nf = native.encode_batch_nbest_flat(*tgx.pack(texts), k)
    assert res.num_samples == len(texts) * k
    ids, oo = res.ids(), res.offsets()
    res.free()
    rows = [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]
    return rows, scores, nf


@pytest.mark.parametrize("vocab", ["vocab_32000", "vocab_65536", "long24", "long40"])
def test_against_the_checker(vocab):
    native = _native(vocab)
    want = _checked(vocab)
    texts = _corpus()
    for k in KS:
        rows, scores, nf = _nbest(native, texts, k)
        assert "nbest_kernel" in native.last_kernel_times()
        for i, (wr, ws) in enumerate(want):
            assert nf[i] == min(k, len(wr)), (vocab, k, i)
            for r in range(k):
                if r < nf[i]:
                    assert rows[i * k + r] == wr[r], (vocab, k, i, r)
                    assert scores[i * k + r] == ws[r], (vocab, k, i, r)
                else:
                    assert rows[i * k + r] == [] and scores[i * k + r] == -math.inf
        # exact counts: n_found < k exactly where the sample has fewer than k segmentations
        assert [bool(nf[i] < k) for i in range(len(texts))] == [len(w[0]) < k for w in want]


def test_against_encode_and_row_properties():
    toks, scores = _vocab("vocab_32000")
    native = _native("vocab_32000")
    flat, offs = synth.make_corpus(64 << 20, "mixed")
    enc = native.encode_batch_flat(flat, offs)
    eids, eoo = enc.ids(), enc.offsets()
    enc.free()
    res, s1, nf1 = native.encode_batch_nbest_flat(flat, offs, 1)
    assert np.array_equal(res.ids(), eids) and np.array_equal(res.offsets(), eoo)
    res.free()
    assert (nf1 == 1).all()
    texts = _corpus()[:200]
    erows = [r for r in _nbest(native, texts, 1)[0]]
    vflat, voffs = tgx.pack(toks)
    for k in (2, 5, 16):
        rows, sc_, nf = _nbest(native, texts, k)
        for i, t in enumerate(texts):
            assert rows[i * k] == erows[i]
            got = rows[i * k:i * k + int(nf[i])]
            assert len({tuple(r) for r in got}) == len(got)
            for r, row in enumerate(got):
                assert b"".join(toks[x] for x in row) == t
                assert nc.path_score(row, scores) == sc_[i * k + r]
            assert all(a >= b for a, b in zip(sc_[i * k:i * k + int(nf[i])], sc_[i * k + 1:i * k + int(nf[i])]))


def test_batch_corpus_and_chunked_paths_agree(monkeypatch):
    native = _native("long40")
    texts = _corpus()
    flat, offs = tgx.pack(texts)
    for k in (3, 16):
        a, sa, na = native.encode_batch_nbest_flat(flat, offs, k)
        corpus = tgx.NativeCorpus(flat, offs)
        b, sb, nb = native.encode_corpus_nbest(corpus, k)
        monkeypatch.setenv("TGX_NBEST_CHUNK_MB", "1")  # ~8 KiB of text per chunk at k = 16; the 70 000-byte sample alone
        c, scc, ncc = native.encode_batch_nbest_flat(flat, offs, k)
        monkeypatch.delenv("TGX_NBEST_CHUNK_MB")
        ia, oa = a.ids(), a.offsets()
        for r in (b, c):
            assert np.array_equal(r.ids(), ia) and np.array_equal(r.offsets(), oa)
        for s_ in (sb, scc):
            assert np.array_equal(s_, sa)
        for n_ in (nb, ncc):
            assert np.array_equal(n_, na)


def test_errors_and_empty_samples():
    toks = [b"a", b"b", b"ab"]
    native = tgx.NativeModel(toks, [-1.0, -1.0, -1.5])
    flat, offs = tgx.pack([b"abab", b"ab", b"abx", b"xa", b"b"])
    with pytest.raises(tgx.TokenGeeXError) as enc:
        native.encode_batch_flat(flat, offs)
    for k in (1, 4, 16):
        with pytest.raises(tgx.TokenGeeXError) as nb:
            native.encode_batch_nbest_flat(flat, offs, k)
        assert nb.value.status == enc.value.status == _lib.ERR_NO_PATH
        assert str(nb.value) == str(enc.value)
        assert (nb.value.sample, nb.value.pos, nb.value.length) == (enc.value.sample, enc.value.pos, enc.value.length)
    for bad in (0, 17):
        with pytest.raises(tgx.TokenGeeXError) as e:
            native.encode_batch_nbest_flat(flat, offs, bad)
        assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(tgx.TokenGeeXError) as e:
        tgx.NativeModel(toks, [-1.0, -np.inf, -1.5]).encode_batch_nbest_flat(*tgx.pack([b"ab"]), 2)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    rows, scores, nf = _nbest(native, [b"", b"ab", b""], 4)
    assert list(nf) == [1, 2, 1]
    assert rows == [[], [], [], [], [2], [0, 1], [], [], [], [], [], []]
    assert list(scores) == [0.0] + [-math.inf] * 3 + [-1.5, -2.0] + [-math.inf] * 2 + [0.0] + [-math.inf] * 3
    res, s0, n0 = native.encode_batch_nbest_flat(np.zeros(0, np.uint8), np.zeros(1, np.uint64), 3)
    assert res.num_samples == 0 and res.num_tokens == 0 and s0.size == 0 and n0.size == 0


def test_tokenizer_with_specials_and_crlf():
    toks, scores = _vocab("vocab_32000")
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], processors=[tgx.CrlfProcessor()],
                       special_tokens=["<|eos|>"])
    eos = tk.special_token_to_id("<|eos|>")
    om = orc.OracleModel(toks, scores)
    texts = ["hello world<|eos|>def f(x):\r\n return x", "<|eos|>", "plain text only", "", "a<|eos|><|eos|>b\r\nc",
             "x = 1\r\n"]
    for k in (1, 4, 16):
        ids, oo, scs, nf = tk.encode_batch_nbest_flat(*tgx.pack([t.encode() for t in texts]), k)
        for i, t in enumerate(texts):
            parts = []
            for sub, special in tgx.tokenizer.split_special_tokens(t, ["<|eos|>"]):
                if special:
                    parts.append(([[eos]], [0.0]))
                else:
                    b = sub.replace("\r\n", "\n").encode()
                    parts.append(nc.nbest(sc.incoming(om, b, max(map(len, toks))), scores, len(b), k))
            want_rows, want_scores = nc.combine_brute(parts, k)
            assert nf[i] == len(want_rows), (k, i)
            for r in range(k):
                row = ids[int(oo[i * k + r]):int(oo[i * k + r + 1])].tolist()
                if r < len(want_rows):
                    assert row == want_rows[r] and scs[i * k + r] == want_scores[r], (k, i, r)
                else:
                    assert row == [] and scs[i * k + r] == -math.inf
        lists = tk.encode_batch_nbest(texts, k)
        assert [len(x) for x in lists] == list(nf)
        assert lists[0][0] == tk.encode(texts[0], 0.0)
    assert tk.encode_nbest(texts[0], 4) == tk.encode_batch_nbest(texts, 4)[0]


def test_nbest_sampling_law_and_k1():
    toks, scores = _vocab("vocab_32000")
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)])
    text = "the quick brown fox"
    k, alpha = 8, 0.5
    lists = tk.encode_nbest(text, k)
    ids, oo, scs, nf = tk.encode_batch_nbest_flat(*tgx.pack([text.encode()]), k)
    n = int(nf[0])
    assert n >= 4
    w = np.exp(alpha * (scs[:n] - scs[0]))
    p = w / w.sum()
    N = 4000
    cnt = np.zeros(n)
    index = {tuple(r): j for j, r in enumerate(lists)}
    for seed in range(N // 200):
        rows = tk.encode_batch_nbest_sample([text] * 200, k, alpha, seed=seed)
        for r in rows:
            cnt[index[tuple(r)]] += 1
    chi2 = float(((cnt - N * p) ** 2 / (N * p)).sum())
    assert chi2 < 3 * (n - 1) + 30, (chi2, cnt, N * p)
    # k = 1 draws encode's path; a fixed seed repeats
    assert tk.encode_nbest_sample(text, 1, alpha, seed=3) == tk.encode(text, 0.0)
    assert tk.encode_batch_nbest_sample([text] * 5, k, alpha, seed=9) == tk.encode_batch_nbest_sample([text] * 5, k, alpha, seed=9)


def test_row1_matches_the_host_astar_alternative():
    toks, scores = _vocab("vocab_32000")
    native = _native("vocab_32000")
    _, alt_offs, alt_ids = native.prune_alternatives()
    om = orc.OracleModel(toks, scores)
    cand = []
    for t, tok in enumerate(toks):
        if len(tok) < 2:
            continue
        rows, scs = nc.nbest(sc.incoming(om, tok, max(map(len, toks))), scores, len(tok), 3)
        if rows[0] != [t] or len(scs) < 3 or not (scs[0] - scs[1] > 1e-9 and scs[1] - scs[2] > 1e-9):
            continue
        cand.append(t)
        if len(cand) >= 400:
            break
    assert len(cand) >= 50
    got, _, nf = _nbest(native, [toks[t] for t in cand], 2)
    for i, t in enumerate(cand):
        alt = alt_ids[int(alt_offs[t]):int(alt_offs[t + 1])].tolist()
        assert nf[i] == 2
        assert got[i * 2 + 1] == alt, (t, toks[t], got[i * 2 + 1], alt)
