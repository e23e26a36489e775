"""GPU parity of the walk compaction of encode5_kernel (csrc/encode5.hip: Walk5): the live walks
of a trip are packed into fewer lanes at depth 4, 5 or 6 (TGX_E5_COMPACT) — ids bit-exact against the CPU oracle and
against the uncompacted kernel, on every build that compacts and every one that opts out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import synth

from util import assert_same_encoding, corpus_and_vocab

DEPTHS = ["off", "4", "5", "6"]


def _distinct_scores(scores, rng):
    return np.asarray(scores, np.float64) - rng.random(len(scores)) * 1e-3


def _deep_texts(rng, n):
    """Samples whose walks run deep (runs of spaces, of one letter, CJK, ASCII words) and shallow ones of the same
    length, so that the rows of a wave mix them: trips with 0 .. 192 walks alive at the compaction depth."""
    words = [b"function", b"return", b"international", b"    ", b"        ",
             "中文字符编码".encode(), "数据结构".encode()]
    out = []
    for i in range(n):
        kind = i % 5
        if kind == 0:
            t = b" " * 300
        elif kind == 1:
            t = b"a" * 300
        elif kind == 2:
            t = b"".join(words[j] for j in rng.integers(0, len(words), 60))[:300]
        elif kind == 3:
            t = bytes(rng.integers(0x21, 0x7F, 300, dtype=np.uint8))
        else:
            t = ("漢字" * 50).encode()[:300]
        out.append(t)
    out += [b"", b"a", b" " * 15, b" " * 16, b" " * 17, b"a" * 63, b"a" * 64, b"a" * 65]
    return out


def _vocab_with_runs(toks, scores):
    """Adds runs of 2..16 spaces and of 'a' so that every position of such a run walks 16 levels."""
    have = set(toks)
    extra = [c * k for c in (b" ", b"a") for k in range(2, 17) if c * k not in have]
    return list(toks) + extra, np.concatenate([np.asarray(scores, np.float64), -3.0 - 0.1 * np.arange(len(extra))])


@pytest.mark.parametrize("vocab", [32000, 65536])
def test_spec_vocabularies_at_every_depth(monkeypatch, vocab):
    """The committed spec vocabularies on the mixed corpus: every compaction depth and none give the oracle's ids."""
    toks, scores, _ = synth.load_spec_vocab(vocab)
    flat, offs = synth.make_corpus(3 << 20, "mixed", seed_offset=1000, max_len=30000)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    want, _ = assert_same_encoding(nat, ora, flat, offs)
    for k in DEPTHS:
        monkeypatch.setenv("TGX_E5_COMPACT", k)
        got, _ = assert_same_encoding(nat, ora, flat, offs)
        assert "encode5_kernel" in nat.last_kernel_times()
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("ppl", ["2", "3", "4"])
@pytest.mark.parametrize("cold", [False, True])
def test_positions_per_lane_hot_and_cold(monkeypatch, ppl, cold):
    """Two to four walks per lane (the builds that compact), every value in LDS or a small LDS copy with every token
    its own score (COLD builds), deep and shallow samples mixed, with dropout (those builds opt out)."""
    rng = np.random.default_rng(int(ppl) * 10 + cold)
    flat, offs, toks, scores = corpus_and_vocab(1 << 20, "mixed", 8000, 16, seed_offset=61, max_len=20000)
    toks, scores = _vocab_with_runs(toks, scores)
    if cold:
        scores = _distinct_scores(scores, rng)
        monkeypatch.setenv("TGX_E5_HOT", "500")
    monkeypatch.setenv("TGX_PPL", ppl)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    f2, o2 = tgx.pack(_deep_texts(rng, 1500))
    for k in DEPTHS:
        monkeypatch.setenv("TGX_E5_COMPACT", k)
        assert_same_encoding(nat, ora, flat, offs)
        assert_same_encoding(nat, ora, f2, o2)
        assert "encode5_kernel" in nat.last_kernel_times()
        if cold:
            assert nat.last_encode_hot_values() == 500
    assert_same_encoding(nat, ora, f2, o2, dropout=0.25, seed=7)


def test_every_walk_deep(monkeypatch):
    """Every position of every sample walks 16 levels (all 192 walks of a trip alive at the compaction depth: the
    trip goes on uncompacted), and samples shorter than the compaction depth."""
    toks = [bytes([c]) for c in range(256)] + [b"a" * k for k in range(2, 17)] + [b"ab", b"ba", b"abab"]
    rng = np.random.default_rng(43)
    scores = -(rng.random(len(toks)) * 6.0 + 1.0)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    texts = [b"a" * 5000, b"ab" * 700 + b"a" * 900, b"a" * 3, b"a" * 4, b"a" * 5, b"a" * 6, b"x" + b"a" * 300 + b"y", b""]
    texts += [b"a" * int(n) for n in rng.integers(1, 400, 300)]
    f, o = tgx.pack(texts)
    for k in DEPTHS:
        monkeypatch.setenv("TGX_E5_COMPACT", k)
        for ppl in ("2", "3", "4"):
            monkeypatch.setenv("TGX_PPL", ppl)
            assert_same_encoding(nat, ora, f, o)


def test_long_token_vocabulary_opts_out(monkeypatch):
    """Tokens of up to 24 bytes (the LONG build, which never compacts): the knob changes nothing."""
    rng = np.random.default_rng(4024)
    flat, offs = synth.make_corpus(384 << 10, "mixed", seed_offset=74, max_len=20000)
    toks, scores = synth.random_vocab(rng, bytes(flat[: 96 << 10]), n_multi=4000, max_len=24, tie_fraction=0.5)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    assert 16 < nat.max_token_len <= 24
    for k in DEPTHS:
        monkeypatch.setenv("TGX_E5_COMPACT", k)
        assert_same_encoding(nat, ora, flat, offs)
        assert "encode5_kernel" in nat.last_kernel_times()
