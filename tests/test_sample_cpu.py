"""Sampling a segmentation from the lattice: the pinned draw, the entry points without a GPU, and the checker of
test_sample_gpu.py against brute-force enumeration."""
import math
import random

import numpy as np
import pytest

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib

import sample_checker as sc

M64 = (1 << 64) - 1


def test_sample_u01_matches_the_formula():
    rng = random.Random(7)
    for _ in range(2000):
        seed, sample, pos, ln = rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(40), rng.randrange(1, 65)
        got = _lib.sample_u01(seed, sample, pos, ln)
        assert got == sc.sample_u01(seed, sample, pos, ln)
        assert 0.0 < got < 1.0


def _unmix(y: int) -> int:
    """Inverse of the three xor-shift / multiply rounds."""
    def unxorshift(v, k):
        x = v
        for _ in range(64 // k + 1):
            x = v ^ (x >> k)
        return x & M64
    y = unxorshift(y, 31)
    y = (y * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    y = unxorshift(y, 27)
    y = (y * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    return unxorshift(y, 30)


@pytest.mark.parametrize("top", [0, (1 << 53) - 1, (1 << 53) - 2, 1 << 52])
def test_sample_u01_extremes_stay_inside(top):
    # a seed that makes x >> 11 == top for (sample, pos, len) = (3, 5, 2)
    x0 = _unmix((top << 11) | 0x5A5)
    seed = x0 ^ 0xD6E8FEB86659FD93 ^ ((3 * 0x9E3779B97F4A7C15) & M64) ^ ((5 * 0xC2B2AE3D27D4EB4F) & M64) \
        ^ ((2 * 0x165667B19E3779F9) & M64)
    u = _lib.sample_u01(seed, 3, 5, 2)
    assert u == sc.sample_u01(seed, 3, 5, 2)
    assert 0.0 < u < 1.0
    if top == 0:
        assert u == 2.0 ** -54


def test_sampling_entry_points_need_a_device():
    if tgx.device_count() > 0:
        pytest.skip("GPU present")
    flat, offs = tgx.pack([b"ab"])
    h = _lib.C.c_void_p()
    st = _lib.lib.tgx_encode_batch_sample(None, _lib.ptr(flat), _lib.ptr(offs), 1, 0.5, 1, None, _lib.C.byref(h))
    assert st == _lib.ERR_DEVICE
    st = _lib.lib.tgx_encode_corpus_sample(None, None, 0.5, 1, None, _lib.C.byref(h))
    assert st == _lib.ERR_DEVICE
    tk = tgx.Tokenizer([(b"a", -1.0, False), (b"b", -1.0, False)])
    with pytest.raises(tgx.TokenGeeXError):
        tk.encode_sample("ab", 0.5, seed=1)


def _tiny_model():
    toks = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"cab"]
    scores = [-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2]
    return toks, np.array(scores), orc.OracleModel(toks, scores)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0, 3.0])
def test_checker_against_enumeration(alpha):
    toks, scores, om = _tiny_model()
    text = b"abcab"
    inc = sc.incoming(om, text, 3)
    probs, logz = sc.segmentation_probs(inc, scores, len(text), alpha)
    r = sc.check_sample(inc, scores, len(text), alpha, 0, 0)
    assert abs(r["logz"] - logz) <= 1e-12 * max(1.0, abs(logz))
    assert tuple(r["ids"]) in probs
    # the draw's law: frequencies over many seeds approach the enumerated probabilities
    N = 20000
    cnt = {}
    for seed in range(N):
        ids = tuple(sc.check_sample(inc, scores, len(text), alpha, seed, 0)["ids"])
        cnt[ids] = cnt.get(ids, 0) + 1
    assert set(cnt) <= set(probs)
    tv = 0.5 * sum(abs(cnt.get(s, 0) / N - p) for s, p in probs.items())
    assert tv < 0.02, tv
    for s, p in probs.items():
        assert abs(cnt.get(s, 0) / N - p) <= 5 * math.sqrt(p * (1 - p) / N) + 1e-12


def test_checker_viterbi_limit():
    toks, scores, om = _tiny_model()
    text = b"abcabca"
    inc = sc.incoming(om, text, 3)
    r = sc.check_sample(inc, scores, len(text), 1e5, 11, 0, viterbi=True)
    assert r["ids"] == r["vids"] == om.encode(text)


def test_checker_no_path():
    toks, scores, om = _tiny_model()
    inc = sc.incoming(om, b"abd", 3)
    r = sc.check_sample(inc, scores, 3, 1.0, 0, 0)
    assert r["ids"] is None and r["logz"] == float("-inf")
