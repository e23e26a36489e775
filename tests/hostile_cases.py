"""Vocabularies, texts and cases for the tests of sampling and n-best away from the project's usual vocabularies
(tests/test_hostile_cpu.py, tests/test_sample_hostile_gpu.py, tests/test_nbest_hostile_gpu.py).  Nothing here calls the
library's kernels: matches come from the CPU oracle, expectations from tests/sample_checker.py and
tests/nbest_checker.py.  The cases are built once per process (lru_cache) and never modified."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import synth

import nbest_checker as nc
import sample_checker as sc
import util

EDGE_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 512)
PLAIN_LENGTHS = (33, 64, 129)
TRIP_BITS, STAY_BITS = 650.0, 550.0
LN2 = math.log(2.0)
NINF = float("-inf")


# ---- vocabularies: each -> (toks: list[bytes], scores: float64[V]) ----------------------------------------------------
_WORDS = (b"sampling", b"lattice", b"fallback", b"range")


def bytes_heavy(score: float, without: tuple = ()):
    """Every single byte (but those in `without`) at `score`, and every prefix of 2..8 bytes of four ASCII words around
    -3: a text of whole words, cut anywhere, is covered by the word tokens but for a byte here and there."""
    toks = [bytes([c]) for c in range(256) if c not in without]
    scores = [float(score)] * len(toks)
    multi = [w[:k] for w in _WORDS for k in range(2, len(w) + 1)]
    assert 2 == min(map(len, multi)) and max(map(len, multi)) == 8 and len(set(multi)) == len(multi)
    toks += multi
    scores += [-2.5 - 0.0625 * (i % 17) for i in range(len(multi))]
    return toks, np.array(scores, np.float64)


def len_edge(max_len: int):
    """Every byte at -8, about 200 tokens of max_len - 2 .. max_len bytes over a..d (the vocabulary of
    test_trace_ring_extremes) and two tokens of every shorter length from 2 up."""
    rng = np.random.default_rng(1000 + max_len)
    long_ = [bytes(rng.integers(97, 101, size=max_len - int(rng.integers(0, 3)), dtype=np.uint8)) for _ in range(200)]
    short = [bytes(rng.integers(97, 101, size=ln, dtype=np.uint8)) for ln in range(2, max_len - 2) for _ in range(2)]
    multi = list(dict.fromkeys(long_ + short))
    toks = [bytes([c]) for c in range(256)] + multi
    scores = np.concatenate([np.full(256, -8.0), -1.0 - rng.random(len(multi))])
    assert max(map(len, toks)) == max_len and any(len(t) == max_len - 1 for t in toks)
    return toks, scores


def all_ties(max_len: int):
    """b"a" * k at -3 k, k = 1 .. max_len: every segmentation of a...a has the same score, exactly."""
    toks = [b"a" * k for k in range(1, max_len + 1)]
    return toks, np.array([-3.0 * k for k in range(1, max_len + 1)], np.float64)


def collapsing():
    """Scores near -1e15 (ulp 0.125) next to scores near -1 on a 1/32 grid: fl(a + s) rounds distinct a to one value.
    With one token at +2.5, one at 0.0 and b"ab" twice: the later id is the token."""
    toks = [b"a", b"b", b"c", b"d", b"ab", b"ba", b"aa", b"bc", b"cd", b"abc", b"ca", b"ad", b"dab", b"bcd", b"dd", b"ab"]
    scores = [-1.0, -1.03125, -1e15, -0.96875, -1.0625, 2.5, 0.0, -1e15 - 0.25, -1e15 - 0.125, -2e15, -1e15 + 0.125,
              -1.09375, -3.15625, -3e15, -1.90625, -0.5]
    assert len(toks) == len(scores) and toks.index(b"ab") == 4 and toks[-1] == b"ab"
    return toks, np.array(scores, np.float64)


def threshold(lowest: float):
    """Every byte at -2 but b"z" at `lowest`, the vocabulary's most negative score, and multi-byte tokens over a..d
    near -1: a text with a z must take that token."""
    rng = np.random.default_rng(207)
    multi = list(dict.fromkeys(bytes(rng.integers(97, 101, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(120)))
    toks = [bytes([c]) for c in range(256)] + multi
    scores = np.concatenate([np.full(256, -2.0), -1.0 - 0.5 * rng.random(len(multi))])
    scores[ord("z")] = lowest
    assert scores.min() == lowest
    return toks, scores


def tiny_poisoned():
    """The 8 tokens of test_distribution and b"x" at -100 (no segmentation of b"abcabca" holds it)."""
    toks = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"cab", b"x"]
    return toks, np.array([-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2, -100.0])


@functools.lru_cache(maxsize=None)
def big_ids():
    return util.load_vocab_500k()


@functools.lru_cache(maxsize=None)
def spec_32000():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return list(toks), np.asarray(scores, np.float64)


# ---- texts --------------------------------------------------------------------------------------------------------------
def edge_texts(toks, seed: int, alphabet: bytes = b"abcd", plain: bool = True):
    """One text per length of EDGE_LENGTHS: multi-byte tokens of the vocabulary drawn and concatenated, cut at the
    length (so the long tokens occur), and with `plain` three texts drawn byte by byte from `alphabet`."""
    rng = np.random.default_rng(seed)
    multi = [t for t in toks if len(t) > 1]
    out = []
    for n in EDGE_LENGTHS:
        parts, have = [], 0
        while have < n:
            parts.append(multi[int(rng.integers(0, len(multi)))])
            have += len(parts[-1])
        out.append(b"".join(parts)[:n])
    if plain:
        ab = np.frombuffer(alphabet, np.uint8)
        out += [bytes(ab[rng.integers(0, ab.size, size=n)]) for n in PLAIN_LENGTHS]
    assert max(map(len, out)) == 512
    return out


def corpus_texts(count: int, seed_offset: int, max_len: int = 512):
    flat, offs = synth.make_corpus(count * max_len, "mixed", min_len=16, max_len=max_len, seed_offset=seed_offset)
    texts = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)][:count]
    assert len(texts) == count and max(map(len, texts)) <= max_len
    return texts


# ---- the rows kernel's range rule -------------------------------------------------------------------------------------
def _logsumexp(xs):
    m = max(xs)
    return m + math.log(math.fsum(math.exp(x - m) for x in xs))


def forward(inc, scores, n: int, alpha: float):
    """A[0] = 0, A[p] = logsumexp over the matches (q, id) ending at p of A[q] + alpha * score; -inf: unreachable."""
    A = [NINF] * (n + 1)
    A[0] = 0.0
    for p in range(1, n + 1):
        c = [A[q] + alpha * float(scores[t]) for q, t in inc[p] if A[q] != NINF]
        if c:
            A[p] = _logsumexp(c)
    return A


def rows_range_margin(inc, scores, n: int, alpha: float) -> float:
    """The range rule in the comment above sample_rows_kernel, restated in the log domain.  The kernel keeps a row's
    values as a * 2^scale with one scale per block of 32 positions, set at the block's start so that the largest of the
    block's accumulators lies in [0.5, 1): the accumulator of position p holds, at that moment, the candidates of the
    matches that start before the block.  Block 0 starts with A[0] = 1 alone: scale 0.  A reachable position whose
    final value lies outside [2^-600, 2^600] of its block's scale raises the flag.
    -> the largest |log2 exp(A[p]) - scale(block of p)| over the reachable positions, in bits (a binary exponent is
    within one bit of the log2; the cases keep 50 bits away from the rule's 600)."""
    A = forward(inc, scores, n, alpha)
    worst = 0.0
    for p0 in range(0, n + 1, 32):
        block = range(p0, min(p0 + 32, n + 1))
        scale = 0
        if p0:
            partial = [[A[q] + alpha * float(scores[t]) for q, t in inc[p] if q < p0 and A[q] != NINF] for p in block]
            partial = [_logsumexp(c) for c in partial if c]
            if not partial:
                continue  # nothing in the block is reachable
            scale = math.floor(max(partial) / LN2) + 1
        for p in block:
            if A[p] != NINF:
                worst = max(worst, abs(A[p] / LN2 - scale))
    return worst


# ---- log Z bounds of tests/test_sample_gpu.py (_assert_logz_truth), restated --------------------------------------------
def logz_bound(kernel: str, n: int, truth: float) -> float:
    """sample_rows_kernel: 1e-13 max(1, |truth|).  sample_kernel: 64 sqrt(n) 2^-52 |truth| + 1e-13."""
    if kernel == "sample_rows_kernel":
        return 1e-13 * max(1.0, abs(truth))
    assert kernel == "sample_kernel", kernel
    return 64.0 * math.sqrt(max(n, 1)) * 2.0 ** -52 * abs(truth) + 1e-13


def log_rounding_model(n: int, logz: float) -> float:
    return 64.0 * math.sqrt(max(n, 1)) * 2.0 ** -52 * abs(logz)


# ---- sampling cases -----------------------------------------------------------------------------------------------------
POISON_DESIGNED = bytes(range(0x80, 0xA8))  # 40 bytes that only byte tokens cover
NOPATH_BAD = (b"\xff", b"sampling\xffrange")  # samples without a path under bytes_heavy(-100.0, without=(0xFF,))


def _designed_stay_texts():
    return edge_texts(bytes_heavy(-100.0)[0], 11, plain=False)


def _designed_texts():
    t = edge_texts(bytes_heavy(-100.0)[0], 11, alphabet=b"abcdefgh")
    return t[:5] + [POISON_DESIGNED] + t[5:]


REAL_ALPHA = 5.0


@functools.lru_cache(maxsize=None)
def _real_pool():
    """The first 60 samples of the mixed corpus that stay in range at alpha = 5: 16 .. 252 bytes, most of them short.  The
    forward value of ordinary text moves by up to ~200 bits per block of 32 bytes at alpha = 1, so at alpha = 5 most
    samples of more than a hundred bytes leave the range on their own (90 of the 200 drawn here, 44 more within 50 bits
    of the rule)."""
    toks, scores = spec_32000()
    om = orc.OracleModel(toks, scores)
    keep = []
    for t in corpus_texts(200, 21):
        if rows_range_margin(sc.incoming(om, t, max(map(len, toks))), scores, len(t), REAL_ALPHA) <= STAY_BITS:
            keep.append(t)
    assert len(keep) >= 60, len(keep)
    return keep[:60]


def _real_texts(poison: bool):
    texts = list(_real_pool())
    if poison:
        base = max(texts, key=len)[:200]
        texts = texts[:30] + [base[:100] + b"\x80" * 64 + base[100:]] + texts[30:]
    return texts


def _threshold_texts(toks):
    out = []
    for t in edge_texts(toks, 13):
        out.append(t[:len(t) // 2] + b"z" + t[len(t) // 2 + 1:] if len(t) >= 31 else t)
    return out


# name -> (vocabulary, alpha, texts, what a plain call runs: 'rows', 'generic', or 'fallback' = rows, then generic)
def _sampling_spec(name: str):
    if name == "designed_trip":
        return bytes_heavy(-100.0), 1.0, _designed_texts(), "fallback"
    if name == "designed_stay":
        return bytes_heavy(-100.0), 1.0, _designed_stay_texts(), "rows"
    if name == "designed_control":
        return bytes_heavy(-100.0), 0.01, _designed_texts(), "rows"
    if name == "real_trip":
        return spec_32000(), REAL_ALPHA, _real_texts(True), "fallback"
    if name == "real_stay":
        return spec_32000(), REAL_ALPHA, _real_texts(False), "rows"
    if name == "nopath_stay":  # the stay batch of a vocabulary without 0xFF (the failing samples are added by the test)
        return bytes_heavy(-100.0, without=(0xFF,)), 1.0, _designed_stay_texts(), "rows"
    if name == "len32":
        v = len_edge(32)
        return v, 1.0, edge_texts(v[0], 32), "rows"
    if name in ("len33", "len64"):
        v = len_edge(int(name[3:]))
        return v, 1.0, edge_texts(v[0], int(name[3:])), "generic"
    if name == "score207":
        v = threshold(-207.0)
        return v, 1.0, _threshold_texts(v[0]), "rows"
    if name == "score207_5":
        v = threshold(-207.5)
        return v, 1.0, _threshold_texts(v[0]), "generic"
    raise KeyError(name)


SAMPLING_CASES = ("designed_trip", "designed_stay", "designed_control", "real_trip", "real_stay", "nopath_stay", "len32",
                  "len33", "len64", "score207", "score207_5")


def gaps_hold(checked, lens) -> bool:
    """Every sample's smallest key gap on its path is at least 1e-6 and 100 times the log-domain rounding model."""
    return all(c["gap"] >= max(1e-6, 100.0 * log_rounding_model(n, c["logz"])) for c, n in zip(checked, lens))


@functools.lru_cache(maxsize=None)
def sampling_case(name: str) -> dict:
    """-> toks, scores, alpha, texts, expect ('rows' | 'generic' | 'fallback'), inc, margins (bits per sample), seed (the
    first of 1, 2, ... at which gaps_hold), checked (check_sample per sample at that seed), truth (80-bit log Z)."""
    (toks, scores), alpha, texts, expect = _sampling_spec(name)
    om = orc.OracleModel(toks, scores)
    ml = max(map(len, toks))
    inc = [sc.incoming(om, t, ml) for t in texts]
    lens = [len(t) for t in texts]
    margins = [rows_range_margin(i, scores, n, alpha) for i, n in zip(inc, lens)]
    for seed in range(1, 65):
        checked = [sc.check_sample(i, scores, n, alpha, seed, s) for s, (i, n) in enumerate(zip(inc, lens))]
        if gaps_hold(checked, lens):
            break
    else:
        raise AssertionError(f"{name}: no seed in 1..64 keeps every gap")
    ot = orc.OracleModel(toks, alpha * scores)
    truth = [ot.marginal_ext(t)[1] for t in texts]
    return dict(name=name, toks=toks, scores=scores, alpha=alpha, texts=texts, expect=expect, inc=inc, margins=margins,
                seed=seed, checked=checked, truth=truth)


# ---- the law after a fallback (tests/test_sample_gpu.py: test_distribution's rules) -----------------------------------
LAW_N, LAW_SEED, LAW_POISON = 20_000, 99, b"x" * 40


def assert_law(cnt: dict, probs: dict, N: int):
    """Counts per segmentation against its probability: no other segmentation, total variation below 0.02, and every
    segmentation of probability >= 0.01 within 5 sigma."""
    assert set(cnt) <= set(probs)
    tv = 0.5 * sum(abs(cnt.get(s, 0) / N - p) for s, p in probs.items())
    assert tv < 0.02, tv
    for s, p in probs.items():
        if p >= 0.01:
            assert abs(cnt.get(s, 0) / N - p) <= 5 * math.sqrt(p * (1 - p) / N), (s, p, cnt.get(s, 0) / N)


def path_tokens(ids, toks):
    """-> [(start, length)] of a row of ids."""
    out, p = [], 0
    for t in ids:
        out.append((p, len(toks[t])))
        p += len(toks[t])
    return out


# ---- n-best cases -------------------------------------------------------------------------------------------------------
def _nbest_spec(name: str):
    if name.startswith("ties"):
        v = all_ties(int(name[4:]))
        return v, [b"a" * n for n in EDGE_LENGTHS + (2, 3, 4, 5, 6)]
    if name == "len64":
        v = len_edge(64)
        return v, edge_texts(v[0], 64)
    if name == "collapsing":
        v = collapsing()
        return v, edge_texts(v[0], 15)
    if name == "big_ids":
        return big_ids(), corpus_texts(40, 22)
    raise KeyError(name)


NBEST_CASES = ("ties16", "ties33", "ties64", "len64", "collapsing", "big_ids")


@functools.lru_cache(maxsize=None)
def nbest_case(name: str) -> dict:
    """-> toks, scores, texts, want: nbest_checker.nbest at k = 16 per sample (the rows of a smaller k are its first k:
    tests/test_nbest_cpu.py)."""
    (toks, scores), texts = _nbest_spec(name)
    om = orc.OracleModel(toks, scores)
    ml = max(map(len, toks))
    want = [nc.nbest(sc.incoming(om, t, ml), scores, len(t), 16) for t in texts]
    return dict(name=name, toks=toks, scores=scores, texts=texts, want=want)
