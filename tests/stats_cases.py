"""Texts, vocabularies, truths and bounds for the tests of the per-sample lattice statistics (tests/test_stats_cpu.py,
tests/test_stats_gpu.py).  Nothing here calls the library's kernels: the truth is the 80-bit oracle
(OracleModel.marginal_ext on alpha * scores) for vocabularies with full byte cover, and a brute-force sum over every
segmentation for texts of at most 12 bytes.  Everything is built once per process (lru_cache) and never modified."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import synth

LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 512, 8192)
ALPHAS = (0.0, 0.1, 1.0, 2.0)
NINF = float("-inf")

# The generic kernel's bound on escore and etokens, normalised by max(1, |truth|): 4 x the largest distance of the f64 host
# twin (the same recurrences) from the 80-bit truth over TWIN_RUNS on the shared texts, measured on the CPU
# (tests/test_stats_cpu.py::test_twin_distance_is_what_the_gpu_bound_was_made_from prints the figures).  The factor covers
# device exp / log1p differing from libm in the last bits.
TWIN_ESCORE_DIST = 4.9e-14   # measured 4.89e-14 (vocab_32000 at alpha 0, the 8192-byte sample)
TWIN_ETOKENS_DIST = 8.8e-15  # measured 8.78e-15 (the same run)
GENERIC_ESCORE_BOUND = 4.0 * TWIN_ESCORE_DIST
GENERIC_ETOKENS_BOUND = 4.0 * TWIN_ETOKENS_DIST
ROWS_RTOL = 1e-10  # util.assert_estep_truth's linear-domain gate, relative to max(1, |truth|)

# (vocabulary, alpha) of the runs the generic bound is measured over: every run the GPU tests put on stats_kernel
TWIN_RUNS = tuple(("vocab_32000", a) for a in ALPHAS) + (("long24", 1.0), ("long40", 1.0), ("long64", 1.0))


@functools.lru_cache(maxsize=None)
def texts():
    """One sample per length of LENGTHS, consecutive cuts of a mixed synthetic corpus: 15 samples in one batch (a second
    wave of the rows kernel, and a row that finds the queue empty)."""
    flat, _ = synth.make_corpus(64 << 10, "mixed", seed_offset=31)
    out, at = [], 0
    for n in LENGTHS:
        out.append(bytes(flat[at:at + n]))
        at += n
    assert [len(t) for t in out] == list(LENGTHS)
    return out


@functools.lru_cache(maxsize=None)
def vocab(name: str):
    """vocab_32000: the spec vocabulary.  long24: tokens of up to 17..32 bytes (tests/test_sample_gpu.py's).  long40 /
    long64: a 40- / 64-byte token that the 8192-byte sample holds on top of a short-token vocabulary."""
    if name == "vocab_32000":
        toks, scores, _ = synth.load_spec_vocab(32000)
        return list(toks), np.asarray(scores, np.float64)
    flat, _ = synth.make_corpus(1 << 20, "mixed", seed_offset=5)
    if name == "long24":
        toks, scores = synth.build_vocab(flat, 4000, 24)
        assert 17 <= max(map(len, toks)) <= 32
        return list(toks), np.asarray(scores, np.float64)
    n = {"long40": 40, "long64": 64}[name]
    toks, scores = synth.build_vocab(flat, 4000, 16)
    big = texts()[-1]
    toks, scores = list(toks) + [big[1000:1000 + n]], np.append(np.asarray(scores, np.float64), -3.0)
    assert max(map(len, toks)) == n
    return toks, scores


@functools.lru_cache(maxsize=None)
def truth(name: str, alpha: float):
    """-> (logz, escore, etokens) f64[len(texts())] from the 80-bit marginals of the model with scores alpha * scores:
    logz = z, etokens = sum of the expected counts, escore = expected counts . raw scores."""
    toks, scores = vocab(name)
    om = orc.OracleModel(toks, alpha * scores)
    z, es, et = [], [], []
    for t in texts():
        expected, lz = om.marginal_ext(t)
        z.append(lz)
        es.append(float(np.dot(expected, scores)))
        et.append(float(expected.sum()))
    return np.array(z), np.array(es), np.array(et)


def lens():
    return np.array([len(t) for t in texts()], np.float64)


def logz_bound(rows: bool, n, z):
    """tests/test_sample_gpu.py::_assert_logz_truth's bounds: rows 1e-13 max(1, |truth|); generic 64 sqrt(n) 2^-52 |truth|
    + 1e-13."""
    z = np.abs(np.asarray(z, np.float64))
    if rows:
        return 1e-13 * np.maximum(1.0, z)
    return 64.0 * np.sqrt(np.maximum(np.asarray(n, np.float64), 1.0)) * 2.0 ** -52 * z + 1e-13


def twin_bound(n, z, t):
    """What the f64 twin (log domain) may miss the truth of escore / etokens by.  Its weights are exp of a difference of two
    forward values, each within the log-domain rounding model 64 sqrt(n) 2^-52 |z| of its truth (logz_bound), so a weight
    has that relative error; a convex combination of terms no larger than the result's scale moves by at most that
    fraction of max(1, |truth|), and the roundings of the combination itself (a few ulp per position, random-walking) are
    far below it."""
    return (64.0 * np.sqrt(np.maximum(np.asarray(n, np.float64), 1.0)) * 2.0 ** -52 * np.maximum(1.0, np.abs(z)) + 1e-13) * np.maximum(1.0, np.abs(t))


def distance(got, want):
    """Largest |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0


# ---- brute force over every segmentation (texts of at most 12 bytes) -------------------------------------------------
def matches(toks, scores, text: bytes):
    """inc[p] = [(q, score)] of the matches ending at p; a later duplicate token overrides an earlier one."""
    table = {}
    for t, s in zip(toks, scores):
        if len(t):
            table[bytes(t)] = float(s)
    n = len(text)
    inc = [[] for _ in range(n + 1)]
    for q in range(n):
        for p in range(q + 1, n + 1):
            s = table.get(text[q:p])
            if s is not None:
                inc[p].append((q, s))
    return inc


def brute(toks, scores, text: bytes, alpha: float):
    """-> (logz, escore, etokens, entropy) by the sum over all segmentations; (-inf, nan, nan, nan) without one."""
    assert len(text) <= 12
    inc = matches(toks, scores, text)
    paths = {0: [(0.0, 0)]}  # (raw score sum, tokens)
    for p in range(1, len(text) + 1):
        paths[p] = [(sc + s, k + 1) for q, s in inc[p] for sc, k in paths.get(q, [])]
    segs = paths[len(text)]
    if not segs:
        return NINF, math.nan, math.nan, math.nan
    w = [alpha * sc for sc, _ in segs]
    m = max(w)
    z = math.fsum(math.exp(x - m) for x in w)
    pr = [math.exp(x - m) / z for x in w]
    logz = m + math.log(z)
    return (logz, math.fsum(p * sc for p, (sc, _) in zip(pr, segs)), math.fsum(p * k for p, (_, k) in zip(pr, segs)),
            -math.fsum(p * math.log(p) for p in pr if p > 0.0))


def tiny():
    toks = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"cab"]
    return toks, np.array([-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2])


# name -> (toks, scores, texts): the brute-force cases
def brute_cases():
    toks, scores = tiny()
    tied = ([b"a" * k for k in range(1, 7)], np.array([-3.0 * k for k in range(1, 7)]))
    dup = (toks + [b"ab"], np.append(scores, -0.25))  # the later b"ab" is the token
    partial = ([b"a", b"ab", b"bc", b"c", b"abc"], np.array([-1.0, -1.5, -0.5, -2.0, -2.5]))  # no b"b"
    positive = (toks, scores + np.array([0.0, 0.0, 0.0, 2.7, 0.0, 0.0, 1.9, 0.0]))
    return {
        "tiny": (toks, scores, [b"abcabca", b"", b"a", b"cabcab", b"abcabcabcabc"]),
        "tied": (tied[0], tied[1], [b"a" * 11, b"a", b""]),
        "duplicate": (dup[0], dup[1], [b"abcabca", b"ab", b"abab"]),
        "partial_cover": (partial[0], partial[1], [b"abc", b"abcabc", b"ab", b"aab", b"abcb", b"b", b"", b"cbc", b"aabc"]),
        "positive": (positive[0], positive[1], [b"abcabca", b"cabab"]),
    }
