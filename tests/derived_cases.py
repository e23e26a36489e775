"""Derived models: vocabularies, derivations, texts and expectations for the tests of tgx_model_create_derived on every
device pass (tests/test_derived_cases_cpu.py, tests/test_derived_gpu.py, tests/test_derive_native.py).

A derived model is a copy of its parent's tables in which the dropped tokens lose their terminal bit and the kept ones
get a new id and a new score; max_token_len falls to the longest kept token.  Such a table holds what no table of
build_flat_trie does: used slots below which no token ends (dead branches), also deeper than the model's own lm, leaves
that are not terminal, and an lm on the other side of a kernel boundary (16 / 32 bytes) from the table's shape.

A case is a parent vocabulary, one or more links (keep_ids ascending, the child's scores) applied in turn, and texts
drawn from the PARENT's multi-byte tokens, so that the dropped tokens' bytes occur in them.  Nothing here calls the
library's kernels: everything expected comes from OracleModel(child tokens, child scores) and the checkers
(sample_checker, nbest_checker, util.estep_truth, decode_checker, spans_checker).  The host-only pieces of the library
that two cases use to BUILD themselves (prune_m_step for m_step_real, FlatTrie.stats for big_parent) need no device.
Everything is built once per process (lru_cache) and never modified."""
from __future__ import annotations

import functools
import struct

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import synth

import hostile_cases as hc
import nbest_checker as nc
import sample_checker as sc
import util

NINF = float("-inf")
TRIE8_MAX_SLOTS = 1 << 21  # kTrie8MaxSlots (csrc/trie_build.h)
COUNT_SLICE = 256 << 10    # bytes of the mixed corpus added to the counting and E-step passes
NBEST_KS = (1, 4, 16)
STATS_ALPHAS = (1.0, 0.3)


# ---- vocabularies -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nested():
    """Every byte at -8 and, for 70 strings of 6..16 bytes over a..d, every prefix from a length of 2..6 up: each
    multi-byte token but the shortest and the longest of its chain has both a proper prefix and a proper extension in the
    vocabulary."""
    rng = np.random.default_rng(4242)
    multi = {}
    for _ in range(70):
        n = int(rng.integers(6, 17))
        s = bytes(rng.integers(97, 101, size=n, dtype=np.uint8))
        for k in range(int(rng.integers(2, 7)), n + 1):
            multi[s[:k]] = None
    multi = list(multi)
    toks = [bytes([c]) for c in range(256)] + multi
    scores = np.concatenate([np.full(256, -8.0), -1.0 - rng.random(len(multi))])
    assert max(map(len, toks)) == 16 and len(set(toks)) == len(toks)
    return toks, scores


def _ids(toks, pred):
    return np.array([i for i, t in enumerate(toks) if pred(t)], np.uint32)


def _new_scores(scores, keep, seed):
    """The kept tokens' scores moved down by up to 0.25 (an M-step moves every score)."""
    return np.asarray(scores, np.float64)[keep] - 0.25 * np.random.default_rng(seed).random(keep.size)


def keep_prefix_holes(toks):
    """Bytes, and the multi-byte tokens that are a proper prefix of no other token: every dropped token is a proper prefix
    of a kept one (interior non-terminals on live paths)."""
    multi = [t for t in toks if len(t) > 1]
    return _ids(toks, lambda t: len(t) == 1 or not any(o != t and o.startswith(t) for o in multi))


def keep_dead_subtrees(toks):
    """Bytes, and the multi-byte tokens without a multi-byte proper prefix in the vocabulary: every dropped token is a
    proper extension of a kept one (dead subtrees below terminals, leaves that are not terminal)."""
    multi = [t for t in toks if len(t) > 1]
    return _ids(toks, lambda t: len(t) == 1 or not any(o != t and t.startswith(o) for o in multi))


def keep_up_to(toks, target):
    return _ids(toks, lambda t: len(t) <= target)


# ---- the case table -----------------------------------------------------------------------------------------------------
LEN_CASES = {"len16_to_le8": (16, 8), "len32_to_16": (32, 16), "len33_to_32": (33, 32), "len64_to_16": (64, 16), "len64_to_4": (64, 4)}
STRUCTURAL = ("prefix_holes", "dead_subtrees") + tuple(LEN_CASES) + ("keep_all_same_scores", "keep_all_new_scores", "empty_token_parent",
                                                                    "chain3")
SMALL_CASES = STRUCTURAL + ("byte_dropped", "keep_one", "keep_none", "scores_past_300", "scores_minus_inf", "m_step_real")
CASES = SMALL_CASES + ("big_parent_40", "big_parent_60")
# every sample has a path, every score is finite: the cases of the sampling, n-best, statistics and E-step comparisons
FULL_COVER = STRUCTURAL + ("scores_past_300", "m_step_real")
# the E-step also where a byte or a score is gone but every text of the case keeps a path
ESTEP_CASES = FULL_COVER + ("byte_dropped", "scores_minus_inf")
# sampling and the lattice statistics need finite scores; the samples of byte_dropped that hold the byte are the test's to add
SAMPLING_CASES = FULL_COVER + ("byte_dropped",)


def _case(name, toks, scores, links, texts, **extra):
    scores = np.asarray(scores, np.float64)
    links = [(np.ascontiguousarray(k, np.uint32), np.ascontiguousarray(s, np.float64)) for k, s in links]
    n = len(toks)
    for keep, cs in links:
        assert keep.size == cs.size and (keep.size == 0 or (np.all(np.diff(keep.astype(np.int64)) > 0) and int(keep[-1]) < n))
        n = keep.size
    return dict(name=name, toks=list(toks), scores=scores, links=links, texts=list(texts), bad_texts=[], **extra)


def _m_step_real():
    """A 4 000-entry build_vocab vocabulary and what prune's M-step leaves of it after the oracle's E-step over 1 MiB: the
    production shape, the control."""
    from tokengeex_amd import _lib
    flat, offs, toks, scores = util.corpus_and_vocab(1 << 20, "mixed", 4000, 16, seed_offset=33, max_len=8192)
    missing = [bytes([b]) for b in range(256) if bytes([b]) not in set(toks)]  # (bytes the corpus lacks: kept by the M-step)
    toks = list(toks)[:4000 - len(missing)] + missing
    scores = np.concatenate([np.asarray(scores, np.float64)[:4000 - len(missing)], np.full(len(missing), -15.0)])
    assert len(toks) == 4000 and len(set(toks)) == 4000
    st, expected, _, _ = orc.OracleModel(toks, scores).estep_flat(flat, offs, 81920, 0.0, 1, threads=8)
    assert st == orc.OK
    idx, new = _lib.prune_m_step(expected, np.array([len(t) == 1 for t in toks], np.uint8))
    assert 256 < idx.size < len(toks) and np.all(np.diff(idx.astype(np.int64)) > 0)
    return _case("m_step_real", toks, scores, [(idx, new)], hc.edge_texts(toks, 71, alphabet=b"etaoin shr"))


def _big_parent(frac):
    """The committed 500 000-entry vocabulary and a child of `frac` of it (bytes kept).  above_trie8: whether the parent's
    table has more slots than 8-byte records address, read from the host-only build."""
    from tokengeex_amd import _lib
    toks, scores = hc.big_ids()
    n_slots = _lib.FlatTrie(toks, scores).stats()["n_slots"]
    rng = np.random.default_rng(500 + int(frac * 100))
    single = np.array([i for i, t in enumerate(toks) if len(t) <= 1], np.int64)
    rest = np.setdiff1d(np.arange(len(toks)), single)
    keep = np.sort(np.concatenate([single, rng.choice(rest, int(len(toks) * frac) - single.size, replace=False)])).astype(np.uint32)
    return _case(f"big_parent_{int(frac * 100)}", toks, scores, [(keep, _new_scores(scores, keep, 501))], hc.corpus_texts(40, 22),
                 n_slots=n_slots, above_trie8=n_slots > TRIE8_MAX_SLOTS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """-> name, toks, scores (the parent's), links [(keep_ids, child scores)], texts, bad_texts (samples without a path
    under the child, for the test to insert), and what the case is named for."""
    if name in ("prefix_holes", "dead_subtrees"):
        toks, scores = nested()
        keep = (keep_prefix_holes if name == "prefix_holes" else keep_dead_subtrees)(toks)
        return _case(name, toks, scores, [(keep, _new_scores(scores, keep, 1))], hc.edge_texts(toks, 41))
    if name in LEN_CASES:
        n, target = LEN_CASES[name]
        toks, scores = hc.len_edge(n)
        keep = keep_up_to(toks, target)
        return _case(name, toks, scores, [(keep, _new_scores(scores, keep, n + target))], hc.edge_texts(toks, 40 + n), target=target)
    if name == "byte_dropped":
        toks, scores = hc.bytes_heavy(-100.0)
        keep = _ids(toks, lambda t: t != b"\xff")
        c = _case(name, toks, scores, [(keep, scores[keep])], hc.edge_texts(toks, 11, plain=False))
        c["bad_texts"] = list(hc.NOPATH_BAD)
        return c
    if name == "keep_all_same_scores":
        toks, scores = nested()
        return _case(name, toks, scores, [(np.arange(len(toks)), scores)], hc.edge_texts(toks, 42))
    if name == "keep_all_new_scores":
        toks, scores = nested()
        new = np.concatenate([scores[:256], -1.0 - np.random.default_rng(9).random(len(toks) - 256)])
        return _case(name, toks, scores, [(np.arange(len(toks)), new)], hc.edge_texts(toks, 42))
    if name == "keep_one":
        toks, scores = nested()
        c = _case(name, toks, scores, [([ord("a")], [-2.0])], [b"", b"a", b"a" * 33, b"", b"a" * 512])
        c["bad_texts"] = [b"b", b"a" * 64 + b"b", b"ba"]
        return c
    if name == "keep_none":
        toks, scores = nested()
        c = _case(name, toks, scores, [([], [])], [b"", b""])
        c["bad_texts"] = [b"a", b"abcd" * 16]
        return c
    if name == "scores_past_300":
        toks, scores = hc.len_edge(16)
        keep = keep_up_to(toks, 12)
        new = _new_scores(scores, keep, 300)
        new[ord("b")] = -301.0
        return _case(name, toks, scores, [(keep, new)], hc.edge_texts(toks, 56))
    if name == "scores_minus_inf":
        toks, scores = hc.len_edge(16)
        keep = keep_up_to(toks, 12)
        new = _new_scores(scores, keep, 301)
        new[int(np.nonzero(keep >= 256)[0][3])] = NINF  # a multi-byte token: every sample keeps a path
        return _case(name, toks, scores, [(keep, new)], hc.edge_texts(toks, 57))
    if name == "empty_token_parent":
        base, bs = nested()
        toks = base[:300] + [b""] + base[300:]
        scores = np.concatenate([bs[:300], [-2.0], bs[300:]])
        assert toks[300] == b""
        i = np.arange(len(toks))
        keep1 = i[(i < 256) | (i == 300) | (i % 5 != 4)]                     # the empty token is kept ...
        keep2 = np.arange(keep1.size)[keep1 != 300]                          # ... and then dropped
        return _case(name, toks, scores, [(keep1, _new_scores(scores, keep1, 5)), (keep2, _new_scores(scores[keep1], keep2, 6))],
                     hc.edge_texts(toks, 43))
    if name == "chain3":
        toks, scores = hc.len_edge(33)
        k1 = keep_up_to(toks, 32)                                            # lm 36 -> 32
        t1, s1 = [toks[i] for i in k1], _new_scores(scores, k1, 31)
        k2 = keep_prefix_holes(t1)
        t2, s2 = [t1[i] for i in k2], _new_scores(s1, k2, 32)
        k3 = keep_up_to(t2, 16)                                              # lm 32 -> 16
        return _case(name, toks, scores, [(k1, s1), (k2, s2), (k3, _new_scores(s2, k3, 33))], hc.edge_texts(toks, 44))
    if name == "m_step_real":
        return _m_step_real()
    if name.startswith("big_parent_"):
        return _big_parent(int(name[11:]) / 100.0)
    raise KeyError(name)


def child(c: dict, depth: int | None = None):
    """-> (tokens, scores) of the vocabulary after the first `depth` links (all of them by default)."""
    toks, scores = c["toks"], c["scores"]
    for keep, cs in c["links"][:depth]:
        toks, scores = [toks[int(i)] for i in keep], cs
    return toks, scores


def dropped(c: dict):
    """The parent's tokens that the last child no longer has."""
    have = set(child(c)[0])
    return [t for t in c["toks"] if t not in have]


def child_lm(c: dict) -> int:
    """The lm of the child model (tgx_api.cpp: finish_model_create)."""
    return max(4, (max([len(t) for t in child(c)[0]] or [0]) + 3) & ~3)


@functools.lru_cache(maxsize=None)
def oracle(name: str, depth: int | None = None) -> orc.OracleModel:
    return orc.OracleModel(*child(case(name), depth))


@functools.lru_cache(maxsize=None)
def parent_oracle(name: str) -> orc.OracleModel:
    c = case(name)
    return orc.OracleModel(c["toks"], c["scores"])


def has_path(name: str, text: bytes) -> bool:
    try:
        oracle(name).encode(text)
        return True
    except orc.NoPath:
        return False


def with_bad_texts(c: dict):
    """The case's texts with its samples without a path inserted, the shortest at the lowest index (as
    test_no_path_after_a_fallback does) -> (texts, indices of the bad ones)."""
    texts, bad = list(c["texts"]), sorted(c["bad_texts"], key=len)
    at = [2 + 4 * k for k in range(len(bad))]
    for i, b in zip(at, bad):
        texts.insert(min(i, len(texts)), b)
    idx = [i for i, t in enumerate(texts) if any(t is b for b in bad)]
    assert len(idx) == len(bad)
    return texts, idx


@functools.lru_cache(maxsize=None)
def count_corpus(name: str):
    """-> (flat, offs) of the counting and E-step passes: the texts and, where every byte has a token, a slice of the mixed
    corpus."""
    c = case(name)
    texts = list(c["texts"])
    if name in FULL_COVER and not name.startswith("big_parent"):
        flat, offs = synth.make_corpus(COUNT_SLICE, "mixed", min_len=16, max_len=4096, seed_offset=77)
        texts += [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    assert sum(map(len, texts)) <= COUNT_SLICE + 8192
    return orc.pack(texts)


# ---- expectations -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampling(name: str, alpha: float = 1.0) -> dict:
    """hostile_cases.sampling_case for the child vocabulary: the first seed of 1..64 at which every gap holds (a case
    without one is a failure of the case), check_sample per text, the 80-bit log Z, the range margins, and the kernel a
    plain call runs ('rows' for lm <= 32 and |alpha * score| <= 207, else 'generic')."""
    c = case(name)
    toks, scores = child(c)
    om, ml = oracle(name), max(map(len, toks))
    texts = c["texts"]
    inc = [sc.incoming(om, t, ml) for t in texts]
    lens = [len(t) for t in texts]
    margins = [hc.rows_range_margin(i, scores, n, alpha) for i, n in zip(inc, lens)]
    for seed in range(1, 65):
        checked = [sc.check_sample(i, scores, n, alpha, seed, s) for s, (i, n) in enumerate(zip(inc, lens))]
        if hc.gaps_hold(checked, lens):
            break
    else:
        raise AssertionError(f"{name}: no seed in 1..64 keeps every gap")
    ot = orc.OracleModel(toks, alpha * scores)
    truth = [ot.marginal_ext(t)[1] for t in texts]
    expect = "rows" if child_lm(c) <= 32 and float(np.abs(alpha * scores).max()) <= 207.0 else "generic"
    return dict(name=name, toks=toks, scores=scores, alpha=alpha, texts=texts, expect=expect, inc=inc, margins=margins, seed=seed,
                checked=checked, truth=truth)


@functools.lru_cache(maxsize=None)
def nbest(name: str):
    """nbest_checker.nbest at k = 16 per text (the rows of a smaller k are its first k)."""
    c = case(name)
    toks, scores = child(c)
    om, ml = oracle(name), max(map(len, toks))
    return [nc.nbest(sc.incoming(om, t, ml), scores, len(t), 16) for t in c["texts"]]


@functools.lru_cache(maxsize=None)
def stats_truth(name: str, alpha: float):
    """-> (logz, escore, etokens, n) per text from the 80-bit marginals of the child with scores alpha * scores (the reference
    of tests/stats_cases.py and test_stats_gpu._truth_of)."""
    c = case(name)
    toks, scores = child(c)
    om = orc.OracleModel(toks, alpha * scores)
    out = [om.marginal_ext(t) for t in c["texts"]]
    return (np.array([z for _, z in out]), np.array([float(np.dot(e, scores)) for e, _ in out]), np.array([float(e.sum()) for e, _ in out]),
            np.array([len(t) for t in c["texts"]], np.float64))


@functools.lru_cache(maxsize=None)
def stats_expect(name: str, alpha: float) -> str:
    """What a plain lattice_stats call runs: 'generic' (lm > 32 or some |alpha * score| > 207), else by the rows kernel's
    range rule over the texts 'rows' (every margin <= STAY_BITS) or 'fallback' (one >= TRIP_BITS: the rows kernel, then
    all of the call again on the generic one).  A case in between is a failure of the case."""
    c = case(name)
    toks, scores = child(c)
    if child_lm(c) > 32 or float(np.abs(alpha * scores).max()) > 207.0:
        return "generic"
    om, ml = oracle(name), max(map(len, toks))
    worst = max(hc.rows_range_margin(sc.incoming(om, t, ml), scores, len(t), alpha) for t in c["texts"])
    assert worst <= hc.STAY_BITS or worst >= hc.TRIP_BITS, (name, alpha, worst)
    return "rows" if worst <= hc.STAY_BITS else "fallback"


def estep_kernels(name: str):
    """-> (family, a kernel that must have run) of the child's E-step: estep7_kernel for tokens of at most 16 bytes with
    scores within +-300, the chained linear kernels for 17..32 bytes, the log-domain kernels otherwise."""
    c = case(name)
    _, scores = child(c)
    lm = child_lm(c)
    if not np.all(np.isfinite(scores)):
        return "log", "estep_kernel"
    if float(np.abs(scores).max()) > 300.0:
        return "log", "estep4_fwd_kernel" if lm <= 16 else "estep_kernel"
    if lm <= 16:
        return "linear", "estep7_kernel"
    return ("linear", "estep4l_fwd_kernel") if lm <= 32 else ("log", "estep_kernel")


# ---- the fixture of tests/native/derive_main.cpp --------------------------------------------------------------------------
def write_fixture(path, names=STRUCTURAL):
    """Little-endian: u64 n_cases; per case u64 name length, name; u64 V, u64 offs[V + 1], bytes, f64 scores[V]; u64 n_links;
    per link u64 n_keep, u32 keep[n_keep], f64 scores[n_keep]; u64 n_texts, u64 offs[n_texts + 1], bytes."""
    with open(path, "wb") as f:
        def packed(items):
            flat, offs = orc.pack(items)
            f.write(struct.pack("<Q", len(items)))
            f.write(offs.astype("<u8").tobytes())
            f.write(flat.tobytes())

        f.write(struct.pack("<Q", len(names)))
        for name in names:
            c = case(name)
            f.write(struct.pack("<Q", len(name)) + name.encode())
            packed(c["toks"])
            f.write(c["scores"].astype("<f8").tobytes())
            f.write(struct.pack("<Q", len(c["links"])))
            for keep, cs in c["links"]:
                f.write(struct.pack("<Q", keep.size) + keep.astype("<u4").tobytes() + cs.astype("<f8").tobytes())
            packed(c["texts"])
