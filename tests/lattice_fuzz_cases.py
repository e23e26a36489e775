"""The randomised cases of the lattice passes (sampling, n-best, lattice statistics): one importable generator for
tests/test_lattice_fuzz_cpu.py, tests/test_lattice_fuzz_gpu.py and tests/measure/fuzz_lattice_gpu.py, which rebuild a case
from its (seed, case) pair.  tests/fuzz_cases.py is the generator of the encode ids and the E-step counts and stays as it
is; this one covers the passes written after it.

Nothing here calls the library's kernels.  Matches come from the CPU oracle's common prefix search, the expectations from
tests/sample_checker.py, tests/nbest_checker.py and the 80-bit truth; the kernels that a call must run follow the selection
rules of csrc/lattice_pass.cpp, restated in expected_kernels().

What make_case shapes, and why (nothing is excused afterwards: every sample that a case holds is held to every check):
  * a sample whose range margin (hostile_cases.rows_range_margin) lies between STAY_BITS and TRIP_BITS is not put into a
    case whose rows kernels could run: whether it raises the range flag is not known on the CPU to within a bit.
  * a poison sample is kept only where its margin is at least TRIP_BITS (alpha is raised to the largest value that the rows
    kernels still take, if that is what it needs); a case where no alpha does has no poison sample.
  * a derived model needs a parent without duplicate tokens (tgx_model_create_derived refuses one), so the families with
    duplicates are never derived.
  * the sample of 66 000 - 70 000 bytes comes with k <= 3, and the all_ties family with at most 1.5 KiB of text: the Python
    checker of n-best costs k x (matches per position) per byte.
  * collapsing holds scores near -1e15.  At alpha > 0 its texts avoid b"c" (every token with a c has such a score): a log Z of
    -1e15 has an ulp of 0.125, and no sampling seed keeps the key gaps 100 roundings apart.  At alpha = 0 they hold it.

The 80-bit truth.  OracleModel.marginal_ext follows the reference's lattice, which gives a position where no token ends the
forward value 1: it is the truth only for a sample in which a token ends at every position and one begins at every position
(`covered`).  For the other samples truth_ext below runs the same forward-backward sums in numpy's 80-bit long double over the
checker's matches, unreachable positions left out; tests/test_lattice_fuzz_cpu.py holds the two to each other where both
apply, and both to the sum over all segmentations on short texts."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import pack, synth

import hostile_cases as hc
import nbest_checker as nc
import sample_checker as sc
import stats_cases as sx
from fuzz_cases import base_text

# the kernel switches the fuzzer draws (all cleared before a case's own are set)
SWITCHES = ("TGX_SAMPLE_PATH", "TGX_STATS_PATH", "TGX_NBEST_CHUNK_MB")
MAX_LENS = (2, 3, 8, 15, 16, 17, 24, 31, 32, 33, 40, 64)
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)
ALPHAS = (0.0, 0.01, 0.1, 0.5, 1.0, 5.0)
EDGE_PRODUCTS = (206.9, 207.0, 207.6)  # max |alpha * score|: just below, at, just above the rows kernels' rule
KS = (1, 2, 3, 4, 5, 8, 16)
FAMILIES = ("random", "random_dup", "bytes_heavy", "len_edge", "all_ties", "collapsing", "threshold")
HOSTILE = FAMILIES[2:]
PASSES = ("sample", "nbest", "stats")
SEED0, N_CASES = 1, 160  # the list of tests/test_lattice_fuzz_cpu.py and tests/test_lattice_fuzz_gpu.py
BRUTE_MAX = 14       # a sample of at most this many bytes is also checked against the sum over all segmentations
TEXT_CAP = 48 << 10   # bytes of text per case apart from the sample above 64 KiB
NINF = float("-inf")
LD = np.longdouble

SAMPLE_RAN = {"rows": {"sample_wslot_kernel", "sample_rows_kernel", "trace32_kernel"},
              "fallback": {"sample_wslot_kernel", "sample_rows_kernel", "sample_kernel"},
              "generic": {"sample_kernel"}}
STATS_RAN = {"rows": {"sample_wslot_kernel", "stats_rows_kernel"}, "generic": {"stats_kernel"},
             "fallback": {"sample_wslot_kernel", "stats_rows_kernel", "stats_kernel"}, "none": set()}
NBEST_CHUNK_KERNELS = ("nbest_kernel", "nbest_trace_kernel", "scan_counts_kernel", "nbest_compact_kernel")


# ---- the selection rules of csrc/lattice_pass.cpp -----------------------------------------------------------------------
def linear_weights_fit(scores, alpha: float) -> bool:
    """Every |alpha * score| <= 207, in f64 as the library forms it."""
    return bool(np.all(np.abs(np.float64(alpha) * np.asarray(scores, np.float64)) <= 207.0))


def nbest_chunks(lens, k: int, budget_mb) -> int:
    """How many chunks nbest_corpus_locked cuts a call into (0 without samples)."""
    if not len(lens):
        return 0
    K = 1 if k <= 1 else 2 if k <= 2 else 4 if k <= 4 else 8 if k <= 8 else 16
    budget = (int(budget_mb) if budget_mb else 8192) << 20
    offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
    s0, chunks = 0, 1
    for s in range(len(lens)):
        nbytes, samples = offs[s + 1] - offs[s0], s + 1 - s0
        if s > s0 and (nbytes + samples) * K * 4 + nbytes * k * 4 > budget:
            chunks += 1
            s0 = s
    return chunks


def expected_kernels(max_len: int, scores, alpha: float, env: dict, trips: bool, n_samples: int) -> dict:
    """-> {'sample': 'rows' | 'fallback' | 'generic', 'stats': the same or 'none'}: what a call of each pass runs."""
    fit = max_len <= 32 and linear_weights_fit(scores, alpha)
    out = {}
    rows = fit and env.get("TGX_SAMPLE_PATH") != "generic"
    out["sample"] = ("fallback" if trips else "rows") if rows else "generic"
    rows = fit and env.get("TGX_STATS_PATH") != "generic"
    out["stats"] = "none" if n_samples == 0 else ("fallback" if trips else "rows") if rows else "generic"
    return out


# ---- the 80-bit truth ------------------------------------------------------------------------------------------------------
def covered(inc, n: int) -> bool:
    """A token ends at every position 1..n and one begins at every position 0..n-1: marginal_ext's lattice is the sample's."""
    begins = [False] * (n + 1)
    for p in range(1, n + 1):
        if not inc[p]:
            return False
        for q, _ in inc[p]:
            begins[q] = True
    return all(begins[:n])


def truth_ext(inc, scores, n: int, alpha: float):
    """-> (logz, escore, etokens) of one sample by forward-backward sums in 80-bit long double, every value kept as a
    mantissa in [0.5, 1) and a binary exponent of its own (as orc_marginal_ext keeps them); positions that no path reaches
    are left out.  (-inf, nan, nan) without a path."""
    if n == 0:
        return 0.0, 0.0, 0.0
    w = {}
    for p in range(1, n + 1):
        for _, t in inc[p]:
            if t not in w:
                w[t] = np.exp(LD(np.float64(alpha) * np.float64(scores[t])))
    fm, fe = [None] * (n + 1), [0] * (n + 1)
    fm[0], fe[0] = LD(1.0), 0

    def _sum(terms):
        emax = max(e for _, e in terms)
        s = LD(0.0)
        for m, e in terms:
            s += np.ldexp(m, e - emax)
        m, k = np.frexp(s)
        return m, emax + int(k)

    for p in range(1, n + 1):
        terms = [(fm[q] * w[t], fe[q]) for q, t in inc[p] if fm[q] is not None]
        if terms:
            fm[p], fe[p] = _sum(terms)
    if fm[n] is None:
        return NINF, math.nan, math.nan
    out = [[] for _ in range(n + 1)]
    for p in range(1, n + 1):
        for q, t in inc[p]:
            out[q].append((p, t))
    gm, ge = [None] * (n + 1), [0] * (n + 1)
    gm[n], ge[n] = LD(1.0), 0
    for q in range(n - 1, -1, -1):
        terms = [(gm[p] * w[t], ge[p]) for p, t in out[q] if gm[p] is not None]
        if terms:
            gm[q], ge[q] = _sum(terms)
    es, et = LD(0.0), LD(0.0)
    for p in range(1, n + 1):
        if gm[p] is None:
            continue
        for q, t in inc[p]:
            if fm[q] is None:
                continue
            post = np.ldexp(fm[q] * w[t] * gm[p] / fm[n], fe[q] + ge[p] - fe[n])
            et += post
            es += post * LD(np.float64(scores[t]))
    logz = np.log(fm[n]) + LD(fe[n]) * np.log(LD(2.0))
    return float(logz), float(es), float(et)


def truth(om_alpha, inc, scores, text: bytes, alpha: float):
    """The 80-bit truth of one sample as stats_cases.truth forms it (marginal_ext of the model with scores alpha * scores)
    where that lattice is the sample's, truth_ext otherwise."""
    n = len(text)
    if not covered(inc, n):
        return truth_ext(inc, scores, n, alpha)
    expected, lz = om_alpha.marginal_ext(text)
    return float(lz), float(np.dot(expected, scores)), float(expected.sum())


# ---- vocabularies and texts ---------------------------------------------------------------------------------------------------
def _from_tokens(rng, multi, n: int) -> bytes:
    """Tokens of `multi` drawn and joined, whole, up to n bytes (a few short of it where nothing fits)."""
    parts, have, misses = [], 0, 0
    while have < n and misses < 8:
        t = multi[int(rng.integers(0, len(multi)))]
        if have + len(t) <= n:
            parts.append(t)
            have += len(t)
        else:
            misses += 1
    return b"".join(parts)


def _draw_vocab(rng, family: str):
    """-> (toks, scores, info) with info: all_bytes (the vocabulary was built with every single byte), alphabet (bytes a
    text of the family is drawn from, or None), n_dup."""
    base = base_text()
    info = dict(all_bytes=True, alphabet=None, n_dup=0, param=None)
    if family in ("random", "random_dup"):
        max_len = int(rng.choice(MAX_LENS))
        info["all_bytes"] = bool(rng.random() < 0.65)
        toks, scores = synth.random_vocab(rng, base[: 64 << 10], n_multi=int(rng.integers(50, 1500)), max_len=max_len,
                                          all_bytes=info["all_bytes"], tie_fraction=float(rng.choice([0.0, 0.2, 0.6])))
        info["param"] = max_len
        if family == "random_dup":  # duplicates: the later id must win
            k = int(rng.integers(1, 21))
            idx = rng.integers(0, len(toks), k)
            toks = toks + [toks[i] for i in idx]
            scores = np.concatenate([scores, -rng.random(k) * 5])
            info["n_dup"] = k
        return toks, scores, info
    if family == "bytes_heavy":
        score = float(rng.choice([-100.0, -20.0, -8.0]))
        without = (0xFF,) if rng.random() < 0.4 else ()
        info.update(all_bytes=not without, param=(score, without))
        return (*hc.bytes_heavy(score, without), info)
    if family == "len_edge":
        max_len = int(rng.choice([16, 17, 32, 33, 64]))
        info.update(alphabet=b"abcd", param=max_len)
        return (*hc.len_edge(max_len), info)
    if family == "all_ties":
        max_len = int(rng.choice([16, 32, 33, 64]))
        info.update(all_bytes=False, alphabet=b"a", param=max_len)
        return (*hc.all_ties(max_len), info)
    if family == "collapsing":
        info.update(all_bytes=False, alphabet=b"abcd")
        return (*hc.collapsing(), info)
    assert family == "threshold", family
    lowest = float(rng.choice([-207.0, -207.5, -100.0]))
    info.update(alphabet=b"abcdz", param=lowest)
    return (*hc.threshold(lowest), info)


def _draw_parent(rng, toks, scores):
    """A parent of the case's vocabulary: 10 - 200 more tokens (substrings of the base text of up to one of MAX_LENS bytes,
    so a parent's longest token may lie across a kernel boundary from the child's) at random places among the case's, and
    other scores for the case's own.  -> dict(toks, scores, keep): parent.derive(keep, the case's scores) is the case's
    model."""
    base = base_text()
    have, extra = set(toks), []
    top = int(rng.choice(MAX_LENS))
    want = int(rng.integers(10, 201))
    for _ in range(50 * want):
        if len(extra) == want:
            break
        ln = int(rng.integers(2, top + 1))
        o = int(rng.integers(0, (64 << 10) - ln))
        t = base[o:o + ln]
        if t not in have:
            have.add(t)
            extra.append(t)
    is_extra = np.zeros(len(toks) + len(extra), bool)
    is_extra[rng.choice(is_extra.size, len(extra), replace=False)] = True
    keep = np.nonzero(~is_extra)[0].astype(np.uint32)
    ptoks, pscores = [None] * is_extra.size, np.empty(is_extra.size, np.float64)
    for i, at in enumerate(np.nonzero(is_extra)[0]):
        ptoks[at] = extra[i]
    for i, at in enumerate(keep):
        ptoks[at] = toks[i]
    pscores[is_extra] = -1.0 - 8.0 * rng.random(len(extra))
    pscores[keep] = -0.5 - 9.0 * rng.random(keep.size)
    assert len(set(ptoks)) == len(ptoks) and [ptoks[i] for i in keep] == list(toks)
    return dict(toks=ptoks, scores=pscores, keep=keep)


def _draw_text(rng, n: int, family: str, info: dict, multi, all_paths: bool) -> bytes:
    base = base_text()
    r = rng.random()
    ab = info["alphabet"]
    if family == "all_ties":
        return b"a" * n
    if family == "collapsing":
        letters = np.frombuffer(ab, np.uint8)
        return bytes(letters[rng.integers(0, letters.size, n)])
    if family in ("random", "random_dup") and not info["all_bytes"]:
        if all_paths or r < 0.75:
            return _from_tokens(rng, multi, n)
    elif r < 0.05:
        return bytes(rng.integers(0, 256, n).astype(np.uint8))
    if family in HOSTILE and r < 0.9:
        if r < 0.3 and family != "bytes_heavy":
            letters = np.frombuffer(ab, np.uint8)
            return bytes(letters[rng.integers(0, letters.size, n)])
        t = _from_tokens(rng, multi, n + 64)[:n]  # cut anywhere: every byte is a token
        if family == "threshold" and n >= 31 and r < 0.6:
            t = t[:n // 2] + b"z" + t[n // 2 + 1:]
        return t
    o = int(rng.integers(0, len(base) - n - 1))
    return base[o:o + n]


# ---- a case ----------------------------------------------------------------------------------------------------------------------
def make_case(seed0: int, case: int) -> dict:
    """Case `case` of a run with seed `seed0`: a vocabulary (family, max token length, byte cover, ties, duplicates; derived
    from a larger parent in a quarter of the cases), texts, alpha, k, the three switches (`env`), the form (batch or resident
    corpus) and the order of the three passes, the sampling seed; and what follows from them on the CPU: the matches (`inc`),
    the range margins, check_sample per sample at the seed, the kernels each pass must run (`expect`) and the number of
    n-best chunks."""
    rng = np.random.default_rng(seed0 * 100003 + case)
    family = str(rng.choice(FAMILIES, p=[0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1]))
    toks, scores, info = _draw_vocab(rng, family)
    scores = np.asarray(scores, np.float64)
    max_len = max(map(len, toks))
    multi = [t for t in toks if len(t) > 1] or list(toks)
    parent = None
    if rng.random() < 0.3 and len(set(toks)) == len(toks):
        parent = _draw_parent(rng, toks, scores)

    # alpha, k, the switches
    alpha = float(rng.choice(ALPHAS))
    if rng.random() < 0.25 and float(np.abs(scores).max()) > 0.0:
        alpha = float(rng.choice(EDGE_PRODUCTS)) / float(np.abs(scores).max())
    if family == "collapsing" and rng.random() < 0.5:
        alpha = 0.0
    if family == "collapsing" and alpha > 0.0:
        info["alphabet"] = b"abd"
    k = int(rng.choice(KS))
    env = {}
    if rng.random() < 0.35: env["TGX_SAMPLE_PATH"] = "generic"
    stats_path = str(rng.choice(["", "generic", "rows"], p=[0.35, 0.3, 0.35]))
    if rng.random() < 0.4: env["TGX_NBEST_CHUNK_MB"] = "1"
    aim_chunks = "TGX_NBEST_CHUNK_MB" in env and rng.random() < 0.4 and family != "all_ties"
    if aim_chunks:
        k = 16
    poison = bool(rng.random() < 0.2)
    big = bool(rng.random() < 1.0 / 16.0) and family != "all_ties"
    if big:
        k = min(k, int(rng.choice([1, 2, 3])))

    # texts
    r = rng.random()
    all_paths = bool(rng.random() < 0.5)  # a vocabulary without byte cover: only samples that have a path
    lens = []
    plain = r >= 0.16  # else S = 0, or empty samples alone: nothing is added to those
    if r < 0.08:
        pass
    elif r < 0.16:
        lens = [0] * int(rng.integers(1, 6))
    else:
        budget = 1536 if family == "all_ties" else int(rng.choice([1 << 10, 4 << 10, 12 << 10, TEXT_CAP - 4096], p=[0.35, 0.35, 0.25, 0.05]))
        count = int(rng.integers(1, 121))
        if aim_chunks:
            budget, count = int(rng.integers(9 << 10, 12 << 10)), 120
        brute = rng.random() < 0.35  # short samples, for the sum over all segmentations
        for _ in range(count):
            q = rng.random()
            if brute and q < 0.3: n = int(rng.integers(1, BRUTE_MAX + 1))
            elif q < (0.5 if aim_chunks else 0.8): n = int(rng.choice(LENGTHS))
            else: n = int(rng.integers(3, 3001))
            n = min(n, budget - sum(lens))
            lens.append(n)
            if sum(lens) >= budget:
                break
    texts = [_draw_text(rng, n, family, info, multi, all_paths) for n in lens]
    if family == "random_dup" and plain:  # a sample that holds the duplicated tokens
        texts.append(b"".join(toks[-info["n_dup"]:])[:2048])
    if not info["all_bytes"] and not all_paths and len(texts) > 1:  # samples without a path, none of them the first
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(1, len(texts)))
            t = texts[at]
            texts[at] = t[:len(t) // 2] + b"\xff" + t[len(t) // 2:]
    if big and plain:
        n = int(rng.integers(66_000, 70_001))
        if info["alphabet"]:
            letters = np.frombuffer(info["alphabet"], np.uint8)
            t = bytes(letters[rng.integers(0, letters.size, n)]) if family == "collapsing" else _from_tokens(rng, multi, n + 64)[:n]
        elif info["all_bytes"]:
            o = int(rng.integers(0, len(base_text()) - n - 1))
            t = base_text()[o:o + n]
        else:
            t = _from_tokens(rng, multi, n)
        texts.insert(int(rng.integers(0, len(texts) + 1)), t)

    # what the CPU knows of them
    om = orc.OracleModel(toks, scores)
    inc = [sc.incoming(om, t, max_len) for t in texts]
    fit = max_len <= 32 and linear_weights_fit(scores, alpha)
    poisoned = None
    if fit and poison and plain:
        single = [i for i, t in enumerate(toks) if len(t) == 1 and not any(t in m for m in multi if len(m) > 1)]
        if single:
            b = toks[min(single, key=lambda i: scores[i])]
            at = int(rng.integers(0, len(texts)))
            t = texts[at][:200]
            t = t[:len(t) // 2] + b * 40 + t[len(t) // 2:]
            ti = sc.incoming(om, t, max_len)
            if hc.rows_range_margin(ti, scores, len(t), alpha) < hc.TRIP_BITS:  # the largest alpha the rows kernels take
                top = 207.0 / float(np.abs(scores).max())
                while not linear_weights_fit(scores, top):
                    top = math.nextafter(top, 0.0)
                if hc.rows_range_margin(ti, scores, len(t), top) >= hc.TRIP_BITS:
                    alpha = top
            if hc.rows_range_margin(ti, scores, len(t), alpha) >= hc.TRIP_BITS:
                texts[at], inc[at], poisoned = t, ti, at
    fit = max_len <= 32 and linear_weights_fit(scores, alpha)
    margins = [hc.rows_range_margin(i, scores, len(t), alpha) if fit else 0.0 for i, t in zip(inc, texts)]
    keep = [j for j, m in enumerate(margins) if j == poisoned or not hc.STAY_BITS < m < hc.TRIP_BITS]
    if poisoned is not None:
        poisoned = keep.index(poisoned)
    texts, inc, margins = [texts[j] for j in keep], [inc[j] for j in keep], [margins[j] for j in keep]
    trips = any(m >= hc.TRIP_BITS for m in margins)
    if stats_path == "generic" or (stats_path == "rows" and fit and not trips):
        env["TGX_STATS_PATH"] = stats_path
    lens = [len(t) for t in texts]

    # the sampling seed: the first of seed .. seed + 7 at which every key gap holds (hostile_cases.gaps_hold)
    seed_base = int(rng.integers(0, 1 << 62))
    seed, checked = None, None
    for s in range(seed_base, seed_base + 8):
        checked = [sc.check_sample(i, scores, n, alpha, s, j) for j, (i, n) in enumerate(zip(inc, lens))]
        if hc.gaps_hold([c for c in checked if c["ids"] is not None], [n for c, n in zip(checked, lens) if c["ids"] is not None]):
            seed = s
            break
    no_path = [j for j, c in enumerate(checked) if c["logz"] == NINF]
    forms = {p: bool(rng.random() < 0.5) for p in PASSES}  # True: the resident-corpus form
    order = [PASSES[i] for i in rng.permutation(3)]
    flat, offs = pack(texts) if texts else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    return dict(seed0=seed0, case=case, family=family, info=info, toks=toks, scores=scores, max_len=max_len, parent=parent,
                alpha=alpha, k=k, env=env, texts=texts, lens=lens, flat=flat, offs=offs, inc=inc, margins=margins,
                poisoned=poisoned, trips=trips, seed_base=seed_base, seed=seed, checked=checked, no_path=no_path, forms=forms,
                order=order, expect=expected_kernels(max_len, scores, alpha, env, trips, len(texts)),
                chunks=nbest_chunks(lens, k, env.get("TGX_NBEST_CHUNK_MB")))


def references(c: dict) -> dict:
    """What the device is compared with: nbest_checker.nbest at the case's k per sample, and the 80-bit truth (z, es, et as
    arrays; -inf / nan for a sample without a path)."""
    toks, scores, alpha = c["toks"], c["scores"], c["alpha"]
    want = [nc.nbest(i, scores, n, c["k"]) for i, n in zip(c["inc"], c["lens"])]
    ot = orc.OracleModel(toks, alpha * scores)
    tr = [truth(ot, i, scores, t, alpha) for i, t in zip(c["inc"], c["texts"])]
    z, es, et = (np.array([t[j] for t in tr], np.float64) for j in range(3))
    return dict(nbest=want, z=z, es=es, et=et)


@functools.lru_cache(maxsize=None)
def case(seed0: int, i: int) -> dict:
    """make_case and references, built once per process and never modified."""
    c = make_case(seed0, i)
    c.update(references(c))
    return c


def tag(c: dict) -> str:
    """The drawn parameters of a case on one line."""
    e = c["env"]
    return (f"(seed0 {c['seed0']}, case {c['case']}) family={c['family']}:{c['info']['param']} V={len(c['toks'])} max_len={c['max_len']} "
            f"all_bytes={c['info']['all_bytes']} dup={c['info']['n_dup']} derived={c['parent'] is not None} S={len(c['texts'])} "
            f"N={int(sum(c['lens']))} longest={max(c['lens'], default=0)} alpha={c['alpha']!r} k={c['k']} seed={c['seed']} "
            f"env={e.get('TGX_SAMPLE_PATH')}/{e.get('TGX_STATS_PATH')}/{e.get('TGX_NBEST_CHUNK_MB')} "
            f"corpus_form={[p for p in PASSES if c['forms'][p]]} order={c['order']} expect={c['expect']} chunks={c['chunks']} "
            f"poisoned={c['poisoned']} no_path={c['no_path'][:4]}")


# ---- the bounds of section 2 -------------------------------------------------------------------------------------------------
def stats_bounds(rows: bool, n, z, es, et, alpha: float):
    """-> (bound on logz, on escore, on etokens, on entropy) per sample: stats_cases.logz_bound; ROWS_RTOL max(1, |truth|) on
    stats_rows_kernel, stats_cases.twin_bound on stats_kernel; entropy (bound on log Z) + alpha (bound on escore)."""
    zb = sx.logz_bound(rows, n, z)
    if rows:
        eb, tb = sx.ROWS_RTOL * np.maximum(1.0, np.abs(es)), sx.ROWS_RTOL * np.maximum(1.0, np.abs(et))
    else:
        eb, tb = sx.twin_bound(n, z, es), sx.twin_bound(n, z, et)
    return zb, eb, tb, zb + alpha * eb
