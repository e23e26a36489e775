"""Shared helpers for the parity tests."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import synth


def corpus_and_vocab(n_bytes=1 << 20, kind="mixed", vocab_size=4000, max_token_length=16, seed_offset=0,
                     max_len=65536):
    flat, offs = synth.make_corpus(n_bytes, kind, max_len=max_len, seed_offset=seed_offset)
    toks, scores = synth.build_vocab(flat[: min(flat.size, 1 << 20)], vocab_size, max_token_length)
    return flat, offs, toks, scores


def assert_same_encoding(native_model, oracle_model, flat, offs, dropout=0.0, seed=0, threads=8):
    want_ids, want_offs = oracle_model.encode_batch_flat(flat, offs, dropout, seed, threads=threads)
    res = native_model.encode_batch_flat(flat, offs, dropout, seed)
    got_ids, got_offs = res.ids(), res.offsets()
    res.free()
    np.testing.assert_array_equal(got_offs, want_offs)
    np.testing.assert_array_equal(got_ids, want_ids)
    return got_ids, got_offs


def estep_longdouble(oracle_model, text: bytes):
    """Expected counts and log z of ONE snippet in 80-bit extended precision (64-bit mantissa), in the linear
    domain with per-position power-of-two exponents: alpha_true[p] = am[p] * 2**ae[p].  Independent of both
    the oracle's and the kernels' arithmetic; rounding ~1e-19 per operation, so it serves as the truth that
    two f64 evaluations are measured against (tests of the E-step tolerance)."""
    ld = np.longdouble
    n = len(text)
    V = oracle_model.vocab_size
    w = np.exp(np.asarray(oracle_model.scores, dtype=ld))
    matches = [oracle_model.common_prefix_search(text[p:p + 64]) for p in range(n)]  # [(id, len)] per start

    def sweep(edges_from):
        """edges_from(x) -> [(id, target)] for source x in sweep order; returns (mantissas, exponents)."""
        m = [ld(0)] * (n + 1)
        e = [0] * (n + 1)
        started = [False] * (n + 1)
        return m, e, started

    # forward
    am, ae, st = sweep(None)
    am[0], st[0] = ld(1), True
    for p in range(n):
        if not st[p]:
            raise ValueError("position without incoming token")
        mm, ee = np.frexp(am[p])
        am[p], ae[p] = mm, ae[p] + int(ee)
        for tid, ln in matches[p]:
            t = p + ln
            term = am[p] * w[tid]
            if not st[t]:
                am[t], ae[t], st[t] = term, ae[p], True
            else:
                am[t] = am[t] + np.ldexp(term, ae[p] - ae[t])
    mm, ee = np.frexp(am[n])
    am[n], ae[n] = mm, ae[n] + int(ee)
    logz = float(np.log(am[n]) + ld(ae[n]) * np.log(ld(2)))
    # backward
    bm = [ld(0)] * (n + 1)
    be = [0] * (n + 1)
    bs = [False] * (n + 1)
    bm[n], bs[n] = ld(1), True
    ends = [[] for _ in range(n + 1)]
    for p in range(n):
        for tid, ln in matches[p]:
            ends[p + ln].append((tid, p))
    expected = np.zeros(V, dtype=ld)
    for q in range(n, 0, -1):
        mm, ee = np.frexp(bm[q])
        bm[q], be[q] = mm, be[q] + int(ee)
        for tid, p in ends[q]:
            term = bm[q] * w[tid]
            expected[tid] += np.ldexp(am[p] * term / am[n], ae[p] + be[q] - ae[n])
            if not bs[p]:
                bm[p], be[p], bs[p] = term, be[q], True
            else:
                bm[p] = bm[p] + np.ldexp(term, be[q] - be[p])
    return expected.astype(np.float64), logz


def rtol_for(snippet_bytes):
    """Tolerance between the f64 oracle (or a log-domain kernel) and the truth: the reference's log-domain sums are
    only defined to ~sqrt(n) ulp(|z|) (tests/test_estep_pairs_gpu.py)."""
    return 1.2e-8 * max(1.0, snippet_bytes / 4096.0)


# kernels whose arithmetic is the linear domain (exact power-of-two rescales) and the log-domain ones
LINEAR_ESTEP = ("estep7_kernel", "estep7_redo_kernel", "estep4l_fwd_kernel", "estep4l_bwd_kernel", "estep5_fwd_kernel")
LOG_ESTEP = ("estep4_fwd_kernel", "estep4_bwd_kernel", "estep_kernel")
_TRUTH: dict = {}


def _digest(*arrays) -> str:
    import hashlib
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def estep_truth(oracle_model, flat, offs, snippet_len=81920, dropout=0.0, seed=0):
    """orc_estep_ext (80-bit extended precision) of one pass, cached per (model, corpus, snippet length, dropout, seed).
    -> (status, expected, logz_sum, err_sample)"""
    key = (_digest(oracle_model._flat, oracle_model._offs, oracle_model.scores), _digest(flat, offs),
           int(snippet_len), float(dropout), int(seed))
    if key not in _TRUTH:
        if len(_TRUTH) >= 24:
            _TRUTH.pop(next(iter(_TRUTH)))
        _TRUTH[key] = oracle_model.estep_ext_flat(flat, offs, snippet_len, dropout, seed, threads=8)
    return _TRUTH[key]


def estep_family(kernels) -> str:
    """'log' when any log-domain E-step kernel ran (a fallback included), else 'linear' (some linear kernel must have)."""
    if any(k in kernels for k in LOG_ESTEP):
        return "log"
    assert any(k in kernels for k in LINEAR_ESTEP), kernels
    return "linear"


def estep_gate(got, gz, kernels, truth, tz, longest):
    """The two-sided gate of tests/measure/fuzz_gpu.py: a pass of the kernels against the truth, with the bounds of
    assert_estep_truth.  -> (family, ok, largest relative distance on counts above 1e-9)"""
    fam = estep_family(kernels)
    big = truth > 1e-9
    dist = float((np.abs(got - truth)[big] / truth[big]).max()) if big.any() else 0.0
    if fam == "linear":
        ok = bool(np.allclose(got, truth, rtol=1e-10, atol=1e-13)) and abs(gz - tz) <= 1e-13 * abs(tz)
    else:
        ok = bool(np.allclose(got, truth, rtol=rtol_for(longest), atol=1e-12)) and abs(gz - tz) <= 1e-12 * abs(tz) + 1e-9
    return fam, ok, dist


def assert_estep_truth(got, gz, kernels, oracle_model, flat, offs, snippet_len=81920, dropout=0.0, seed=0,
                       want=None, wz=None):
    """The truth gate of every E-step comparison.  Linear-domain kernels: every count within rtol 1e-10, atol 1e-13 of
    the truth and log Z within 1e-13 relative.  Log-domain kernels: within rtol_for(longest snippet) — their error is
    the f64 oracle's kind.  The oracle's own result (want, wz), when given, must be within rtol_for of the truth: if that
    fails it is the f64 formula's rounding, not a kernel's."""
    st, truth, tz, _ = estep_truth(oracle_model, flat, offs, snippet_len, dropout, seed)
    assert st == orc.OK
    longest = int(np.diff(offs.astype(np.int64)).max()) if offs.size > 1 else 0
    rtol = rtol_for(min(snippet_len, longest))
    if want is not None:
        bad = ~np.isclose(want, truth, rtol=rtol, atol=1e-12)
        assert not bad.any(), ("the f64 ORACLE (not a kernel) misses the truth", np.nonzero(bad)[0][:5])
        assert abs(wz - tz) <= 1e-12 * abs(tz) + 1e-9, ("the f64 ORACLE's log Z (not a kernel's)", wz, tz)
    fam = estep_family(kernels)
    if fam == "linear":
        np.testing.assert_allclose(got, truth, rtol=1e-10, atol=1e-13, err_msg=f"linear-domain kernels {sorted(kernels)}")
        assert abs(gz - tz) <= 1e-13 * abs(tz), (gz, tz, sorted(kernels))
    else:
        np.testing.assert_allclose(got, truth, rtol=rtol, atol=1e-12, err_msg=f"log-domain kernels {sorted(kernels)}")
        assert abs(gz - tz) <= 1e-12 * abs(tz) + 1e-9, (gz, tz, sorted(kernels))
    return fam


def load_vocab_500k():
    """The 500 000-entry synthetic vocabulary of BASELINE.json configs[3] (prune's start): built once by
    tools/make_vocab_cache.py 500000 (synth.build_vocab over 64 MiB of the mixed corpus, minutes of numpy) and
    committed, compressed, as tests/golden/vocab_500000.npz (token bytes, lengths, distinct score values + index).
    -> (tokens: list[bytes], scores: float64[500000])"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_500000.npz"))
    fb = z["flat"].tobytes()
    o = np.concatenate([[0], np.cumsum(z["lens"].astype(np.int64))])
    toks = [fb[o[i]:o[i + 1]] for i in range(o.size - 1)]
    scores = z["uscores"][z["inv"]].astype(np.float64)
    assert len(toks) == 500000 and scores.size == 500000
    return toks, scores


class AllowByHand:
    """The allow pattern of the merge / generate tests (test_merge_cpu.ALLOW: any one character | [a-z]+ |
    [A-Z][a-z]+ | CJK run | one ASCII punctuation mark with optional single spaces around it) evaluated WITHOUT a
    regex engine, with the meaning Rust's `regex` gives it (`.` = any character but a newline, `$` = end of text,
    `[[:punct:]]` = ASCII punctuation): the checker's side of the comparison must not go through the product's
    pattern translation (tokengeex_amd.merge.compile_rust_regex)."""
    _PUNCT = set("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")

    def search(self, s: str):
        if len(s) == 1 and s != "\n":
            return True
        if s and all("a" <= c <= "z" for c in s):
            return True
        if len(s) >= 2 and "A" <= s[0] <= "Z" and all("a" <= c <= "z" for c in s[1:]):
            return True
        if s and all(0x3400 <= ord(c) <= 0x4DBF or 0x4E00 <= ord(c) <= 0x9FFF for c in s):
            return True
        core = s[1:] if s.startswith(" ") else s
        core = core[:-1] if core.endswith(" ") and len(core) > 1 else core
        return len(core) == 1 and core in self._PUNCT
