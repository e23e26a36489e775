"""The randomised cases of tests/measure/fuzz_gpu.py, one importable function: the fuzzer, tools/dev/fuzz_case.py and the
regression tests (tests/test_estep_pairs_gpu.py) rebuild a case from its (seed, case) pair.  This generator covers the
encode ids (all its entry points and kernels) and the E-step counts; sampling, n-best and the lattice statistics have a
generator of their own, tests/lattice_fuzz_cases.py."""
from __future__ import annotations

import functools

import numpy as np

from tokengeex_amd import pack, synth

# the kernel switches the fuzzer draws (all cleared before a case's own are set)
SWITCHES = ("TGX_PPL", "TGX_EPPL", "TGX_PATH", "TGX_LONG_THRESHOLD", "TGX_E5_HOT", "TGX_E6_POOL", "TGX_E2E_CHUNK_MB",
            "TGX_ESTEP_PIECES", "TGX_ESTEP_WINDOW", "TGX_CORUN", "TGX_TRACE_CARRY", "TGX_E7_HOT", "TGX_E7_WAVES",
            "TGX_E7_RANK", "TGX_E7_OVF_AT", "TGX_ESTEP", "TGX_VALUE_RANK")


@functools.lru_cache(maxsize=1)
def base_text() -> bytes:
    flat, _ = synth.make_corpus(2 << 20, "mixed", seed_offset=77)
    return bytes(flat)


def make_case(seed0: int, case: int) -> dict:
    """Case `case` of a fuzz run with seed `seed0`: a vocabulary shape (max token length 1..40, with or without full byte
    cover, duplicate and tied scores), a batch shape (empty and 1-byte samples, lengths around the 16/32/64 block
    boundaries, a few long ones), dropout, the kernel switches (`env`) and the E-step's snippet length, drawn in the
    fuzzer's order."""
    base = base_text()
    rng = np.random.default_rng(seed0 * 100003 + case)
    max_len = int(rng.choice([2, 3, 5, 8, 12, 15, 16, 17, 20, 24, 31, 32, 33, 40]))
    all_bytes = bool(rng.random() < 0.8)
    toks, scores = synth.random_vocab(rng, base[: 64 << 10], n_multi=int(rng.integers(50, 3000)), max_len=max_len,
                                      all_bytes=all_bytes, tie_fraction=float(rng.choice([0.0, 0.2, 0.6])))
    if rng.random() < 0.3:  # duplicates: the later id must win
        k = int(rng.integers(1, 20))
        idx = rng.integers(0, len(toks), k)
        toks = toks + [toks[i] for i in idx]
        scores = np.concatenate([scores, -rng.random(k) * 5])
    lens = []
    for _ in range(int(rng.integers(1, 400))):
        r = rng.random()
        if r < 0.1: lens.append(int(rng.choice([0, 1, 2])))
        elif r < 0.4: lens.append(int(rng.choice([15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129])))
        elif r < 0.97: lens.append(int(rng.integers(3, 3000)))
        else: lens.append(int(rng.integers(20000, 90000)))
    texts = []
    for n in lens:
        if rng.random() < 0.05:
            texts.append(bytes(rng.integers(0, 256, n).astype(np.uint8)))
        else:
            o = int(rng.integers(0, len(base) - n - 1))
            texts.append(base[o:o + n])
    flat, offs = pack(texts)
    dropout = float(rng.choice([0.0, 0.0, 0.1, 0.5, 1.0]))
    sd = int(rng.integers(0, 1 << 62))
    env = {}
    # round 4: the trace's two modes; estep7_kernel's table size, waves, rank order, overflow build;
    # the chained kernels now and then
    if rng.random() < 0.5: env["TGX_TRACE_CARRY"] = str(int(rng.choice([0, 1])))
    if rng.random() < 0.4: env["TGX_E7_HOT"] = str(int(rng.choice([0, 5, 60, 700])))
    if rng.random() < 0.3: env["TGX_E7_WAVES"] = str(int(rng.choice([1, 3, 8])))
    if rng.random() < 0.3: env["TGX_E7_RANK"] = "model"
    if rng.random() < 0.3: env["TGX_E7_OVF_AT"] = str(int(rng.choice([3, 50, 400, 2000])))
    if rng.random() < 0.15: env["TGX_ESTEP"] = "chain"
    if rng.random() < 0.5: env["TGX_VALUE_RANK"] = str(rng.choice(["counts", "model"]))  # encode5's values re-ranked by match counts
    if rng.random() < 0.6: env["TGX_PPL"] = str(int(rng.choice([1, 2, 4])))
    if rng.random() < 0.6: env["TGX_EPPL"] = str(int(rng.choice([1, 2, 4])))
    # round 2: kernel choice (encode5 / encode4), long-sample kernel threshold, score table size (cold values
    # through the pools), pool size (overflow -> redo pass)
    if rng.random() < 0.5: env["TGX_PATH"] = str(rng.choice(["rows4", "rows5"]))
    if rng.random() < 0.5: env["TGX_LONG_THRESHOLD"] = str(int(rng.choice([0, 1, 100, 1000, 30000])))
    # round 3: both encode kernels at once (needs a threshold that leaves samples on both sides)
    if env.get("TGX_LONG_THRESHOLD") in ("100", "1000") and rng.random() < 0.6: env["TGX_CORUN"] = str(int(rng.choice([16, 96, 200])))
    if rng.random() < 0.4: env["TGX_E5_HOT"] = str(int(rng.choice([0, 3, 40, 500])))
    if rng.random() < 0.3: env["TGX_E6_POOL"] = str(int(rng.choice([0, 4, 16, 128])))
    # round 3: the E-step on pieces (snippets cut where no match crosses), small windows
    if rng.random() < 0.5:
        env["TGX_ESTEP_PIECES"] = "1"
        env["TGX_ESTEP_WINDOW"] = str(int(rng.choice([256, 512, 2048])))
    snip = int(rng.choice([48, 1000, 4096, 81920]))   # drawn last: the fuzzer's E-step draws it after encode
    return dict(toks=toks, scores=scores, texts=texts, lens=lens, flat=flat, offs=offs, max_len=max_len,
                all_bytes=all_bytes, dropout=dropout, seed=sd, env=env, snip=snip,
                estep_dropout=dropout if dropout < 1.0 else 0.3)
