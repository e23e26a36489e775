"""The randomised cases of the lattice passes (tests/lattice_fuzz_cases.py), established without a device over the list
that tests/test_lattice_fuzz_gpu.py runs: cases 0 .. N_CASES - 1 of seed SEED0.

  * every case finds a sampling seed within its 8 tries;
  * the f64 host twin of the statistics (tgx_lattice_stats_host, the kernels' own log-domain recurrences) meets the bounds
    that stats_kernel is held to (stats_cases.logz_bound, stats_cases.twin_bound, the entropy's sum of the two) on every sample
    of every case, and marks the samples without a path that the checker marks;
  * on the samples of at most 14 bytes the checkers and the truth agree with the sum over all segmentations
    (sample_checker.enumerate_segmentations, nbest_checker.brute_force);
  * truth_ext, the truth of a sample whose lattice marginal_ext does not represent, is marginal_ext's where both apply;
  * the list covers what it was drawn for (COVERAGE: at least two cases of each).

N_CASES = 160: the largest multiple of 8 with which this module and the reference side of the GPU module each stay under about
a minute on the CPU machine of this change.  Measured there, one process, the cases built once and shared by the tests: 48.3 s
for this module (44.7 s of it building the cases and their expectations; the twin 0.4 s, truth_ext against marginal_ext 2.0 s,
the sums over all segmentations 0.1 s), 45.9 s for the reference side of the GPU module.  With 168 cases: 61.8 s and 56.9 s."""
import math

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import _lib

import lattice_fuzz_cases as lf
import nbest_checker as nc
import sample_checker as sc


def _cases():
    return [lf.case(lf.SEED0, i) for i in range(lf.N_CASES)]


def test_every_case_finds_a_sampling_seed():
    for c in _cases():
        assert c["seed"] is not None and c["seed_base"] <= c["seed"] < c["seed_base"] + 8, lf.tag(c)
        assert len(c["checked"]) == len(c["texts"]) == len(c["nbest"]) == c["z"].size
        for j, w in enumerate(c["checked"]):  # the checker and the truth name the same samples as without a path
            assert (w["logz"] == lf.NINF) == (c["z"][j] == lf.NINF) == (j in c["no_path"]) == (c["nbest"][j][0] == []), (lf.tag(c), j)
            if j not in c["no_path"]:
                assert abs(w["logz"] - c["z"][j]) <= 1e-9 * max(1.0, abs(c["z"][j])), (lf.tag(c), j)


def test_a_case_is_its_seed_and_number():
    a, b = lf.make_case(lf.SEED0, 3), lf.make_case(lf.SEED0, 3)
    assert a["texts"] == b["texts"] and a["toks"] == b["toks"] and np.array_equal(a["scores"], b["scores"])
    assert (a["alpha"], a["k"], a["env"], a["seed"], a["forms"], a["order"]) == (b["alpha"], b["k"], b["env"], b["seed"], b["forms"], b["order"])
    assert lf.tag(a) == lf.tag(lf.case(lf.SEED0, 3))


def test_the_twin_meets_every_stats_bound():
    worst = {"logz": 0.0, "escore": 0.0, "etokens": 0.0, "entropy": 0.0}
    for c in _cases():
        st = _lib.lattice_stats_host(c["toks"], c["scores"], c["flat"], c["offs"], c["alpha"])
        assert len(st) == len(c["texts"]) and st.n_no_path == len(c["no_path"]), lf.tag(c)
        assert np.nonzero(st.no_path)[0].tolist() == c["no_path"], lf.tag(c)
        ok = np.array([j not in c["no_path"] for j in range(len(c["texts"]))], bool)
        if not ok.all():
            assert np.all(np.isneginf(st.logz[~ok])) and np.all(np.isnan(st.expected_score[~ok])) and np.all(np.isnan(st.expected_tokens[~ok]))
        if not ok.any():
            continue
        n, z, es, et = np.array(c["lens"], np.float64)[ok], c["z"][ok], c["es"][ok], c["et"][ok]
        zb, eb, tb, hb = lf.stats_bounds(False, n, z, es, et, c["alpha"])
        errs = {"logz": (np.abs(st.logz[ok] - z), zb), "escore": (np.abs(st.expected_score[ok] - es), eb),
                "etokens": (np.abs(st.expected_tokens[ok] - et), tb), "entropy": (np.abs(st.entropy[ok] - (z - c["alpha"] * es)), hb)}
        for what, (d, b) in errs.items():
            worst[what] = max(worst[what], float((d / b).max()))
            assert np.all(d <= b), (lf.tag(c), what, int(np.argmax(d / b)), float(d.max()), float((d / b).max()))
    print("[lattice fuzz] the twin's largest error-to-bound ratios:", {k: f"{v:.3g}" for k, v in worst.items()})


def _close(got, want, what):
    # at most 14 bytes: a few dozen operations on either side, each within a few ulp of values of the result's size
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (what, got, want)


def test_the_checkers_agree_with_the_sum_over_all_segmentations():
    seen = 0
    for c in _cases():
        toks, scores, alpha, k = c["toks"], c["scores"], c["alpha"], c["k"]
        for j, (t, inc) in enumerate(zip(c["texts"], c["inc"])):
            n = len(t)
            if n > lf.BRUTE_MAX:
                continue
            what = (lf.tag(c), j, t)
            segs = sc.enumerate_segmentations(inc, n)
            if not segs:
                assert j in c["no_path"], what
                continue
            seen += 1
            probs, logz = sc.segmentation_probs(inc, scores, n, alpha)
            _close(c["checked"][j]["logz"], logz, what)
            _close(c["z"][j], logz, what)
            assert tuple(c["checked"][j]["ids"]) in probs, what
            _close(c["es"][j], math.fsum(p * math.fsum(float(scores[i]) for i in s) for s, p in probs.items()), what)
            _close(c["et"][j], math.fsum(p * len(s) for s, p in probs.items()), what)
            rows, scs = nc.brute_force(inc, scores, n)
            assert c["nbest"][j][0] == rows[:k] and c["nbest"][j][1] == scs[:k], what
    assert seen >= 100, seen


def test_truth_ext_is_marginal_ext_where_both_apply():
    """Samples of up to 600 bytes in which a token ends and one begins at every position: the two 80-bit sums differ by
    their own roundings, a few 2^-64 per position."""
    seen = 0
    for c in _cases():
        om = orc.OracleModel(c["toks"], c["alpha"] * c["scores"])
        for j, (t, inc) in enumerate(zip(c["texts"], c["inc"])):
            if 0 < len(t) <= 600 and seen < 400 and j % 3 == 0 and lf.covered(inc, len(t)):
                seen += 1
                a, b = lf.truth_ext(inc, c["scores"], len(t), c["alpha"]), lf.truth(om, inc, c["scores"], t, c["alpha"])
                for x, y in zip(a, b):
                    assert abs(x - y) <= 1e-15 * max(1.0, abs(y)) * max(1.0, math.sqrt(len(t))), (lf.tag(c), j, a, b)
    assert seen >= 100, seen


def coverage(cases) -> dict:
    """What the list holds -> the number of cases that hold it."""
    cnt = {}

    def add(name, yes):
        cnt[name] = cnt.get(name, 0) + (1 if yes else 0)

    for c in cases:
        toks, ml = c["toks"], c["max_len"]
        add("tokens <= 16", ml <= 16)
        add("tokens 17-32", 17 <= ml <= 32)
        add("tokens 33-64", 33 <= ml <= 64)
        add("no byte cover, a later sample without a path", not c["info"]["all_bytes"] and any(j > 0 for j in c["no_path"]))
        first = {}
        for i, t in enumerate(toks):
            first.setdefault(t, i)
        add("a duplicate token matches", len(first) < len(toks) and any(first[toks[t]] != t for inc in c["inc"] for at in inc for _, t in at))
        for f in lf.HOSTILE:
            add("family " + f, c["family"] == f)
        add("derived", c["parent"] is not None)
        for name, values in (("TGX_SAMPLE_PATH", (None, "generic")), ("TGX_STATS_PATH", (None, "generic", "rows")), ("TGX_NBEST_CHUNK_MB", (None, "1"))):
            for v in values:
                add(f"{name}={v}", c["env"].get(name) == v)
        for p in lf.PASSES:
            add(p + " on a batch", not c["forms"][p])
            add(p + " on a corpus", c["forms"][p])
        for k in lf.KS:
            add(f"k={k}", c["k"] == k)
        add("n-best in >= 2 chunks", c["chunks"] >= 2)
        top = float(np.abs(c["alpha"] * c["scores"]).max())
        add("max |alpha score| in [206, 207]", 206.0 <= top <= 207.0)
        add("max |alpha score| in (207, 208.5]", 207.0 < top <= 208.5)
        add("a poison sample", c["poisoned"] is not None and c["trips"])
        add("S = 0", len(c["texts"]) == 0)
        add("only empty samples", len(c["texts"]) > 0 and max(c["lens"]) == 0)
        add("a sample above 64 KiB", max(c["lens"], default=0) > 65536)
        assert sum(c["lens"]) - (max(c["lens"]) if max(c["lens"], default=0) > 65536 else 0) <= lf.TEXT_CAP, lf.tag(c)
    return cnt


def test_the_list_covers_what_it_was_drawn_for():
    cnt = coverage(_cases())
    print("[lattice fuzz] coverage:", cnt)
    short = {k: v for k, v in cnt.items() if v < 2}
    assert not short, short
