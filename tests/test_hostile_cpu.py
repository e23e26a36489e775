"""What the hostile GPU tests (tests/test_sample_hostile_gpu.py, tests/test_nbest_hostile_gpu.py) rely on, established
without a GPU from the checkers alone: the range rule's restatement on hand-computed cases, every sampling case on its
side of the rule by 50 bits, the selection thresholds, the key gaps at the chosen seeds, the law of the checker's own
draws, and the n-best checker against brute force on the tied and the collapsing vocabulary."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc

import hostile_cases as hc
import nbest_checker as nc
import sample_checker as sc

LN2 = math.log(2.0)


def _inc(toks, scores, text):
    return sc.incoming(orc.OracleModel(toks, scores), text, max(map(len, toks)))


def test_margin_of_a_run_of_byte_tokens():
    """40 bytes that only byte tokens at -100 cover: A[p] = -100 p exactly.  Block 0 (scale 0) ends at position 31, so
    its distance is 3100 / ln 2 = 4472.4 bits; block 1's scale is the exponent of A[32], position 40 lies 800 / ln 2 =
    1154.2 bits below A[32].  At alpha = 0.01 the step is 1.44 bits: 31 / ln 2 = 44.7 bits."""
    toks, scores = hc.bytes_heavy(-100.0)
    inc = _inc(toks, scores, hc.POISON_DESIGNED)
    assert hc.forward(inc, scores, 40, 1.0) == [-100.0 * p for p in range(41)]
    assert abs(hc.rows_range_margin(inc, scores, 40, 1.0) - 3100.0 / LN2) <= 1.0
    assert abs(hc.rows_range_margin(inc, scores, 31, 1.0) - 3100.0 / LN2) <= 1.0
    assert abs(hc.rows_range_margin(inc, scores, 40, 0.01) - 31.0 / LN2) <= 1.0
    # one 32-byte token at -3, then 8 bytes at -100 each: block 0 holds position 0 alone (distance 0), block 1's scale
    # is the exponent of A[32] = -3 and position 40 lies 800 / ln 2 = 1154.2 bits below it
    head = bytes(range(0x40, 0x60))
    toks2, scores2 = [head] + [bytes([c]) for c in range(0xA0, 0xA8)], np.array([-3.0] + [-100.0] * 8)
    text = head + bytes(range(0xA0, 0xA8))
    inc2 = _inc(toks2, scores2, text)
    assert hc.forward(inc2, scores2, 40, 1.0)[31:34] == [hc.NINF, -3.0, -103.0]
    assert abs(hc.rows_range_margin(inc2, scores2, 40, 1.0) - 800.0 / LN2) <= 1.0
    assert hc.rows_range_margin(inc2, scores2[:1], 32, 1.0) <= 1.0


def test_margin_of_a_text_whose_blocks_stay_close():
    """b"ab" * 100 with tokens a, b at -1 and ab at -1.5: a pair adds log(e^-2 + e^-1.5) = -1.026, so A[200] = -102.6 lies
    148 bits below A[0], while a block of 32 positions spans 16 pairs: 16.5 * 1.026 / ln 2 = 24.4 bits (and one for the
    exponent).  One scale for the whole text would give the 148."""
    toks, scores = [b"a", b"b", b"ab"], np.array([-1.0, -1.0, -1.5])
    text = b"ab" * 100
    inc = _inc(toks, scores, text)
    A = hc.forward(inc, scores, 200, 1.0)
    pair = math.log(math.exp(-2.0) + math.exp(-1.5))
    assert abs(A[200] - 100 * pair) < 1e-9 and abs(A[200] / LN2 + 148.0) < 0.1
    m = hc.rows_range_margin(inc, scores, 200, 1.0)
    assert 15.5 * -pair / LN2 - 1.0 <= m <= 16.5 * -pair / LN2 + 1.0, m
    assert hc.rows_range_margin(inc, scores, 200, 0.0) <= 32.0  # alpha 0 counts paths: at most one bit per position
    # unreachable positions do not count, and a text nothing reaches gives 0
    inc = _inc(toks, scores, b"abxab")
    assert hc.rows_range_margin(inc, scores, 5, 1.0) <= 3.0 / LN2 + 1.0
    assert hc.forward(inc, scores, 5, 1.0)[3:] == [hc.NINF] * 3


@pytest.mark.parametrize("name", hc.SAMPLING_CASES)
def test_sampling_case_is_as_designed(name):
    c = hc.sampling_case(name)
    toks, scores, alpha, texts = c["toks"], c["scores"], c["alpha"], c["texts"]
    lens = [len(t) for t in texts]
    assert max(lens) <= 512
    if name not in ("real_trip", "real_stay"):
        assert sorted(lens)[:1] == [0] and set(hc.EDGE_LENGTHS) <= set(lens)
    # which kernel a plain call ends on: the launcher's rule (lm <= 32 and every |alpha * score| <= 207), then the range
    lm = max(4, (max(map(len, toks)) + 3) & ~3)
    weights_fit = bool(np.all(np.abs(alpha * scores) <= 207.0))
    if c["expect"] == "generic":
        assert lm > 32 or not weights_fit
        if name == "score207_5":
            assert lm <= 32 and float(np.abs(alpha * scores).max()) == 207.5
        if name == "len33":
            assert max(map(len, toks)) == 33 and lm == 36
    else:
        assert lm <= 32 and weights_fit
        m = c["margins"]
        assert all(x <= hc.STAY_BITS or x >= hc.TRIP_BITS for x in m), sorted(m)
        assert (max(m) >= hc.TRIP_BITS) == (c["expect"] == "fallback"), max(m)
    if name == "score207":
        assert float(np.abs(alpha * scores).max()) == 207.0
    if name == "len32":
        assert max(map(len, toks)) == 32
    # every sample has a path, a finite log Z that the 80-bit truth confirms, and its gaps at the chosen seed
    assert 1 <= c["seed"] <= 64
    for i, (w, n, z) in enumerate(zip(c["checked"], lens, c["truth"])):
        assert w["ids"] is not None and b"".join(toks[t] for t in w["ids"]) == texts[i]
        assert w["gap"] >= 1e-6 and w["gap"] >= 100.0 * hc.log_rounding_model(n, w["logz"]), (i, w["gap"])
        assert abs(w["logz"] - z) <= hc.logz_bound("sample_kernel", n, z), (i, w["logz"], z)
    assert hc.gaps_hold(c["checked"], lens)


def test_sampling_cases_hold_the_tokens_they_are_about():
    """The long-token cases put their longest token on a sampled path, across a block boundary of the kernel that runs;
    the threshold cases put the token with the extreme score on a path; the poison runs are sampled byte by byte."""
    c = hc.sampling_case("len32")
    spans = [sp for w in c["checked"] for sp in hc.path_tokens(w["ids"], c["toks"])]
    assert any(ln == 32 and q % 32 != 0 for q, ln in spans) and any(ln == 31 for q, ln in spans)
    for name, ml in (("len33", 33), ("len64", 64)):
        c = hc.sampling_case(name)
        spans = [sp for w in c["checked"] for sp in hc.path_tokens(w["ids"], c["toks"])]
        assert any(ln == ml and q // 64 != (q + ln) // 64 for q, ln in spans), name
    for name in ("score207", "score207_5"):
        c = hc.sampling_case(name)
        assert sum(ord("z") in w["ids"] for w in c["checked"]) >= 10
    c = hc.sampling_case("designed_trip")
    i = c["texts"].index(hc.POISON_DESIGNED)
    assert c["checked"][i]["ids"] == list(hc.POISON_DESIGNED) and c["margins"][i] >= hc.TRIP_BITS
    c = hc.sampling_case("real_trip")
    i = [j for j, t in enumerate(c["texts"]) if b"\x80" * 64 in t]
    assert len(i) == 1 and c["margins"][i[0]] >= hc.TRIP_BITS
    assert sum(m >= hc.TRIP_BITS for m in c["margins"]) == 1
    # the arithmetic of DESIGN.md: the byte tokens 0x80 .. 0xFE of the committed vocabulary at alpha = 5
    toks, scores = hc.spec_32000()
    s80 = float(scores[toks.index(b"\x80")])
    assert abs(s80 + 5.92) < 0.01 and abs(5.0 * -s80 / LN2 - 42.7) < 0.1 and math.ceil(600.0 / (5.0 * -s80 / LN2)) == 15


def test_no_path_samples():
    """The two failing samples of the no-path test have no path, and what of them is reachable stays in range."""
    c = hc.sampling_case("nopath_stay")
    assert b"\xff" not in c["toks"] and len(c["toks"]) == 255 + 24
    om = orc.OracleModel(c["toks"], c["scores"])
    for t in hc.NOPATH_BAD:
        inc = sc.incoming(om, t, 8)
        assert sc.check_sample(inc, c["scores"], len(t), c["alpha"], c["seed"], 0)["ids"] is None
        assert hc.rows_range_margin(inc, c["scores"], len(t), c["alpha"]) <= hc.STAY_BITS
        with pytest.raises(orc.NoPath):
            om.encode(t)


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_the_law_of_the_checker_after_the_poison(alpha):
    """The checker's own draws of N = 20 000 copies of b"abcabca" (sample indices 0 .. N - 1, seed 99) meet the
    total-variation and 5-sigma rules the GPU test applies, and the poison sample trips the range rule."""
    toks, scores = hc.tiny_poisoned()
    text, N = b"abcabca", hc.LAW_N
    inc = _inc(toks, scores, text)
    probs, _ = sc.segmentation_probs(inc, scores, len(text), alpha)
    cnt = {}
    for i in range(N):
        row = tuple(sc.check_sample(inc, scores, len(text), alpha, hc.LAW_SEED, i)["ids"])
        cnt[row] = cnt.get(row, 0) + 1
    hc.assert_law(cnt, probs, N)
    assert hc.rows_range_margin(_inc(toks, scores, hc.LAW_POISON), scores, len(hc.LAW_POISON), alpha) >= hc.TRIP_BITS
    assert hc.rows_range_margin(inc, scores, len(text), alpha) <= hc.STAY_BITS
    assert float(np.abs(alpha * scores).max()) <= 207.0


TIED_TEXTS = [b"a" * n for n in (1, 2, 5, 6, 8, 9, 13, 14)]
COLLAPSING_TEXTS = [b"abcabcdab", b"ccc", b"abcdabcdabcdab", b"baab", b"aabab", b"dabcdd", b"cabcabcab", b"bcdbcdcd", b"abababab",
                    b"cdcacdcabcd"]


@pytest.mark.parametrize("vocab,texts", [(lambda: hc.all_ties(8), TIED_TEXTS), (hc.collapsing, COLLAPSING_TEXTS)])
def test_nbest_checker_against_brute_force(vocab, texts):
    toks, scores = vocab()
    om = orc.OracleModel(toks, scores)
    for text in texts:
        assert len(text) <= 14
        inc = sc.incoming(om, text, max(map(len, toks)))
        want_rows, want_scores = nc.brute_force(inc, scores, len(text))
        assert want_rows
        for k in range(1, 17):
            rows, scs = nc.nbest(inc, scores, len(text), k)
            assert rows == want_rows[:k] and scs == want_scores[:k], (text, k)
            assert len(rows) == min(k, len(want_rows))
        assert want_rows[0] == om.encode(text)


def test_all_ties_gives_sixteen_equal_scores():
    for ml in (8, 16, 33, 64):
        toks, scores = hc.all_ties(ml)
        om = orc.OracleModel(toks, scores)
        for n in (6, 7, 40):
            rows, scs = nc.nbest(sc.incoming(om, b"a" * n, ml), scores, n, 16)
            assert len(rows) == 16 and scs == [-3.0 * n] * 16 and len({tuple(r) for r in rows}) == 16
        # a...a of n <= max_len bytes has 2^(n - 1) segmentations
        for n in (1, 2, 3, 4, 5):
            assert len(nc.nbest(sc.incoming(om, b"a" * n, ml), scores, n, 16)[0]) == 2 ** (n - 1)


def test_collapsing_really_collapses():
    """Among the 16 rows of some sample two rows have the same f64 score and different exact sums; the token at +2.5, the
    token at 0.0 and the later id of the duplicated token are on rows, the earlier id on none."""
    c = hc.nbest_case("collapsing")
    toks, scores = c["toks"], c["scores"]
    exact = lambda row: sum(Fraction(float(scores[t])) for t in row)
    collapsed, used = 0, set()
    for rows, scs in c["want"]:
        used.update(t for r in rows for t in r)
        for a in range(len(rows)):
            for b in range(a + 1, len(rows)):
                if scs[a] == scs[b] and exact(rows[a]) != exact(rows[b]):
                    collapsed += 1
    assert collapsed >= 10, collapsed
    assert {toks.index(b"ba"), toks.index(b"aa"), 15} <= used and 4 not in used
    assert scores[toks.index(b"ba")] == 2.5 and scores[toks.index(b"aa")] == 0.0 and scores.min() < -1e15


def test_nbest_cases_hold_what_they_are_about():
    c = hc.nbest_case("len64")
    lens = {ln for rows, _ in c["want"] for r in rows for _, ln in hc.path_tokens(r, c["toks"])}
    assert {63, 64} <= lens
    for name, ml in (("ties16", 16), ("ties33", 33), ("ties64", 64)):
        c = hc.nbest_case(name)
        assert {ln for rows, _ in c["want"] for r in rows for _, ln in hc.path_tokens(r, c["toks"])} >= {ml, ml - 1}
        short = {len(t): len(w[0]) for t, w in zip(c["texts"], c["want"]) if len(w[0]) < 16}
        assert short == {0: 1, 1: 1, 2: 2, 3: 4, 4: 8}
    c = hc.nbest_case("big_ids")
    assert len(c["toks"]) == 500000 and max(t for rows, _ in c["want"] for r in rows for t in r) >= 1 << 16
    assert all(len(rows) == 16 for rows, _ in c["want"]) and max(map(len, c["texts"])) <= 512
