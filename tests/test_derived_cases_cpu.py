"""Every case of tests/derived_cases.py has the property it is named for, shown without a GPU from the oracle and the
checkers alone: which tokens a derivation drops and how they relate to the kept ones, that their bytes occur in the
texts, the child's longest token and lm against the parent's, which texts have a path, where the Viterbi path moves,
and, for the sampling legs, the key gaps at the chosen seed and the side of the rows kernel's range rule."""
import numpy as np
import pytest

from oracle import oracle as orc

import derived_cases as dc
import hostile_cases as hc
import util


def _multi(toks):
    return [t for t in toks if len(t) > 1]


def _occurs(tokens, texts):
    blob = b"\x00".join(texts)
    return sum(1 for t in tokens if t in blob)


@pytest.mark.parametrize("name", dc.SMALL_CASES)
def test_links_are_valid_and_texts_are_the_parents(name):
    c = dc.case(name)
    n = len(c["toks"])
    for keep, cs in c["links"]:
        assert keep.dtype == np.uint32 and cs.dtype == np.float64 and keep.size == cs.size
        assert keep.size == 0 or (int(keep[-1]) < n and np.all(np.diff(keep.astype(np.int64)) > 0))
        n = keep.size
    toks, scores = dc.child(c)
    assert len(toks) == len(scores) == n and set(toks) <= set(c["toks"])
    assert len({t for t in c["toks"] if t}) == len([t for t in c["toks"] if t])  # no duplicates: the library derives
    if name not in ("keep_one", "keep_none"):
        lens = [len(t) for t in c["texts"]]
        assert set(hc.EDGE_LENGTHS) <= set(lens) and max(lens) == 512
    # which texts have a path under the child
    for t in c["texts"]:
        assert dc.has_path(name, t), (name, len(t))
    for t in c["bad_texts"]:
        assert not dc.has_path(name, t), (name, t)
        assert len(dc.parent_oracle(name).encode(t)) >= 1  # the parent had one
    assert (name in dc.FULL_COVER) <= (all(bytes([b]) in set(toks) for b in range(256)) and bool(np.all(np.isfinite(scores))))


@pytest.mark.parametrize("name", ["prefix_holes", "dead_subtrees"])
def test_hole_patterns(name):
    c = dc.case(name)
    toks, _ = dc.child(c)
    kept, gone = _multi(toks), dc.dropped(c)
    assert len(gone) >= 100 and len(kept) >= 20 and all(len(t) > 1 for t in gone)
    if name == "prefix_holes":   # interior non-terminals on live paths
        assert all(any(k != g and k.startswith(g) for k in kept) for g in gone)
        assert not any(a != b and a.startswith(b) for a in kept for b in kept)
        assert max(map(len, toks)) == 16
    else:                        # dead subtrees below terminals: the deepest dropped token lies below the child's lm
        assert all(any(k != g and g.startswith(k) for k in kept) for g in gone)
        assert not any(a != b and a.startswith(b) for a in kept for b in kept)
        assert max(map(len, gone)) == 16 > dc.child_lm(c) == 8 and max(map(len, toks)) <= 6
    assert _occurs(gone, c["texts"]) >= len(gone) // 2


@pytest.mark.parametrize("name", list(dc.LEN_CASES))
def test_lm_moves_across_the_kernel_boundaries(name):
    n, target = dc.LEN_CASES[name]
    c = dc.case(name)
    toks, _ = dc.child(c)
    gone = dc.dropped(c)
    assert max(map(len, c["toks"])) == n and max(map(len, toks)) == target
    parent_lm = max(4, (n + 3) & ~3)
    assert dc.child_lm(c) == {"len16_to_le8": 8, "len32_to_16": 16, "len33_to_32": 32, "len64_to_16": 16, "len64_to_4": 4}[name] < parent_lm
    # the families: fused above 32, the 17..32 kernels, the <= 16 kernels
    family = lambda lm: 0 if lm <= 16 else 1 if lm <= 32 else 2
    if name != "len16_to_le8":
        assert family(dc.child_lm(c)) < family(parent_lm)
    assert all(len(t) > target for t in gone) and max(map(len, gone)) == n > dc.child_lm(c)  # dead branches deeper than lm
    assert all(bytes([b]) in set(toks) for b in range(256))
    assert _occurs([t for t in gone if len(t) == n], c["texts"]) >= 1 and _occurs(gone, c["texts"]) >= 5


def test_byte_dropped():
    c = dc.case("byte_dropped")
    toks, _ = dc.child(c)
    assert dc.dropped(c) == [b"\xff"] and len(toks) == len(c["toks"]) - 1
    assert toks[0xFE] == b"\xfe" and toks[0xFF] == c["toks"][0x100]       # every id above the byte moves down by one
    assert all(b"\xff" in t for t in c["bad_texts"]) and not any(b"\xff" in t for t in c["texts"])
    texts, bad = dc.with_bad_texts(c)
    assert len(bad) == 2 and len(texts[bad[0]]) < len(texts[bad[1]])
    with pytest.raises(orc.NoPath) as e:
        dc.oracle("byte_dropped").encode_batch_flat(*orc.pack(texts))
    assert (e.value.sample, e.value.pos) == (bad[0], len(texts[bad[0]]))


def test_identity_derivations():
    same, new = dc.case("keep_all_same_scores"), dc.case("keep_all_new_scores")
    for c in (same, new):
        assert dc.child(c)[0] == c["toks"] and dc.dropped(c) == []
    assert np.array_equal(dc.child(same)[1].view(np.uint64), same["scores"].view(np.uint64))
    # new scores: the Viterbi path moves on at least one text (here: on most of them)
    par, chi = dc.parent_oracle("keep_all_new_scores"), dc.oracle("keep_all_new_scores")
    moved = [i for i, t in enumerate(new["texts"]) if par.encode(t) != chi.encode(t)]
    assert len(moved) >= 1, moved
    assert any(len(new["texts"][i]) == 512 for i in moved)


@pytest.mark.parametrize("name", ["keep_one", "keep_none"])
def test_nearly_empty_children(name):
    c = dc.case(name)
    toks, scores = dc.child(c)
    assert len(toks) == (1 if name == "keep_one" else 0)
    assert b"" in c["texts"] and dc.oracle(name).encode(b"") == []
    assert c["bad_texts"] and dc.child_lm(c) == 4
    if name == "keep_one":
        assert toks == [b"a"] and dc.oracle(name).encode(b"a" * 33) == [0] * 33
    else:
        assert all(len(t) == 0 for t in c["texts"])


def test_score_edges():
    c = dc.case("scores_past_300")
    _, scores = dc.child(c)
    assert max(map(len, c["toks"])) == 16 and float(np.abs(c["scores"]).max()) <= 300.0  # the parent is estep7's
    assert scores.min() == -301.0 and int((scores < -300.0).sum()) == 1
    assert dc.estep_kernels("scores_past_300")[0] == "log"
    chi = dc.oracle("scores_past_300")
    assert any(ord("b") in chi.encode(t) for t in c["texts"])              # the token at -301 lies on Viterbi paths
    c = dc.case("scores_minus_inf")
    toks, scores = dc.child(c)
    bad = np.nonzero(np.isneginf(scores))[0]
    assert bad.size == 1 and len(toks[int(bad[0])]) > 1 and np.isfinite(np.delete(scores, bad)).all()
    assert _occurs([toks[int(bad[0])]], c["texts"]) == 1                  # the token occurs, and no path may take it
    assert not any(int(bad[0]) in dc.oracle("scores_minus_inf").encode(t) for t in c["texts"])


def test_empty_token_parent():
    c = dc.case("empty_token_parent")
    assert c["toks"][300] == b"" and c["toks"].count(b"") == 1
    first, _ = dc.child(c, 1)
    last, _ = dc.child(c)
    assert b"" in first and b"" not in last and len(last) == len(first) - 1
    assert first.index(b"") < len(first) - 1                               # ids after it move in the second link


def test_chain3():
    c = dc.case("chain3")
    assert len(c["links"]) == 3
    lms = [max(4, (max(map(len, dc.child(c, d)[0])) + 3) & ~3) for d in range(4)]
    assert lms == [36, 32, 32, 16], lms
    t1, t2, t3 = dc.child(c, 1)[0], dc.child(c, 2)[0], dc.child(c, 3)[0]
    gone2 = [t for t in t1 if t not in set(t2)]
    assert gone2 and all(any(k != g and k.startswith(g) for k in _multi(t2)) for g in gone2)
    assert len(t3) < len(t2) < len(t1) < len(c["toks"])


def test_m_step_real():
    c = dc.case("m_step_real")
    toks, scores = dc.child(c)
    assert len(c["toks"]) == 4000 and 256 < len(toks) < 4000 and all(bytes([b]) in set(toks) for b in range(256))
    assert len(set(scores.tolist())) > len(toks) // 2                      # every token its own score, as after an M-step
    assert dc.estep_kernels("m_step_real") == ("linear", "estep7_kernel")


@pytest.mark.parametrize("name", ["big_parent_40", "big_parent_60"])
def test_big_parent(name):
    c = dc.case(name)
    toks, scores = dc.child(c)
    frac = int(name[11:]) / 100.0
    assert len(c["toks"]) == 500000 and len(toks) == int(500000 * frac)
    assert c["above_trie8"] == (c["n_slots"] > dc.TRIE8_MAX_SLOTS)
    assert (2 * len(toks) <= len(c["toks"])) == (name == "big_parent_40")   # the refusal's other condition
    assert len(c["texts"]) == 40 and all(dc.has_path(name, t) for t in c["texts"])
    print(f"{name}: parent table {c['n_slots']} slots, above the 8-byte records' limit: {c['above_trie8']}")


@pytest.mark.parametrize("name", dc.SAMPLING_CASES)
def test_sampling_legs(name):
    """The seed search of hostile_cases.sampling_case with its 1..64 bound found a seed at which every gap holds; every
    text lies on the side of the range rule its expected kernel needs; the 80-bit log Z confirms the checker's."""
    s = dc.sampling(name)
    lens = [len(t) for t in s["texts"]]
    assert 1 <= s["seed"] <= 64 and hc.gaps_hold(s["checked"], lens)
    c = dc.case(name)
    assert s["expect"] == ("generic" if name == "scores_past_300" else "rows")
    if s["expect"] == "rows":
        assert dc.child_lm(c) <= 32 and max(s["margins"]) <= hc.STAY_BITS, max(s["margins"])
    for chk, t, truth in zip(s["checked"], s["texts"], s["truth"]):
        assert chk["ids"] is not None and b"".join(s["toks"][i] for i in chk["ids"]) == t
        assert abs(chk["logz"] - truth) <= 1e-9 * max(1.0, abs(truth))


@pytest.mark.parametrize("name", dc.SAMPLING_CASES)
def test_stats_legs_are_on_one_side_of_the_range_rule(name):
    """By 50 bits, as the sampling cases of tests/hostile_cases.py are.  The child with a score at -301 is the one that
    trips the rule at alpha 0.3 (90 nats a byte on a run of that byte) and goes to the generic kernel outright at 1."""
    for alpha in dc.STATS_ALPHAS:
        want = "rows"
        if name == "scores_past_300":
            want = "generic" if alpha == 1.0 else "fallback"
        assert dc.stats_expect(name, alpha) == want, (name, alpha)
        z, es, et, n = dc.stats_truth(name, alpha)
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(es)) and np.all(et[n > 0] >= 1.0)


@pytest.mark.parametrize("name", dc.ESTEP_CASES)
def test_estep_truth_exists(name):
    """The 80-bit E-step of the child over the case's corpus succeeds (what util.assert_estep_truth asserts first), at
    dropout 0 and 0.05, and the f64 oracle's support is the truth's."""
    om = dc.oracle(name)
    flat, offs = dc.count_corpus(name)
    assert flat.size <= dc.COUNT_SLICE + 8192
    for dropout, seed in ((0.0, 0), (0.05, 3)):
        st, truth, tz, _ = util.estep_truth(om, flat, offs, 81920, dropout, seed)
        assert st == orc.OK and np.isfinite(tz)
        st, want, wz, _ = om.estep_flat(flat, offs, 81920, dropout, seed, threads=8)
        assert st == orc.OK and np.array_equal(want != 0, truth != 0)
    assert dc.estep_kernels(name)[0] in ("linear", "log")
