"""Derived models (tgx_model_create_derived) on every device pass, at the vocabulary's edges (cases: tests/derived_cases.py,
established on the CPU by tests/test_derived_cases_cpu.py; the table derivation itself: tests/test_derive_native.py).

Per case the parent is created, the child derived (a chain: link by link) and THE PARENT FREED before the child runs
anything, as tokengeex_amd/prune.py does.  Every expectation is the oracle's for the child's vocabulary, never another
model's of the library: encode bit-exact on every kernel path the child's lm admits, the integer counting passes ==,
the E-step against the 80-bit truth with util.assert_estep_truth's bounds (the kernel family a plain call takes, and the
chained, log-domain and generic kernels and the pieces of cuts.hip forced), prune_alternatives ==, sampling ids == the
checker's with log Z within hostile_cases.logz_bound, n-best == nbest_checker's, the lattice statistics within the
bounds of tests/test_stats_gpu.py, decode and spans from the child's token bytes.  Which kernels ran is read from
last_kernel_times() for every leg: no case takes a fallback unseen.  (The E-step adds with floating-point atomics, so
the identity derivation is held to the truth like every other case, not to its parent's bits.)"""
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, tensors

import decode_checker as dk
import derived_cases as dc
import hostile_cases as hc
import spans_checker as sp
import stats_cases as sx
import util

ENCODE_KERNELS = {"encode_kernel", "encode2_kernel", "encode4_kernel", "encode4l_kernel", "encode5_kernel", "encode6_kernel"}
SAMPLE_KERNELS = {"sample_wslot_kernel", "sample_rows_kernel", "sample_kernel", "trace32_kernel"}
SAMPLE_RAN = {"rows": {"sample_wslot_kernel", "sample_rows_kernel", "trace32_kernel"}, "generic": {"sample_kernel"}}
STATS_KERNELS = {"sample_wslot_kernel", "stats_rows_kernel", "stats_kernel"}
STATS_RAN = {"rows": {"sample_wslot_kernel", "stats_rows_kernel"}, "generic": {"stats_kernel"},
             "fallback": {"sample_wslot_kernel", "stats_rows_kernel", "stats_kernel"}}
NO_SPECIALS = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))


def derive(name: str, for_estep: bool = False):
    """The case's last child, every ancestor freed as soon as its child exists."""
    c = dc.case(name)
    m = tgx.NativeModel(c["toks"], c["scores"], for_estep=for_estep)
    for keep, cs in c["links"]:
        nxt = m.derive(keep, cs, for_estep=for_estep)
        m.free()
        m = nxt
    assert m.vocab_size == len(dc.child(c)[0]) and m.max_token_len == max([len(t) for t in dc.child(c)[0]] or [0])
    return m


@functools.lru_cache(maxsize=None)
def _child(name: str, for_estep: bool = False):
    """One derived model per (case, flag) for the module; its parent no longer exists."""
    return derive(name, for_estep)


def _rows(res):
    ids, oo = res.ids().copy(), res.offsets().copy()
    res.free()
    return ids, oo


def _encode_paths(name):
    """(TGX_PATH or None, the kernel that must run) for every path the child's lm and scores admit."""
    c = dc.case(name)
    lm, scores = dc.child_lm(c), dc.child(c)[1]
    if not np.all(np.isfinite(scores)):
        return [(None, "encode_kernel")]   # no hash, no 8-byte records: the fused kernel, on a table built for the rows kernels
    if lm <= 16:
        return [(None, "encode5_kernel"), ("rows4", "encode4_kernel"), ("fused", "encode_kernel")]
    return [(None, "encode5_kernel"), ("rows4", "encode4l_kernel"), ("rows2", "encode2_kernel"), ("fused", "encode_kernel")]


# ---- encode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("for_estep", [False, True])
@pytest.mark.parametrize("name", dc.SMALL_CASES)
def test_encode(name, for_estep, monkeypatch):
    c = dc.case(name)
    nat, ora = _child(name, for_estep), dc.oracle(name)
    flat, offs = tgx.pack(c["texts"])
    monkeypatch.setenv("TGX_LONG_THRESHOLD", "0")
    for path, kernel in _encode_paths(name):
        if path:
            monkeypatch.setenv("TGX_PATH", path)
        for dropout, seed in ((0.0, 0), (0.1, 5)):
            util.assert_same_encoding(nat, ora, flat, offs, dropout, seed)
            ran = set(nat.last_kernel_times()) & ENCODE_KERNELS
            assert ran == {kernel}, (name, path, dropout, ran)
        monkeypatch.delenv("TGX_PATH", raising=False)
    # a threshold low enough that the 512-byte text goes to encode6_kernel (tokens of at most 16 bytes, 8-byte records)
    if _encode_paths(name)[0][1] == "encode5_kernel" and dc.child_lm(c) <= 16 and max(map(len, c["texts"])) >= 512:
        monkeypatch.setenv("TGX_LONG_THRESHOLD", "256")
        for dropout, seed in ((0.0, 0), (0.1, 5)):
            util.assert_same_encoding(nat, ora, flat, offs, dropout, seed)
            assert {"encode5_kernel", "encode6_kernel"} <= set(nat.last_kernel_times()), (name, nat.last_kernel_times())


@pytest.mark.parametrize("name", ["byte_dropped", "keep_one", "keep_none"])
def test_no_path_is_the_oracles(name):
    """Samples without a path under the child: TGX_ERR_NO_PATH names the oracle's sample and position, from encode, the
    counting passes and sampling alike; lattice_stats marks exactly those rows; the other rows are what they are alone."""
    c = dc.case(name)
    nat, ora = _child(name), dc.oracle(name)
    texts, bad = dc.with_bad_texts(c)
    flat, offs = tgx.pack(texts)
    with pytest.raises(orc.NoPath) as want:
        ora.encode_batch_flat(flat, offs)
    assert want.value.sample == bad[0]
    corpus = tgx.NativeCorpus(flat, offs)
    calls = [lambda: nat.encode_batch_flat(flat, offs), lambda: nat.encode_corpus(corpus), lambda: nat.count_tokens(corpus),
             lambda: nat.count_pairs(corpus), lambda: nat.encode_batch_sample_flat(flat, offs, 1.0, 3)]
    for call in calls:
        with pytest.raises(tgx.TokenGeeXError) as got:
            call()
        assert got.value.status == _lib.ERR_NO_PATH
        assert (got.value.sample, got.value.pos, got.value.length) == (want.value.sample, want.value.pos, len(texts[bad[0]]))
    st = nat.lattice_stats_flat(flat, offs, 1.0)
    assert st.n_no_path == len(bad) and np.nonzero(st.no_path)[0].tolist() == bad
    assert np.all(np.isneginf(st.logz[bad])) and np.all(np.isnan(st.expected_score[bad])) and np.all(np.isnan(st.expected_tokens[bad]))
    good = [i for i in range(len(texts)) if i not in bad]
    alone = nat.lattice_stats_flat(*tgx.pack([texts[i] for i in good]), 1.0)
    for x, y in ((st.logz, alone.logz), (st.expected_score, alone.expected_score), (st.expected_tokens, alone.expected_tokens)):
        assert np.array_equal(np.asarray(x)[good].view(np.uint64), np.asarray(y).view(np.uint64))
    assert alone.n_no_path == 0
    # the failure is not kept: the texts that have a path, on the same model
    util.assert_same_encoding(nat, ora, *tgx.pack(c["texts"]))
    empty = [i for i, t in enumerate(c["texts"]) if not t]
    ids, oo = _rows(nat.encode_batch_flat(*tgx.pack(c["texts"])))
    assert all(oo[i] == oo[i + 1] for i in empty) and len(empty) >= 1


def test_minus_inf_child_refuses_what_a_built_model_refuses():
    """A child with a score at -inf: sampling and the statistics need finite scores (ERR_UNSUPPORTED, as for a model built
    from such a vocabulary: tests/test_stats_gpu.py), and the refusal leaves the model able to encode."""
    c = dc.case("scores_minus_inf")
    nat = _child("scores_minus_inf")
    flat, offs = tgx.pack(c["texts"])
    for call in (lambda: nat.encode_batch_sample_flat(flat, offs, 1.0, 1), lambda: nat.lattice_stats_flat(flat, offs, 1.0)):
        with pytest.raises(tgx.TokenGeeXError) as e:
            call()
        assert e.value.status == _lib.ERR_UNSUPPORTED
    util.assert_same_encoding(nat, dc.oracle("scores_minus_inf"), flat, offs)
    assert set(nat.last_kernel_times()) & ENCODE_KERNELS == {"encode_kernel"}


# ---- the integer passes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SMALL_CASES)
def test_counts(name):
    c = dc.case(name)
    nat, ora = _child(name), dc.oracle(name)
    flat, offs = dc.count_corpus(name)
    corpus = tgx.NativeCorpus(flat, offs)
    np.testing.assert_array_equal(nat.count_tokens(corpus), ora.count_tokens_flat(flat, offs, threads=8))
    assert set(nat.last_kernel_times()) & ENCODE_KERNELS, nat.last_kernel_times()
    wk, wc = ora.count_pairs_flat(flat, offs, threads=8)
    keys, counts = nat.count_pairs(corpus)
    np.testing.assert_array_equal(keys, wk)
    np.testing.assert_array_equal(counts, wc)
    order = np.lexsort((wk, -wc.astype(np.int64)))
    for k in (1, 16, wk.size + 10):
        tk, tc, total = nat.count_pairs_top(corpus, k)
        assert total == wk.size and tk.size == min(k, wk.size), (name, k)
        np.testing.assert_array_equal(tk, wk[order[:tk.size]])
        np.testing.assert_array_equal(tc, wc[order[:tk.size]])
    if name in dc.FULL_COVER:
        assert wk.size > 100 and int(ora.count_tokens_flat(flat, offs, threads=8).sum()) > 10000


@pytest.mark.parametrize("for_estep", [False, True])
@pytest.mark.parametrize("name", [n for n in dc.SMALL_CASES if n != "keep_none"])
def test_prune_alternatives(name, for_estep):
    got = _child(name, for_estep).prune_alternatives()
    want = orc.prune_alternatives(dc.oracle(name))
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_common_prefix_search_on_every_suffix():
    for name in ("prefix_holes", "dead_subtrees", "len64_to_4", "chain3", "byte_dropped", "keep_none"):
        c = dc.case(name)
        nat, ora = _child(name), dc.oracle(name)
        texts = [t for t in c["texts"] + c["bad_texts"] if t][-3:]
        assert len(texts) >= 2
        for t in texts:
            for p in range(len(t) + 1):
                assert nat.common_prefix_search(t[p:p + 96]) == ora.common_prefix_search(t[p:p + 96]), (name, p)


# ---- the E-step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("for_estep", [True, False])
@pytest.mark.parametrize("name", dc.ESTEP_CASES)
def test_estep(name, for_estep):
    nat, ora = _child(name, for_estep), dc.oracle(name)
    flat, offs = dc.count_corpus(name)
    corpus = tgx.NativeCorpus(flat, offs)
    family, kernel = dc.estep_kernels(name)
    for dropout, seed in ((0.0, 0), (0.05, 3)):
        got, gz = nat.estep(corpus, 81920, dropout, seed)
        kernels = nat.last_kernel_times()
        assert kernel in kernels and util.estep_family(kernels) == family, (name, dropout, sorted(kernels))
        if family == "linear":
            assert not set(kernels) & set(util.LOG_ESTEP), (name, sorted(kernels))
        st, want, wz, _ = ora.estep_flat(flat, offs, 81920, dropout, seed, threads=8)
        assert st == orc.OK and np.array_equal(got != 0, want != 0)
        util.assert_estep_truth(got, gz, kernels, ora, flat, offs, 81920, dropout, seed, want, wz)


FORCED_ESTEP_CASES = ("prefix_holes", "dead_subtrees", "len16_to_le8", "len32_to_16", "len33_to_32", "len64_to_16", "len64_to_4",
                      "empty_token_parent", "chain3", "m_step_real")


@pytest.mark.parametrize("force", ["chain", "log", "fused", "pieces"])
@pytest.mark.parametrize("for_estep", [True, False])
@pytest.mark.parametrize("name", FORCED_ESTEP_CASES)
def test_estep_on_the_older_kernels_and_on_pieces(name, for_estep, force, monkeypatch):
    """The kernels a plain call no longer reaches for these children, forced as tests/test_estep_pairs_gpu.py forces them:
    the chained linear-domain kernels (TGX_ESTEP=chain; with for_estep and a parent of longer tokens they walk the
    DERIVED reversed table), the log-domain ones (TGX_ESTEP=log), the generic one (TGX_PATH=fused), and the default
    kernels over pieces cut by cut_windows_kernel (TGX_ESTEP_PIECES=1 at a window of 256 bytes)."""
    c = dc.case(name)
    nat, ora = _child(name, for_estep), dc.oracle(name)
    flat, offs = dc.count_corpus(name)
    corpus = tgx.NativeCorpus(flat, offs)
    short = dc.child_lm(c) <= 16
    if force == "chain":
        monkeypatch.setenv("TGX_ESTEP", "chain")
        family, any_of = "linear", {"estep4l_fwd_kernel", "estep5_fwd_kernel"}
    elif force == "log":
        monkeypatch.setenv("TGX_ESTEP", "log")
        family, any_of = "log", {"estep4_fwd_kernel"} if short else {"estep_kernel"}
    elif force == "fused":
        monkeypatch.setenv("TGX_PATH", "fused")
        family, any_of = "log", {"estep_kernel"}
    else:
        monkeypatch.setenv("TGX_ESTEP_PIECES", "1")
        monkeypatch.setenv("TGX_ESTEP_WINDOW", "256")
        family, any_of = "linear", {dc.estep_kernels(name)[1]}
    for dropout, seed in ((0.0, 0), (0.05, 3)):
        got, gz = nat.estep(corpus, 81920, dropout, seed)
        kernels = nat.last_kernel_times()
        assert set(kernels) & any_of and util.estep_family(kernels) == family, (name, force, dropout, sorted(kernels))
        if force != "pieces":
            assert "estep7_kernel" not in kernels, (name, force, sorted(kernels))
        else:
            assert nat.last_estep_pieces() > offs.size - 1, (name, nat.last_estep_pieces())
        st, want, wz, _ = ora.estep_flat(flat, offs, 81920, dropout, seed, threads=8)
        assert st == orc.OK and np.array_equal(got != 0, want != 0)
        util.assert_estep_truth(got, gz, kernels, ora, flat, offs, 81920, dropout, seed, want, wz)


# ---- sampling, n-best, statistics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SAMPLING_CASES)
def test_sampling(name):
    s = dc.sampling(name)
    nat = _child(name)
    flat, offs = tgx.pack(s["texts"])
    res, z = nat.encode_corpus_sample(tgx.NativeCorpus(flat, offs), s["alpha"], s["seed"], return_logz=True)
    ran = set(nat.last_kernel_times()) & SAMPLE_KERNELS
    ids, oo = _rows(res)
    assert ran == SAMPLE_RAN[s["expect"]], (name, ran)
    wrote = "sample_rows_kernel" if s["expect"] == "rows" else "sample_kernel"
    for i, (w, t, truth) in enumerate(zip(s["checked"], s["texts"], s["truth"])):
        assert ids[int(oo[i]):int(oo[i + 1])].tolist() == w["ids"], (name, i, len(t), w["gap"])
        bound = hc.logz_bound(wrote, len(t), truth)
        assert abs(z[i] - truth) <= bound, (name, i, len(t), z[i], truth, abs(z[i] - truth), bound)
    res2, z2 = nat.encode_batch_sample_flat(flat, offs, s["alpha"], s["seed"], return_logz=True)
    ids2, oo2 = _rows(res2)
    assert np.array_equal(ids2, ids) and np.array_equal(oo2, oo) and np.array_equal(np.asarray(z2).view(np.uint64), np.asarray(z).view(np.uint64))


@pytest.mark.parametrize("name", dc.FULL_COVER)
def test_nbest(name):
    c = dc.case(name)
    nat = _child(name)
    toks, scores = dc.child(c)
    want = dc.nbest(name)
    flat, offs = tgx.pack(c["texts"])
    enc_ids, enc_oo = _rows(nat.encode_batch_flat(flat, offs))
    for k in dc.NBEST_KS:
        res, sc_, nf = nat.encode_batch_nbest_flat(flat, offs, k)
        assert "nbest_kernel" in nat.last_kernel_times() and "nbest_trace_kernel" in nat.last_kernel_times()
        assert res.num_samples == len(c["texts"]) * k
        ids, oo = _rows(res)
        rows = [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]
        for i, (wr, ws) in enumerate(want):
            assert nf[i] == min(k, len(wr)), (name, k, i)
            for r in range(k):
                if r < nf[i]:
                    assert rows[i * k + r] == wr[r], (name, k, i, r)
                    assert sc_[i * k + r] == ws[r], (name, k, i, r, sc_[i * k + r], ws[r])
                    assert b"".join(toks[t] for t in rows[i * k + r]) == c["texts"][i]
                else:
                    assert rows[i * k + r] == [] and sc_[i * k + r] == -np.inf
            assert rows[i * k] == enc_ids[int(enc_oo[i]):int(enc_oo[i + 1])].tolist(), (name, k, i)


@pytest.mark.parametrize("alpha", dc.STATS_ALPHAS)
@pytest.mark.parametrize("name", dc.SAMPLING_CASES)
def test_lattice_stats(name, alpha):
    """The bounds of tests/test_stats_gpu.py: log Z as sampling's; expected score and tokens within 1e-10 max(1, |truth|)
    on stats_rows_kernel and within stats_cases.twin_bound on stats_kernel (the cases are not on its shared list); the
    entropy within (bound on log Z) + alpha (bound on the expected score)."""
    c = dc.case(name)
    nat = _child(name)
    z, es, et, n = dc.stats_truth(name, alpha)
    expect = dc.stats_expect(name, alpha)
    rows = expect == "rows"  # (after a fallback the generic kernel wrote the results)
    st = nat.lattice_stats_flat(*tgx.pack(c["texts"]), alpha)
    ran = set(nat.last_kernel_times()) & STATS_KERNELS
    assert ran == STATS_RAN[expect], (name, alpha, ran)
    assert st.n_no_path == 0 and not st.no_path.any() and np.array_equal(st.n_bytes, n)
    zb = sx.logz_bound(rows, n, z)
    eb = sx.ROWS_RTOL * np.maximum(1.0, np.abs(es)) if rows else sx.twin_bound(n, z, es)
    tb = sx.ROWS_RTOL * np.maximum(1.0, np.abs(et)) if rows else sx.twin_bound(n, z, et)
    dz, de, dt = np.abs(st.logz - z), np.abs(st.expected_score - es), np.abs(st.expected_tokens - et)
    dh = np.abs(st.entropy - (z - alpha * es))
    print(f"[derived stats] {name} alpha {alpha} {'rows' if rows else 'generic'}: logz err/bound {float((dz / zb).max()):.3g}, "
          f"escore dist {sx.distance(st.expected_score, es):.3g}, etokens dist {sx.distance(st.expected_tokens, et):.3g}")
    assert np.all(dz <= zb), (name, int(np.argmax(dz / zb)), dz.max())
    assert np.all(de <= eb), (name, int(np.argmax(de / eb)), de.max())
    assert np.all(dt <= tb), (name, int(np.argmax(dt / tb)), dt.max())
    assert np.all(dh <= zb + alpha * eb), (name, int(np.argmax(dh)), dh.max())


# ---- decode and spans -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in dc.SMALL_CASES if n != "keep_none"])
def test_decode_and_spans_use_the_childs_bytes(name):
    c = dc.case(name)
    nat = _child(name)
    toks, _ = dc.child(c)
    flat, offs = tgx.pack(c["texts"])
    res = nat.encode_batch_flat(flat, offs)
    ids, oo = res.ids().copy(), res.offsets().copy()
    rows = [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]
    want_bytes, want_offs, want_replaced = dk.decode_rows(rows, toks, [], True)
    text = nat.decode_result(res, *NO_SPECIALS, True)
    assert np.array_equal(text.bytes(), want_bytes) and np.array_equal(text.offsets(), want_offs) and text.num_replaced == want_replaced
    if flat.size and int(flat.max()) < 0x80:  # ASCII texts are valid UTF-8: the decoded text is the input
        assert np.array_equal(text.bytes(), flat) and want_replaced == 0
    for unit in ("byte", "char"):
        got = tensors.to_spans(res, nat, unit=unit).cpu().numpy()
        assert np.array_equal(got, sp.flat(ids, oo, sp.vocab_lookup(toks), unit)), (name, unit)
    res.free()


# ---- the identity, the parent, threads, the large parent ----------------------------------------------------------------------
def test_identity_derivation_is_the_parent_bit_for_bit():
    c = dc.case("keep_all_same_scores")
    parent, nat = tgx.NativeModel(c["toks"], c["scores"]), _child("keep_all_same_scores")
    flat, offs = tgx.pack(c["texts"])
    s = dc.sampling("keep_all_same_scores")
    for dropout, seed in ((0.0, 0), (0.1, 5)):
        a, b = _rows(parent.encode_batch_flat(flat, offs, dropout, seed)), _rows(nat.encode_batch_flat(flat, offs, dropout, seed))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    cf, co = dc.count_corpus("keep_all_same_scores")
    corpus = tgx.NativeCorpus(cf, co)
    assert np.array_equal(parent.count_tokens(corpus), nat.count_tokens(corpus))
    for x, y in zip(parent.count_pairs(corpus), nat.count_pairs(corpus)):
        assert np.array_equal(x, y)
    (ra, za), (rb, zb) = (m.encode_batch_sample_flat(flat, offs, 1.0, s["seed"], return_logz=True) for m in (parent, nat))
    a, b = _rows(ra), _rows(rb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(za).view(np.uint64), np.asarray(zb).view(np.uint64))
    (ra, sa, na), (rb, sb, nb) = (m.encode_batch_nbest_flat(flat, offs, 4) for m in (parent, nat))
    a, b = _rows(ra), _rows(rb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(na, nb)
    sa, sb = parent.lattice_stats_flat(flat, offs, 0.3), nat.lattice_stats_flat(flat, offs, 0.3)
    for x, y in ((sa.logz, sb.logz), (sa.expected_score, sb.expected_score), (sa.expected_tokens, sb.expected_tokens)):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    for x, y in zip(parent.prune_alternatives(), nat.prune_alternatives()):
        assert np.array_equal(x, y)
    parent.free()


def test_derivation_does_not_write_through_to_the_parent():
    """Encode and E-step of a parent that stays alive, before and after five children were derived from it, run and freed."""
    names = ("prefix_holes", "dead_subtrees", "keep_all_new_scores", "keep_one", "keep_none")
    c = dc.case(names[0])
    assert all(dc.case(n)["toks"] is not None and dc.case(n)["toks"] == c["toks"] for n in names)
    parent, ora = tgx.NativeModel(c["toks"], c["scores"], for_estep=True), dc.parent_oracle(names[0])
    flat, offs = tgx.pack(c["texts"])
    corpus = tgx.NativeCorpus(flat, offs)

    def check():
        util.assert_same_encoding(parent, ora, flat, offs)
        got, gz = parent.estep(corpus, 81920, 0.0, 0)
        assert "estep7_kernel" in parent.last_kernel_times()
        util.assert_estep_truth(got, gz, parent.last_kernel_times(), ora, flat, offs, 81920, 0.0, 0)
        assert parent.common_prefix_search(c["texts"][-4]) == ora.common_prefix_search(c["texts"][-4])

    check()
    for for_estep in (True, False):
        for n in names:
            keep, cs = dc.case(n)["links"][0]
            d = parent.derive(keep, cs, for_estep=for_estep)
            good = dc.case(n)["texts"]
            util.assert_same_encoding(d, dc.oracle(n), *tgx.pack(good))
            d.free()
        check()
    parent.free()


def test_two_threads_derive_while_a_third_encodes():
    """The parent's lock (tgx_model_create_derived takes it for the copy): two host threads derive from one parent, each
    several times, while a third encodes with it; every result is the oracle's."""
    names = ("prefix_holes", "dead_subtrees")
    c = dc.case(names[0])
    parent, ora = tgx.NativeModel(c["toks"], c["scores"], for_estep=True), dc.parent_oracle(names[0])
    flat, offs = tgx.pack(c["texts"])
    want = {n: dc.oracle(n).encode_batch_flat(*tgx.pack(dc.case(n)["texts"])) for n in names}
    want_parent = ora.encode_batch_flat(flat, offs)
    errors, done = [], threading.Event()

    def deriver(n, for_estep):
        try:
            keep, cs = dc.case(n)["links"][0]
            for _ in range(4):
                d = parent.derive(keep, cs, for_estep=for_estep)
                ids, oo = _rows(d.encode_batch_flat(*tgx.pack(dc.case(n)["texts"])))
                d.free()
                if not (np.array_equal(ids, want[n][0]) and np.array_equal(oo, want[n][1])):
                    errors.append(f"{n}: the child's ids differ from the oracle's")
        except Exception as exc:  # noqa: BLE001 (reported on the main thread)
            errors.append(f"{n}: {exc!r}")

    def encoder():
        try:
            rounds = 0
            while rounds < 4 or (not done.is_set() and rounds < 200):
                ids, oo = _rows(parent.encode_batch_flat(flat, offs))
                rounds += 1
                if not (np.array_equal(ids, want_parent[0]) and np.array_equal(oo, want_parent[1])):
                    errors.append("the parent's ids differ from the oracle's")
                    return
        except Exception as exc:  # noqa: BLE001
            errors.append(f"parent: {exc!r}")

    threads = [threading.Thread(target=deriver, args=(names[0], True)), threading.Thread(target=deriver, args=(names[1], False))]
    enc = threading.Thread(target=encoder)
    for t in threads + [enc]:
        t.start()
    for t in threads:
        t.join()
    done.set()
    enc.join()
    parent.free()
    assert not errors, errors


@functools.lru_cache(maxsize=None)
def _big_parent(for_estep: bool):
    c = dc.case("big_parent_40")
    return tgx.NativeModel(c["toks"], c["scores"], for_estep=for_estep)


def test_big_parent():
    """The committed 500 000-entry vocabulary.  A parent table above the 8-byte records' limit refuses a child for encode
    of at most half its size (the caller builds that one from scratch); every other child is accepted and is the
    oracle's on encode, the token counts, n-best and, derived for the E-step, the E-step."""
    c40, c60 = dc.case("big_parent_40"), dc.case("big_parent_60")
    parent = _big_parent(False)
    assert parent.trie_bytes == c40["n_slots"] * 16
    keep40, s40 = c40["links"][0]
    if c40["above_trie8"]:
        with pytest.raises(tgx.TokenGeeXError) as e:
            parent.derive(keep40, s40)
        assert e.value.status == _lib.ERR_UNSUPPORTED
        legs = [("big_parent_60", False), ("big_parent_40", True), ("big_parent_60", True)]
    else:
        legs = [("big_parent_40", False), ("big_parent_60", False), ("big_parent_40", True), ("big_parent_60", True)]
    for name, for_estep in legs:
        c = dc.case(name)
        keep, cs = c["links"][0]
        d = parent.derive(keep, cs, for_estep=for_estep)
        ora = dc.oracle(name)
        flat, offs = tgx.pack(c["texts"])
        util.assert_same_encoding(d, ora, flat, offs)
        assert set(d.last_kernel_times()) & ENCODE_KERNELS, d.last_kernel_times()
        ids, _ = _rows(d.encode_batch_flat(flat, offs))
        corpus = tgx.NativeCorpus(flat, offs)
        np.testing.assert_array_equal(d.count_tokens(corpus), ora.count_tokens_flat(flat, offs, threads=8))
        if for_estep:
            got, gz = d.estep(corpus, 81920, 0.0, 0)
            kernels = d.last_kernel_times()
            st, want, wz, _ = ora.estep_flat(flat, offs, 81920, 0.0, 0, threads=8)
            assert st == orc.OK and np.array_equal(got != 0, want != 0)
            assert util.assert_estep_truth(got, gz, kernels, ora, flat, offs, 81920, 0.0, 0, want, wz) == "linear"
        else:
            want = dc.nbest(name)
            res, sc_, nf = d.encode_batch_nbest_flat(flat, offs, 4)
            nids, noo = _rows(res)
            for i, (wr, ws) in enumerate(want):
                for r in range(min(4, len(wr))):
                    assert nids[int(noo[i * 4 + r]):int(noo[i * 4 + r + 1])].tolist() == wr[r] and sc_[i * 4 + r] == ws[r], (name, i, r)
            assert int(ids.max()) >= 1 << 16
        d.free()
