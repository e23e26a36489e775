"""Sampling on the GPU where the usual vocabularies never go (cases: tests/hostile_cases.py, established on the CPU by
tests/test_hostile_cpu.py): the range fallback of sample_rows_kernel to sample_kernel on a designed and on a realistic
trigger and what it leaves behind, a sample without a path after a fallback, the kernel selection at 32 / 33 / 64-byte
tokens and at |alpha * score| = 207 / 207.5, and the law of the draw after a fallback.

Every expectation is sample_checker.check_sample's at a seed chosen on the CPU so that every key gap is at least 1e-6
and 100 times the log-domain rounding model: the ids must be the checker's for every sample, none excused.  log Z is
held to the 80-bit truth (oracle marginal_ext) with the bounds of tests/test_sample_gpu.py (_assert_logz_truth,
restated in hostile_cases.logz_bound): 1e-13 max(1, |z|) after sample_rows_kernel, 64 sqrt(n) 2^-52 |z| + 1e-13 after
sample_kernel.  The kernels that ran are read from last_kernel_times()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import functools

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib

import hostile_cases as hc
import sample_checker as sc

SAMPLE_KERNELS = {"sample_wslot_kernel", "sample_rows_kernel", "sample_kernel", "trace32_kernel"}
RAN = {"fallback": {"sample_wslot_kernel", "sample_rows_kernel", "sample_kernel"},
       "rows": {"sample_wslot_kernel", "sample_rows_kernel", "trace32_kernel"},
       "generic": {"sample_kernel"}}


@functools.lru_cache(maxsize=None)
def _native(vocab: str):
    """One model per vocabulary: the calls of a test and of the tests after it share it."""
    name = {"designed": "designed_trip", "real": "real_trip"}.get(vocab, vocab)
    c = hc.sampling_case(name)
    return tgx.NativeModel(c["toks"], c["scores"])


def _call(native, texts, alpha, seed, corpus=False):
    """-> (ids, offsets, logz, the sampling kernels that ran)"""
    flat, offs = tgx.pack(texts)
    if corpus:
        res, z = native.encode_corpus_sample(tgx.NativeCorpus(flat, offs), alpha, seed, return_logz=True)
    else:
        res, z = native.encode_batch_sample_flat(flat, offs, alpha, seed, return_logz=True)
    ran = set(native.last_kernel_times()) & SAMPLE_KERNELS
    ids, oo = res.ids().copy(), res.offsets().copy()
    res.free()
    return ids, oo, np.array(z), ran


def _assert_case(c, got, ran: str):
    """The kernels of `ran`, the checker's ids for every sample, log Z within the bound of the kernel that wrote it."""
    ids, oo, z, names = got
    assert names == RAN[ran], (c["name"], names)
    wrote = "sample_rows_kernel" if ran == "rows" else "sample_kernel"
    assert oo.size == len(c["texts"]) + 1
    for i, (w, t, truth) in enumerate(zip(c["checked"], c["texts"], c["truth"])):
        assert ids[int(oo[i]):int(oo[i + 1])].tolist() == w["ids"], (c["name"], i, len(t), w["gap"])
        bound = hc.logz_bound(wrote, len(t), truth)
        print(f"{c['name']} sample {i} n {len(t)} {wrote} logz {z[i]!r} truth {truth!r} err {abs(z[i] - truth):.3g} bound {bound:.3g}")
        assert abs(z[i] - truth) <= bound, (c["name"], i, len(t), z[i], truth, abs(z[i] - truth), bound)
        assert abs(z[i] - w["logz"]) <= 1e-9 * max(1.0, abs(w["logz"]))


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))  # log Z bit for bit


@pytest.mark.parametrize("vocab", ["designed", "real"])
def test_fallback(vocab, monkeypatch):
    """designed: bytes_heavy(-100) at alpha 1, the edge-length texts and 40 bytes that only byte tokens cover (144 bits
    a step).  real: the committed 32 000-entry vocabulary at alpha 5, 60 corpus samples that stay in range and one with
    64 bytes of 0x80 in its middle (42.7 bits a step).  The call runs sample_rows_kernel, then all of it again on
    sample_kernel, and no trace32_kernel; it is the generic path's result bit for bit, in the batch and the corpus form;
    the next call on the model, in range, runs the rows kernel alone."""
    trip, stay = hc.sampling_case(vocab + "_trip"), hc.sampling_case(vocab + "_stay")
    native = _native(vocab)
    got = _call(native, trip["texts"], trip["alpha"], trip["seed"])
    _assert_case(trip, got, "fallback")
    monkeypatch.setenv("TGX_SAMPLE_PATH", "generic")
    forced = _call(native, trip["texts"], trip["alpha"], trip["seed"])
    monkeypatch.delenv("TGX_SAMPLE_PATH")
    assert forced[3] == RAN["generic"]
    _same(got, forced)
    as_corpus = _call(native, trip["texts"], trip["alpha"], trip["seed"], corpus=True)
    assert as_corpus[3] == RAN["fallback"]
    _same(got, as_corpus)
    # nothing is left behind: the same model, a batch in range
    _assert_case(stay, _call(native, stay["texts"], stay["alpha"], stay["seed"]), "rows")
    _assert_case(stay, _call(native, stay["texts"], stay["alpha"], stay["seed"], corpus=True), "rows")
    # and a fallback again after it
    _same(got, _call(native, trip["texts"], trip["alpha"], trip["seed"]))


def test_control_small_alpha_stays_in_range():
    """The designed batch, poison sample included, at alpha = 0.01 (1.44 bits a step): the rows kernel alone."""
    c = hc.sampling_case("designed_control")
    _assert_case(c, _call(_native("designed"), c["texts"], c["alpha"], c["seed"]), "rows")


def test_no_path_after_a_fallback():
    """A vocabulary without 0xFF; two samples hold that byte, the shorter at the lower index (the kernels take the
    longer first).  With the poison sample the call falls back and sample_kernel reports the failure; without it the
    rows kernel and the trace do.  Either way it is encode's error."""
    c = hc.sampling_case("nopath_stay")
    native = _native("nopath_stay")
    texts = list(c["texts"])
    texts[2:2] = [hc.NOPATH_BAD[0]]
    texts += [hc.NOPATH_BAD[1]]
    bad = (2, len(hc.NOPATH_BAD[0]))
    for poison, ran in ((True, "fallback"), (False, "rows")):
        batch = texts[:9] + ([hc.POISON_DESIGNED] if poison else []) + texts[9:]
        flat, offs = tgx.pack(batch)
        with pytest.raises(tgx.TokenGeeXError) as enc:
            native.encode_batch_flat(flat, offs)
        with pytest.raises(tgx.TokenGeeXError) as smp:
            native.encode_batch_sample_flat(flat, offs, c["alpha"], c["seed"])
        assert set(native.last_kernel_times()) & SAMPLE_KERNELS == RAN[ran]
        assert smp.value.status == enc.value.status == _lib.ERR_NO_PATH
        assert str(smp.value) == str(enc.value)
        assert (smp.value.sample, smp.value.pos, smp.value.length) == (enc.value.sample, enc.value.pos, enc.value.length) \
            == (bad[0], bad[1], bad[1])
    # the failure is not kept either: the batch without the two samples, on the same model
    _assert_case(c, _call(native, c["texts"], c["alpha"], c["seed"]), "rows")


@pytest.mark.parametrize("name", ["len32", "len33", "len64", "score207", "score207_5"])
def test_kernel_selection_at_its_edges(name):
    """len32: tokens of up to 32 bytes stay on the rows kernel, and a sampled path holds a 32-byte token that starts
    inside a block of 32 (its candidate lands on the lane that restarts for the next block).  len33 / len64: lm = 36 / 64,
    the generic kernel unforced, with a token of the full length across a block of 64 on a sampled path (at 64 bytes the
    receiving lane is the finalising lane).  score207 / score207_5: the most negative alpha * score is -207.0 (rows,
    w = 2^-298.6 on the path of every text with a z) and -207.5 (generic)."""
    c = hc.sampling_case(name)
    native = _native(name)
    got = _call(native, c["texts"], c["alpha"], c["seed"])
    _assert_case(c, got, c["expect"])
    ids, oo = got[0], got[1]
    spans = [sp for i in range(len(c["texts"])) for sp in hc.path_tokens(ids[int(oo[i]):int(oo[i + 1])].tolist(), c["toks"])]
    if name == "len32":
        assert any(ln == 32 and q % 32 != 0 for q, ln in spans)
    elif name in ("len33", "len64"):
        ml = int(name[3:])
        assert max(ln for _, ln in spans) == ml and any(ln == ml and q // 64 != (q + ln) // 64 for q, ln in spans)
    else:
        assert int((ids == ord("z")).sum()) >= 10


@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_the_law_after_a_fallback(alpha):
    """N = 20 000 copies of b"abcabca" and one sample of 40 b"x" at -100 in one call that falls back: the empirical
    frequencies of the copies against segmentation_probs by test_distribution's rules (total variation < 0.02, 5 sigma
    for every segmentation of probability >= 0.01)."""
    toks, scores = hc.tiny_poisoned()
    text, N = b"abcabca", hc.LAW_N
    probs, logz = sc.segmentation_probs(sc.incoming(orc.OracleModel(toks, scores), text, 3), scores, len(text), alpha)
    native = tgx.NativeModel(toks, scores)
    ids, oo, z, ran = _call(native, [text] * N + [hc.LAW_POISON], alpha, hc.LAW_SEED)
    assert ran == RAN["fallback"]
    cnt = {}
    for i in range(N):
        row = tuple(ids[int(oo[i]):int(oo[i + 1])].tolist())
        cnt[row] = cnt.get(row, 0) + 1
    hc.assert_law(cnt, probs, N)
    assert ids[int(oo[N]):int(oo[N + 1])].tolist() == [toks.index(b"x")] * 40
    assert abs(z[N] - alpha * -4000.0) <= hc.logz_bound("sample_kernel", 40, alpha * -4000.0)
    assert np.all(np.abs(z[:N] - logz) <= hc.logz_bound("sample_kernel", len(text), logz))
