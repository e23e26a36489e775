"""The host twin of the lattice statistics (tgx_lattice_stats_host) without a device: against a brute-force sum over every
segmentation, against the 80-bit truth on the shared case list (tests/stats_cases.py), against the f64 oracle's log Z,
and its argument errors."""
import math

import numpy as np
import pytest

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib

import stats_cases as sx


def _twin(toks, scores, texts, alpha):
    flat, offs = tgx.pack(texts)
    return _lib.lattice_stats_host(toks, scores, flat, offs, alpha)


def _close(got, want, what):
    # texts of at most 12 bytes: a few dozen f64 operations on either side, each within a few ulp of values of the result's
    # size; 1e-12 max(1, |want|) is several thousand ulp
    if math.isnan(want):
        assert math.isnan(got), what
    elif math.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (what, got, want)


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0, 4.0])
@pytest.mark.parametrize("case", sorted(sx.brute_cases()))
def test_twin_matches_the_sum_over_all_segmentations(case, alpha):
    toks, scores, texts = sx.brute_cases()[case]
    st = _twin(toks, scores, texts, alpha)
    assert len(st) == len(texts) and st.alpha == alpha
    assert np.array_equal(st.n_bytes, [len(t) for t in texts])
    bad = 0
    for i, t in enumerate(texts):
        z, es, et, h = sx.brute(toks, scores, t, alpha)
        _close(st.logz[i], z, (case, t, "logz"))
        _close(st.expected_score[i], es, (case, t, "escore"))
        _close(st.expected_tokens[i], et, (case, t, "etokens"))
        _close(st.entropy[i], h, (case, t, "entropy"))
        bad += z == sx.NINF
        assert bool(st.no_path[i]) == (z == sx.NINF)
        if len(t) and z != sx.NINF:
            _close(st.bits_per_byte[i], -z / (len(t) * math.log(2.0)), (case, t, "bits per byte"))
    assert st.n_no_path == bad
    if case == "partial_cover":
        assert bad == 2  # b"abcb" and b"b": the call is TGX_OK all the same


def test_alpha_zero_counts_the_segmentations():
    toks, scores = sx.tiny()
    st = _twin(toks, scores, [b"abcabca", b""], 0.0)
    inc = sx.matches(toks, scores, b"abcabca")
    paths = {0: 1}
    for p in range(1, 8):
        paths[p] = sum(paths.get(q, 0) for q, _ in inc[p])
    n_seg = paths[7]
    assert n_seg > 1
    assert abs(st.logz[0] - math.log(n_seg)) <= 1e-14 and abs(st.entropy[0] - math.log(n_seg)) <= 1e-14
    assert (st.logz[1], st.expected_score[1], st.expected_tokens[1]) == (0.0, 0.0, 0.0)


def test_a_later_duplicate_overrides_an_earlier_one():
    toks, scores = [b"a", b"b", b"ab", b"ab"], np.array([-1.0, -1.0, -5.0, -0.5])
    a = _twin(toks, scores, [b"ab"], 1.0)
    b = _twin([b"a", b"b", b"ab"], np.array([-1.0, -1.0, -0.5]), [b"ab"], 1.0)
    assert (a.logz[0], a.expected_score[0], a.expected_tokens[0]) == (b.logz[0], b.expected_score[0], b.expected_tokens[0])


@pytest.mark.parametrize("name,alpha", sx.TWIN_RUNS)
def test_twin_against_the_truth(name, alpha):
    toks, scores = sx.vocab(name)
    st = _twin(toks, scores, sx.texts(), alpha)
    z, es, et = sx.truth(name, alpha)
    n = sx.lens()
    assert st.n_no_path == 0
    assert np.all(np.abs(st.logz - z) <= sx.logz_bound(False, n, z)), np.abs(st.logz - z).max()
    assert np.all(np.abs(st.expected_score - es) <= sx.twin_bound(n, z, es))
    assert np.all(np.abs(st.expected_tokens - et) <= sx.twin_bound(n, z, et))
    ent = z - alpha * es
    assert np.all(np.abs(st.entropy - ent) <= sx.logz_bound(False, n, z) + alpha * sx.twin_bound(n, z, es))
    assert (st.logz[0], st.expected_score[0], st.expected_tokens[0]) == (0.0, 0.0, 0.0)  # the empty sample


def test_twin_distance_is_what_the_gpu_bound_was_made_from(capsys):
    """stats_cases.GENERIC_*_BOUND is 4 x the twin's largest distance over TWIN_RUNS as measured when the test was written
    (escore 4.89e-14, etokens 8.78e-15, relative to max(1, |truth|)).  Another libm may move the twin by a last bit here or
    there: it must stay within the bound the device kernel is given."""
    flat, offs = tgx.pack(sx.texts())
    de = dt = 0.0
    for name, alpha in sx.TWIN_RUNS:
        toks, scores = sx.vocab(name)
        st = _lib.lattice_stats_host(toks, scores, flat, offs, alpha)
        _, es, et = sx.truth(name, alpha)
        de, dt = max(de, sx.distance(st.expected_score, es)), max(dt, sx.distance(st.expected_tokens, et))
    with capsys.disabled():
        print(f"\n[stats twin] largest distance from the 80-bit truth: escore {de:.3g}, etokens {dt:.3g}")
    assert de <= sx.GENERIC_ESCORE_BOUND and dt <= sx.GENERIC_ETOKENS_BOUND, (de, dt)


def test_twin_logz_against_the_f64_oracle():
    toks, scores = sx.vocab("vocab_32000")
    om = orc.OracleModel(toks, scores)
    st = _twin(toks, scores, sx.texts(), 1.0)
    for i, t in enumerate(sx.texts()):
        _, z = om.marginal(t)
        # two f64 log-domain sums of the same lattice: each within the log-domain bound of the truth
        assert abs(st.logz[i] - z) <= 2.0 * float(sx.logz_bound(False, len(t), z)), (i, st.logz[i], z)


def test_argument_errors():
    toks, scores = sx.tiny()
    flat, offs = tgx.pack([b"abc"])
    for alpha in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.lattice_stats_host(toks, scores, flat, offs, alpha)
        assert e.value.status == _lib.ERR_INVALID, alpha
    for bad in (float("inf"), -float("inf"), float("nan")):
        s = scores.copy()
        s[3] = bad
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.lattice_stats_host(toks, s, flat, offs, 1.0)
        assert e.value.status == _lib.ERR_UNSUPPORTED, bad
    s = scores.copy()
    s[2] = -1e308
    with pytest.raises(tgx.TokenGeeXError) as e:
        _lib.lattice_stats_host(toks, s, flat, offs, 100.0)  # alpha * score overflows
    assert e.value.status == _lib.ERR_INVALID
    assert _lib.lattice_stats_host(toks, s, flat, offs, 1.0).n_no_path == 0


def test_no_samples_and_null_outputs():
    toks, scores = sx.tiny()
    st = _twin(toks, scores, [], 1.0)
    assert len(st) == 0 and st.n_no_path == 0 and st.entropy.shape == (0,)
    vflat, voffs = tgx.pack(toks)
    flat, offs = tgx.pack([b"abc", b"x"])
    lz = np.zeros(2)
    assert _lib.lib.tgx_lattice_stats_host(_lib.ptr(vflat), _lib.ptr(voffs), _lib.ptr(scores), len(toks), _lib.ptr(flat), _lib.ptr(offs), 2, 1.0,
                                           _lib.ptr(lz), None, None, None) == 0
    assert lz[1] == sx.NINF and lz[0] == _twin(toks, scores, [b"abc"], 1.0).logz[0]
