"""Sampling, n-best and the lattice statistics on the GPU over the randomised cases of tests/lattice_fuzz_cases.py (cases
0 .. N_CASES - 1 of seed SEED0, established on the CPU by tests/test_lattice_fuzz_cpu.py), in blocks of 8 cases per test.

Per case: the three switches are cleared and the case's own set, the model is built (derived from its parent where drawn, the
parent freed), and the three passes run in the drawn order on that one handle, each in its drawn form (batch or resident
corpus).  Then, with no sample excused:
  * the kernels that ran are the ones the selection rules of csrc/lattice_pass.cpp give for the case;
  * sampling: the checker's ids for every sample at the case's seed; log Z within hostile_cases.logz_bound of the 80-bit
    truth, by the kernel that wrote it;
  * n-best: ids, scores and n_found exactly the checker's; at k = 1 row 0 is encode's; a call that the 1 MiB budget cuts
    runs nbest_kernel once per chunk;
  * statistics: log Z, expected score, expected tokens and entropy within lattice_fuzz_cases.stats_bounds of the truth
    (ROWS_RTOL on stats_rows_kernel, stats_cases.twin_bound on stats_kernel); its log Z is sampling's bit for bit where the
    same kind of kernel wrote both;
  * a sample without a path: sampling and n-best raise encode's error (the lowest such sample), statistics marks it and
    holds the other samples to their bounds.

N_CASES = 160: the largest multiple of 8 whose reference side (the cases and their expectations, built once per process and
shared by the blocks) stays under about a minute on the CPU machine of this change, 45.9 s (168 cases: 56.9 s, and
tests/test_lattice_fuzz_cpu.py over a minute).  On an MI355X, measured with the first 168 cases: 19.9 s for the module, the
slowest block of 8 cases 2.3 s, reference side included (that machine builds it in 14 s); the device side of all the cases
together, models built and results compared, 2.0 s.  With the 160 cases, inside the whole suite: the slowest block 2.7 s."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import hostile_cases as hc
import lattice_fuzz_cases as lf

BLOCK = 8
SAMPLE_KERNELS = set().union(*lf.SAMPLE_RAN.values()) | {"trace32_kernel"}
STATS_KERNELS = set().union(*lf.STATS_RAN.values())


def _ran(native):
    """The names of the last call's kernels, in launch order (the library keeps the first 8)."""
    names = (_lib.C.c_char_p * 8)()
    n = _lib.lib.tgx_last_kernel_times(native._h, names, None, 8)
    return [names[i].decode() for i in range(n)]


def build_model(c):
    if c["parent"] is None:
        return tgx.NativeModel(c["toks"], c["scores"])
    parent = tgx.NativeModel(c["parent"]["toks"], c["parent"]["scores"])
    child = parent.derive(c["parent"]["keep"], c["scores"])
    parent.free()
    return child


def _rows_of(res):
    ids, oo = res.ids().copy(), res.offsets().copy()
    res.free()
    return [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]


def _encode_error(native, c):
    """encode's error on the case's batch, or None"""
    try:
        native.encode_batch_flat(c["flat"], c["offs"]).free()
    except tgx.TokenGeeXError as ex:
        return ex
    return None


def _same_error(got, want, c, what):
    assert want is not None and got.status == want.status == _lib.ERR_NO_PATH, (what, lf.tag(c))
    assert str(got) == str(want) and (got.sample, got.pos, got.length) == (want.sample, want.pos, want.length), (what, lf.tag(c), str(got), str(want))
    assert got.sample == c["no_path"][0], (what, lf.tag(c), got.sample)


def run_sample(native, c, ratios):
    """-> (the kind of kernel that wrote log Z, log Z) or None where the call raised encode's error"""
    corpus = tgx.NativeCorpus(c["flat"], c["offs"]) if c["forms"]["sample"] else None
    try:
        if corpus is not None:
            res, z = native.encode_corpus_sample(corpus, c["alpha"], c["seed"], return_logz=True)
        else:
            res, z = native.encode_batch_sample_flat(c["flat"], c["offs"], c["alpha"], c["seed"], return_logz=True)
        err = None
    except tgx.TokenGeeXError as ex:
        err = ex
    ran = set(_ran(native)) & SAMPLE_KERNELS
    assert ran == lf.SAMPLE_RAN[c["expect"]["sample"]], ("sampling kernels", lf.tag(c), ran)
    if c["no_path"]:
        assert err is not None, ("sampling: no error", lf.tag(c))
        _same_error(err, _encode_error(native, c), c, "sampling")
        return None
    assert err is None, ("sampling", lf.tag(c), str(err))
    rows, z = _rows_of(res), np.array(z)
    wrote = "sample_rows_kernel" if c["expect"]["sample"] == "rows" else "sample_kernel"
    assert len(rows) == len(c["texts"]) == z.size, ("sampling rows", lf.tag(c))
    for j, (w, n) in enumerate(zip(c["checked"], c["lens"])):
        assert rows[j] == w["ids"], ("sampling ids", lf.tag(c), j, n, w["gap"])
        bound = hc.logz_bound(wrote, n, c["z"][j])
        ratios[wrote] = max(ratios.get(wrote, 0.0), abs(z[j] - c["z"][j]) / bound)
        assert abs(z[j] - c["z"][j]) <= bound, ("sampling log Z", lf.tag(c), j, n, z[j], c["z"][j], bound)
    return wrote, z


def run_nbest(native, c, ratios):
    k = c["k"]
    corpus = tgx.NativeCorpus(c["flat"], c["offs"]) if c["forms"]["nbest"] else None
    try:
        res, scores, nf = native.encode_corpus_nbest(corpus, k) if corpus is not None else native.encode_batch_nbest_flat(c["flat"], c["offs"], k)
        err = None
    except tgx.TokenGeeXError as ex:
        err = ex
    ran = _ran(native)
    if c["no_path"]:
        assert err is not None, ("n-best: no error", lf.tag(c))
        assert set(lf.NBEST_CHUNK_KERNELS[:3]) <= set(ran) <= set(lf.NBEST_CHUNK_KERNELS), ("n-best kernels", lf.tag(c), ran)
        _same_error(err, _encode_error(native, c), c, "n-best")
        return
    assert err is None, ("n-best", lf.tag(c), str(err))
    # one nbest_kernel per chunk, four timed kernels per chunk, the first 8 kept
    assert ran == list(lf.NBEST_CHUNK_KERNELS) * min(c["chunks"], 2), ("n-best kernels", lf.tag(c), ran)
    assert res.num_samples == len(c["texts"]) * k
    rows = _rows_of(res)
    for j, (wr, ws) in enumerate(c["nbest"]):
        assert nf[j] == min(k, len(wr)), ("n-best n_found", lf.tag(c), j, int(nf[j]), len(wr))
        for r in range(k):
            if r < nf[j]:
                assert rows[j * k + r] == wr[r], ("n-best ids", lf.tag(c), j, r)
                assert scores[j * k + r] == ws[r], ("n-best score", lf.tag(c), j, r, scores[j * k + r], ws[r])
            else:
                assert rows[j * k + r] == [] and scores[j * k + r] == -math.inf, ("n-best past n_found", lf.tag(c), j, r)
    if k == 1:
        enc = _rows_of(native.encode_batch_flat(c["flat"], c["offs"]))
        assert enc == rows, ("n-best at k = 1 is not encode", lf.tag(c))


def run_stats(native, c, ratios):
    """-> (the kind of kernel that wrote log Z, log Z)"""
    corpus = tgx.NativeCorpus(c["flat"], c["offs"]) if c["forms"]["stats"] else None
    st = native.lattice_stats_corpus(corpus, c["alpha"]) if corpus is not None else native.lattice_stats_flat(c["flat"], c["offs"], c["alpha"])
    ran = set(_ran(native)) & STATS_KERNELS
    if len(c["texts"]) or corpus is not None:  # (lattice_stats_flat has nothing to upload at S = 0 and makes no call)
        assert ran == lf.STATS_RAN[c["expect"]["stats"]], ("statistics kernels", lf.tag(c), ran)
    rows = c["expect"]["stats"] == "rows"
    wrote = "stats_rows_kernel" if rows else "stats_kernel"
    assert len(st) == len(c["texts"]) and st.n_no_path == len(c["no_path"]), ("statistics no_path", lf.tag(c), st.n_no_path)
    assert np.nonzero(st.no_path)[0].tolist() == c["no_path"], ("statistics no_path", lf.tag(c))
    assert np.array_equal(st.n_bytes, c["lens"])
    ok = np.array([j not in c["no_path"] for j in range(len(c["texts"]))], bool)
    if not ok.all():
        assert np.all(np.isneginf(st.logz[~ok])) and np.all(np.isnan(st.expected_score[~ok])) and np.all(np.isnan(st.expected_tokens[~ok])) \
            and np.all(np.isnan(st.entropy[~ok])), ("statistics of a sample without a path", lf.tag(c))
    if ok.any():
        n, z, es, et = np.array(c["lens"], np.float64)[ok], c["z"][ok], c["es"][ok], c["et"][ok]
        zb, eb, tb, hb = lf.stats_bounds(rows, n, z, es, et, c["alpha"])
        errs = {"logz": (np.abs(st.logz[ok] - z), zb), "escore": (np.abs(st.expected_score[ok] - es), eb),
                "etokens": (np.abs(st.expected_tokens[ok] - et), tb), "entropy": (np.abs(st.entropy[ok] - (z - c["alpha"] * es)), hb)}
        for what, (d, b) in errs.items():
            key = f"{wrote} {what}"
            ratios[key] = max(ratios.get(key, 0.0), float((d / b).max()))
            at = int(np.argmax(d / b))
            assert np.all(d <= b), ("statistics " + what, lf.tag(c), wrote, int(np.nonzero(ok)[0][at]), float(d[at]), float(b[at]))
    return wrote, np.asarray(st.logz)


def run_case(c, ratios=None):
    """One case on the device; raises AssertionError with the case's tag on a mismatch.  `ratios` collects the largest
    error-to-bound ratio per kernel and quantity."""
    ratios = {} if ratios is None else ratios
    assert c["seed"] is not None, lf.tag(c)
    for name in lf.SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(c["env"])
    native = build_model(c)
    try:
        wrote = {}
        for p in c["order"]:
            wrote[p] = {"sample": run_sample, "nbest": run_nbest, "stats": run_stats}[p](native, c, ratios)
        if wrote["sample"] is not None and len(c["texts"]):
            # test_stats_gpu.py::test_logz_is_sampling_logz_bit_for_bit: rows with rows, generic with generic
            (ks, zs), (kt, zt) = wrote["sample"], wrote["stats"]
            if (ks == "sample_rows_kernel") == (kt == "stats_rows_kernel"):
                assert np.array_equal(zs.view(np.uint64), zt.view(np.uint64)), ("log Z of statistics is not sampling's", lf.tag(c), ks, kt)
    except AssertionError:
        print("MISMATCH", lf.tag(c), flush=True)  # (pytest shortens the assertion's own message)
        raise
    finally:
        native.free()
        for name in lf.SWITCHES:
            os.environ.pop(name, None)
    return ratios


@pytest.mark.parametrize("block", range(lf.N_CASES // BLOCK))
def test_cases(block):
    ratios = {}
    for i in range(block * BLOCK, (block + 1) * BLOCK):
        run_case(lf.case(lf.SEED0, i), ratios)
    print(f"[lattice fuzz] cases {block * BLOCK}..{(block + 1) * BLOCK - 1}: largest error-to-bound ratios",
          {k: f"{v:.3g}" for k, v in sorted(ratios.items())})
