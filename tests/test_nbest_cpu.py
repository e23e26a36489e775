"""N-best segmentation without a GPU: the checker against brute-force enumeration, its row 0 against the oracle's
encode, the prefix property, the segment product and the n-best draw against their formulas, and the entry points."""
import math
import os
import random
import subprocess

import numpy as np
import pytest

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, synth
from tokengeex_amd.tokenizer import combine_nbest, nbest_draw

import nbest_checker as nc
import sample_checker as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_model():
    toks = [b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"cab"]
    scores = [-1.0, -1.5, -2.0, -1.2, -2.5, -3.0, -0.7, -2.2]
    return toks, np.array(scores), orc.OracleModel(toks, scores)


def _tied_model():
    """Quantised scores: many exact ties between segmentations."""
    toks = [b"a", b"b", b"aa", b"ab", b"ba", b"bb", b"aab", b"abb", b"aaa"]
    scores = [-1.0, -1.0, -2.0, -2.0, -1.0, -2.0, -3.0, -2.0, -3.0]
    return toks, np.array(scores), orc.OracleModel(toks, scores)


TEXTS = [b"abcab", b"abcabca", b"cabcab", b"a", b"aabbaab", b"abababba", b"bbaaab"]


@pytest.mark.parametrize("model", [_tiny_model, _tied_model])
def test_checker_against_brute_force(model):
    toks, scores, om = model()
    for text in TEXTS:
        inc = sc.incoming(om, text, max(map(len, toks)))
        want_rows, want_scores = nc.brute_force(inc, scores, len(text))
        for k in range(1, 17):
            rows, scs = nc.nbest(inc, scores, len(text), k)
            assert rows == want_rows[:k], (text, k)
            assert scs == want_scores[:k]
            assert len(rows) == min(k, len(want_rows))


@pytest.mark.parametrize("model", [_tiny_model, _tied_model])
def test_row0_is_encode_and_rows_are_valid(model):
    toks, scores, om = model()
    for text in TEXTS:
        inc = sc.incoming(om, text, max(map(len, toks)))
        rows, scs = nc.nbest(inc, scores, len(text), 16)
        if not rows:  # (a byte the model has no token for)
            assert b"c" in text
            continue
        assert rows[0] == om.encode(text)
        assert len({tuple(r) for r in rows}) == len(rows)
        assert all(a >= b for a, b in zip(scs, scs[1:]))
        for r, s in zip(rows, scs):
            assert b"".join(toks[t] for t in r) == text
            assert nc.path_score(r, scores) == s


def test_prefix_property_on_a_real_vocabulary():
    flat, offs = synth.make_corpus(64 << 10, "mixed", max_len=200, seed_offset=9)
    toks, scores = synth.build_vocab(flat, 800, 8)
    scores = np.round(np.asarray(scores, np.float64), 1)  # ties
    om = orc.OracleModel(list(toks), scores)
    for i in range(0, min(40, offs.size - 1)):
        text = bytes(flat[int(offs[i]):int(offs[i + 1])])
        inc = sc.incoming(om, text, max(map(len, toks)))
        full, fs = nc.nbest(inc, scores, len(text), 16)
        assert full[0] == om.encode(text)
        for k in (1, 2, 3, 5, 8):
            rows, scs = nc.nbest(inc, scores, len(text), k)
            assert rows == full[:k] and scs == fs[:k]


def test_no_path():
    toks, scores, om = _tiny_model()
    inc = sc.incoming(om, b"abd", 3)
    assert nc.nbest(inc, scores, 3, 4) == ([], [])
    assert nc.nbest(sc.incoming(om, b"", 3), scores, 0, 4) == ([[]], [0.0])


def _fake_device(seg_lists, k):
    """Per-segment lists -> the device's output shape (nbest rows per segment)."""
    ids, offs, scs, nf = [], [0], [], []
    for rows, s in seg_lists:
        nf.append(len(rows))
        for r in range(k):
            row = rows[r] if r < len(rows) else []
            ids += row
            offs.append(offs[-1] + len(row))
            scs.append(s[r] if r < len(rows) else -math.inf)
    return np.array(ids, np.uint32), np.array(offs, np.uint64), np.array(scs), np.array(nf, np.uint32)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_segment_product_against_brute_force(k):
    toks, scores, om = _tied_model()
    rng = random.Random(k)
    base = 100
    # samples: lists of segments, a segment being a special index or text
    samples = [[b"aab"], [], [0], [b"ab", 1, b"ba"], [b"abb", b"aab"], [2, b"aba", 0, b"bb", 1], [b"a", 0]]
    for _ in range(10):
        samples.append([rng.choice([b"ab", b"aab", b"ba", b"abab", 0, 1]) for _ in range(rng.randrange(1, 5))])
    seg_offs, seg_special, seg_lists = [0], [], []
    for smp in samples:
        for g in smp:
            if isinstance(g, int):
                seg_special.append(g)
            else:
                seg_special.append(-1)
                inc = sc.incoming(om, g, 3)
                seg_lists.append(nc.nbest(inc, scores, len(g), k))
        seg_offs.append(len(seg_special))
    ids, id_offs, scs, nf = _fake_device(seg_lists, k)
    got_ids, got_offs, got_scores, got_nf = combine_nbest(np.array(seg_offs, np.uint64), np.array(seg_special, np.int32), base,
                                                          ids, id_offs, scs, nf, k)
    assert got_offs.size == len(samples) * k + 1
    j = 0
    for s, smp in enumerate(samples):
        parts = []
        for g in smp:
            if isinstance(g, int):
                parts.append(([[base + g]], [0.0]))
            else:
                parts.append(seg_lists[j])
                j += 1
        want_rows, want_scores = nc.combine_brute(parts, k)
        assert got_nf[s] == len(want_rows)
        for r in range(k):
            row = got_ids[int(got_offs[s * k + r]):int(got_offs[s * k + r + 1])].tolist()
            if r < len(want_rows):
                assert row == want_rows[r], (s, r)
                assert got_scores[s * k + r] == want_scores[r]
            else:
                assert row == [] and got_scores[s * k + r] == -math.inf


@pytest.mark.parametrize("alpha", [0.0, 0.3, 1.0, 50.0])
def test_nbest_draw_matches_the_formula(alpha):
    rng = np.random.default_rng(3)
    S, k = 300, 8
    scores = -np.round(rng.exponential(3.0, (S, k)), 1)
    scores = -np.sort(-scores, axis=1)
    nf = rng.integers(1, k + 1, S).astype(np.uint32)
    for i in range(S):
        scores[i, nf[i]:] = -np.inf
    for seed in (0, 12345, 2**64 - 1):
        got = nbest_draw(scores, nf, alpha, seed)
        for i in range(S):
            best, arg = -math.inf, -1
            for r in range(int(nf[i])):
                key = alpha * scores[i, r] - math.log(-math.log(_lib.sample_u01(seed, i, r, 0)))
                if key > best:
                    best, arg = key, r
            assert got[i] == arg


def test_symbols_and_header():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "tgx.h")).read()
    for name in ("tgx_encode_batch_nbest", "tgx_encode_corpus_nbest"):
        assert name in out
        assert name + "(" in hdr
    assert "#define TGX_MAX_NBEST 16" in hdr
    assert _lib.MAX_NBEST == 16


def test_entry_points_reject_bad_arguments():
    flat, offs = tgx.pack([b"ab"])
    h = _lib.C.c_void_p()
    ok = (_lib.ERR_DEVICE, _lib.ERR_INVALID)
    assert _lib.lib.tgx_encode_batch_nbest(None, _lib.ptr(flat), _lib.ptr(offs), 1, 2, None, None, _lib.C.byref(h)) in ok
    assert _lib.lib.tgx_encode_batch_nbest(None, _lib.ptr(flat), _lib.ptr(offs), 1, 2, None, None, None) in ok
    assert _lib.lib.tgx_encode_corpus_nbest(None, None, 2, None, None, _lib.C.byref(h)) in ok
    tk = tgx.Tokenizer([(b"a", -1.0, False), (b"b", -1.0, False)])
    for bad in (0, 17):
        with pytest.raises(tgx.TokenGeeXError) as e:
            tk.encode_batch_nbest_flat(flat, offs, bad)
        assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(tgx.TokenGeeXError) as e:
        tk.encode_batch_nbest_sample(["ab"], 2, float("nan"), seed=1)
    assert e.value.status == _lib.ERR_INVALID
    if tgx.device_count() == 0:
        with pytest.raises(tgx.TokenGeeXError) as e:
            tk.encode_nbest("ab", 2)
        assert e.value.status == _lib.ERR_DEVICE
