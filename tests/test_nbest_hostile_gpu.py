"""N-best on the GPU where the usual vocabularies never go (cases: tests/hostile_cases.py, established on the CPU by
tests/test_hostile_cpu.py): lattices in which all K entries of every list tie and the pinned key alone orders them,
tokens of 63 and 64 bytes (lm = 64: one wave per block, the back-pointer's length field 0, the receiving lane the
finalising lane), scores whose sums collapse in f64, positive and zero scores, a duplicated token, ids above 2^16, the
block-boundary lengths and the chunked path over 64-byte tokens.

Rows, scores and n_found are nbest_checker.nbest's bit for bit, for k in 1, 3, 8, 16; row 0 is encode's, rows are
pairwise distinct, scores do not increase, and a row's path_score is its reported score.  The 500 000-entry model is
built once for the module (the longest fixture here: 0.13 s measured, see test_case)."""
import functools
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import hostile_cases as hc
import nbest_checker as nc

KS = [1, 3, 8, 16]


@functools.lru_cache(maxsize=None)
def _native(name: str):
    c = hc.nbest_case(name)
    t = time.time()
    native = tgx.NativeModel(c["toks"], c["scores"])
    print(f"NativeModel of {name}: {len(c['toks'])} tokens in {time.time() - t:.2f} s")
    return native


def _launches(native):
    """The first eight timed launches of the last call, by name, repeats included."""
    names, ms = (_lib.C.c_char_p * 8)(), (_lib.C.c_float * 8)()
    n = _lib.lib.tgx_last_kernel_times(native._h, names, ms, 8)
    return [names[i].decode() for i in range(n)]


def _nbest(native, texts, k):
    res, scores, nf = native.encode_batch_nbest_flat(*tgx.pack(texts), k)
    assert res.num_samples == len(texts) * k
    ids, oo = res.ids().copy(), res.offsets().copy()
    res.free()
    return [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)], scores, nf


def _encode(native, texts):
    res = native.encode_batch_flat(*tgx.pack(texts))
    ids, oo = res.ids().copy(), res.offsets().copy()
    res.free()
    return [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]


def _assert_rows(c, texts, want, k, rows, scores, nf, enc):
    toks, vs = c["toks"], c["scores"]
    for i, (wr, ws) in enumerate(want):
        assert nf[i] == min(k, len(wr)), (c["name"], k, i, len(texts[i]))
        got = rows[i * k:i * k + int(nf[i])]
        for r in range(k):
            if r < nf[i]:
                assert rows[i * k + r] == wr[r], (c["name"], k, i, len(texts[i]), r)
                assert scores[i * k + r] == ws[r], (c["name"], k, i, r, scores[i * k + r], ws[r])
                assert nc.path_score(rows[i * k + r], vs) == scores[i * k + r]
                assert b"".join(toks[t] for t in rows[i * k + r]) == texts[i]
            else:
                assert rows[i * k + r] == [] and scores[i * k + r] == -math.inf
        assert rows[i * k] == enc[i], (c["name"], k, i)
        assert len({tuple(r) for r in got}) == len(got)
        assert all(a >= b for a, b in zip(scores[i * k:i * k + int(nf[i])], scores[i * k + 1:i * k + int(nf[i])]))


@pytest.mark.parametrize("name", hc.NBEST_CASES)
def test_case(name):
    """ties16 / ties33 / ties64: a...a at the edge lengths and at 2 .. 6 bytes under b"a" * k at -3 k: every list is K
    equal scores, ordered by the key through nb_merge; n_found = min(k, 2^(n - 1)) below 6 bytes, k from there on.
    len64: a 64-byte and a 63-byte token on the rows.  collapsing: sums that round together near -1e15, +2.5, 0.0, the
    later id of the duplicated token.  big_ids: the committed 500 000-entry vocabulary on 40 corpus samples, ids of
    2^16 and above on the rows (the model's build is the long step: 0.13 s measured on an MI355X host, the test 0.5 s)."""
    c = hc.nbest_case(name)
    native = _native(name)
    texts, want = c["texts"], c["want"]
    enc = _encode(native, texts)
    for k in KS:
        rows, scores, nf = _nbest(native, texts, k)
        ran = _launches(native)
        assert ran[:2] == ["nbest_kernel", "nbest_trace_kernel"] and ran.count("nbest_kernel") == 1, ran
        _assert_rows(c, texts, want, k, rows, scores, nf, enc)
        lens = {len(c["toks"][t]) for r in rows for t in r}
        used = {t for r in rows for t in r}
        if name.startswith("ties"):
            ml = int(name[4:])
            for i, t in enumerate(texts):
                n = len(t)
                assert nf[i] == (1 if n == 0 else min(k, 2 ** (n - 1)) if n < 6 else k), (name, k, n)
                assert list(scores[i * k:i * k + int(nf[i])]) == [-3.0 * n] * int(nf[i])
            assert ml in lens and (k < 16 or ml - 1 in lens)
        elif name == "len64" and k == 16:
            assert {63, 64} <= lens
        elif name == "collapsing":
            toks = c["toks"]
            assert {toks.index(b"ba"), toks.index(b"aa"), 15} <= used and 4 not in used
            assert min(scores[np.isfinite(scores)]) < -1e15
        elif name == "big_ids":
            assert max(used) >= 1 << 16 and (nf == k).all()


def test_chunked_path_with_long_tokens(monkeypatch):
    """len64's texts eight times over (14 KiB) at a budget of 1 MiB: two chunks at k = 16 (128 bytes of scratch per text
    byte), so the second chunk's rows start at a sample and byte offset of their own; ids, offsets, scores and n_found
    are the unchunked call's, and the checker's."""
    c = hc.nbest_case("len64")
    native = _native("len64")
    texts, want = c["texts"] * 8, c["want"] * 8
    flat, offs = tgx.pack(texts)
    enc = _encode(native, texts)
    for k in (3, 16):
        a, sa, na = native.encode_batch_nbest_flat(flat, offs, k)
        assert _launches(native).count("nbest_kernel") == 1
        monkeypatch.setenv("TGX_NBEST_CHUNK_MB", "1")
        b, sb, nb = native.encode_batch_nbest_flat(flat, offs, k)
        monkeypatch.delenv("TGX_NBEST_CHUNK_MB")
        assert _launches(native).count("nbest_kernel") == (2 if k == 16 else 1)
        ids, oo = a.ids().copy(), a.offsets().copy()
        assert np.array_equal(b.ids(), ids) and np.array_equal(b.offsets(), oo)
        assert np.array_equal(sb.view(np.uint64), sa.view(np.uint64)) and np.array_equal(nb, na)
        a.free()
        b.free()
        rows = [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(oo.size - 1)]
        _assert_rows(c, texts, want, k, rows, sa, na, enc)
        assert 64 in {len(c["toks"][t]) for r in rows for t in r}
