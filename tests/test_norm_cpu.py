"""The host twin of the device normalisation (tgx_normalize_host: the kernels' tiles, slots and pieces through the decoder,
the stream machine and the index arithmetic of csrc/norm.h) against normalize_flat (csrc/unicode_norm.cpp) and, for rows
that are UTF-8, against unicodedata.normalize.  All four forms; no device."""
import functools
import unicodedata as ud

import numpy as np
import pytest

from tokengeex_amd import _lib

import norm_cases as nc


def _twin(form, rows):
    flat, offs = _lib.pack(rows)
    f, o, k = _lib.normalize_host_twin(form, flat, offs)
    assert o.shape[0] == len(rows) + 1 and int(o[0]) == 0 and int(o[-1]) == f.size
    return f, o, k


def _same(form, rows, key):
    want_f, want_o = nc.truth(form, list(rows))
    f, o, k = _twin(form, rows)
    bad = np.nonzero(np.diff(o.astype(np.int64)) != np.diff(want_o.astype(np.int64)))[0]
    assert bad.size == 0, (form, key, "row", int(bad[0]), rows[int(bad[0])])
    assert np.array_equal(o, want_o) and np.array_equal(f, want_f), (form, key)
    return k


@functools.lru_cache(maxsize=None)
def _every_scalar(wrap):
    return tuple(wrap.format(chr(cp)) for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF)


@pytest.mark.parametrize("form", nc.FORMS)
@pytest.mark.parametrize("wrap", ["{}", "a{}b", "e{}\u0301"])
def test_every_scalar_value(form, wrap):
    """one batch per wrap, so the scalars fall at every phase of a slot and of a tile"""
    texts = _every_scalar(wrap)
    rows = [t.encode("utf-8") for t in texts]
    flat, offs = _lib.pack(rows)
    f, o, k = _lib.normalize_host_twin(form, flat, offs)
    want_f, want_o = _lib.normalize_flat(form, flat, offs)
    assert np.array_equal(o, want_o) and np.array_equal(f, want_f)
    want = [ud.normalize(form.upper(), t).encode("utf-8") for t in texts]
    lens = np.fromiter((len(w) for w in want), np.int64, len(want))
    assert np.array_equal(np.diff(o.astype(np.int64)), lens) and f.tobytes() == b"".join(want)
    # the pieces are the rows that hold an active scalar (or, behind 'e', a mark): what the header documents
    active = {"nfd": 14101, "nfc": 2060, "nfkd": 17776, "nfkc": 5747}[form]
    assert k == (len(rows) if wrap.startswith("e") else active)
    if wrap == "a{}b":   # ... and as one row
        f1, o1, k1 = _lib.normalize_host_twin(form, flat, np.array([0, flat.size], np.uint64))
        assert np.array_equal(f1, f) and o1.tolist() == [0, f.size] and k1 == k


@pytest.mark.parametrize("form", nc.FORMS)
def test_random_sequences_with_combining_marks(form):
    assert _same(form, nc.random_rows(), "random") > 10000


@pytest.mark.parametrize("form", nc.FORMS)
def test_edges_of_slots_tiles_and_rows(form):
    rows = nc.edge_batch()
    assert sum(len(r) for r in rows) > 12 * nc.TILE and sum(not r for r in rows) > 10
    assert _same(form, rows, "edges") > 20
    f, o, _ = _twin(form, rows)
    got = [bytes(f[int(o[i]):int(o[i + 1])]) for i in range(len(rows))]
    # a mark that starts a row does not compose with the row in front of it; a sequence cut by a row end stays as it is
    k = rows.index("\u0301abc".encode())
    assert got[k - 1].endswith(b"e") and got[k] == rows[k]
    k = rows.index(b"\x81abc")
    assert got[k - 1] == rows[k - 1] and got[k] == rows[k]
    assert all(len(g) > 0 for g, r in zip(got, rows) if r) and all(g == b"" for g, r in zip(got, rows) if not r)


@pytest.mark.parametrize("form", nc.FORMS)
def test_past_cap_corpus_reaches_every_threshold(form):
    """the arithmetic of csrc/norm.hip's launchers on the corpus, from the mirrored constants, and the twin on it"""
    cap, tile, block, piece_block = 4096, 4096, 256, 64     # kNormMaxBlocks, kFrontTile, the row kernels' block, kPieceBlock
    flat, offs = nc.past_cap_corpus()
    n, S = flat.size, offs.size - 1
    lens = np.diff(offs.astype(np.int64))
    assert n > cap * tile + 2 * tile and S > block * cap
    want_f, want_o = _lib.normalize_flat(form, flat, offs)
    f, o, k = _lib.normalize_host_twin(form, flat, offs)
    print(f"{form}: bytes {n}, tiles {-(-n // tile)}, rows {S}, pieces {k}")
    assert np.array_equal(o, want_o) and np.array_equal(f, want_f)
    assert k > piece_block * cap
    # the ASCII of three tiles lies in the second trip's tiles, and there are pieces behind it
    long = np.flatnonzero(lens == 3 * tile)
    assert long.size == 1 and int(offs[long[0]]) >= cap * tile
    run = flat[int(offs[long[0]]):int(offs[long[0] + 1])]
    assert (run < 128).all() and not np.array_equal(f[int(o[long[0] + 1]):], flat[int(offs[long[0] + 1]):])
    assert (lens[:-1] + lens[1:] == 0).sum() > 3000


@pytest.mark.parametrize("form", nc.FORMS)
def test_bytes_that_are_not_utf8_pass_through(form):
    _same(form, nc.INVALID, "invalid")
    _same(form, [b"".join(nc.INVALID)], "invalid, one row")
    for cut in range(1, 4):   # every cut of a four-byte scalar and of a mark behind its base
        for whole in ("\U0001d165".encode(), "e\u0301".encode(), "\u00e9\u0323".encode(), "\uac00\u11a8".encode()):
            _same(form, [b"ab" + whole[:cut], whole[cut:] + b"cd"], ("cut", cut, whole))


@pytest.mark.parametrize("form", nc.FORMS)
def test_window(form):
    marks31, marks32 = nc.descending_marks(31), nc.descending_marks(32)
    # a starter and 31 non-starters fill the window
    rows = [b"ok", ("e" + marks31).encode(), b"", ("x" + marks31 + "y" + marks31).encode()]
    assert _same(form, rows, "31 marks") == 3
    # one more is refused, and the lower of two such rows is named
    for bad, want in (([b"ok", ("e" + marks32).encode()], 1), ([b"ok", b"", ("e" + marks32).encode(), ("e" + marks31).encode(), ("o" + marks32 + "!").encode()], 2),
                      ([(marks32 + "\u0301").encode()] + [b"a" * 5000, ("e" + marks32).encode()], 0)):
        with pytest.raises(_lib.TokenGeeXError) as e:
            _twin(form, bad)
        assert e.value.status == _lib.ERR_UNSUPPORTED and e.value.sample == want and "32" in str(e.value), (form, want, e.value)
    # 3000 active starters in one piece: the window never grows
    rows = [("\uac00" + "\u1161" * 3000).encode(), b"tail"]
    assert _same(form, rows, "jamo") == 1


def test_mixed_text_has_no_piece_under_the_canonical_forms():
    rows = nc.mixed_rows()
    flat, offs = _lib.pack(rows)
    assert flat.size >= 40 << 10 and (flat >= 0x80).sum() > 1000
    for form in ("nfc", "nfd"):
        f, o, k = _lib.normalize_host_twin(form, flat, offs)
        assert k == 0 and np.array_equal(f, flat) and np.array_equal(o, offs)
    assert _same("nfkc", rows, "mixed") > 0
    assert not np.array_equal(_twin("nfkc", rows)[0], flat)   # its fullwidth punctuation changes


def test_arguments():
    flat, offs = _lib.pack([b"abc"])
    for call in (lambda: _lib.lib.tgx_normalize_host(4, _lib.ptr(flat), _lib.ptr(offs), 1, None, None, None),):
        assert call() == _lib.ERR_INVALID
    import ctypes as C
    ot, oo, k = C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert _lib.lib.tgx_normalize_host(4, _lib.ptr(flat), _lib.ptr(offs), 1, C.byref(ot), C.byref(oo), C.byref(k)) == _lib.ERR_INVALID
    assert "form" in _lib.lib.tgx_last_error().decode()
    for rows in ([], [b""], [b"", b"", b""]):
        f, o, k = _twin("nfc", rows)
        assert f.size == 0 and o.tolist() == [0] * (len(rows) + 1) and k == 0
