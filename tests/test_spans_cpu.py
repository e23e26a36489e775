"""Token spans through the host twin (tgx_spans_host: the index arithmetic of csrc/spans.h that the kernels of
csrc/spans.hip run, over host arrays; no device) against the plain restatement in tests/spans_checker.py and against the
text itself.  Everything is compared exactly: this is integer data movement."""
import functools
import itertools

import numpy as np
import pytest

from tokengeex_amd import _lib, synth

import decode_checker as dc
import spans_checker as sc

TILE = 1024      # kSpanTile of csrc/spans.h: elements per tile of the flat writer
POISON = -77     # what a destination holds before the call: an element that was skipped shows
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]
UNITS = ["byte", "char"]
BYTE_TOKENS = [bytes([b]) for b in range(256)]


def _rows_to_flat(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    ids = np.fromiter(itertools.chain.from_iterable(rows), dtype=np.uint32, count=int(offs[-1]))
    return ids, offs


class Vocab:
    def __init__(self, tokens, specials=()):
        self.tokens, self.specials = list(tokens), list(specials)
        self.vf, self.vo = _lib.pack(self.tokens)
        self.sf, self.so = _lib.pack(self.specials)
        self.V, self.NS = len(self.tokens), len(self.specials)
        self.lookup = sc.vocab_lookup(self.tokens, self.specials)

    def twin(self, ids, offs, **kw):
        return _lib.spans_host(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, **kw)

    def check_flat(self, ids, offs, key=None):
        """both units and both dtypes against the checker -> {unit: [T, 2] int64}"""
        got = {}
        for unit in UNITS:
            want = sc.flat(ids, offs, self.lookup, unit)
            for dt in (np.int32, np.int64):
                out = np.full(want.shape, POISON, dt)
                assert self.twin(ids, offs, unit=unit, dtype=dt, out=out) is out
                assert out.dtype == dt and np.array_equal(out, want), (key, unit, dt)
            got[unit] = want
        return got

    def check_padded(self, ids, offs, row_lens, key=None):
        for unit, (bos, eos), pside, tside, dt in itertools.product(UNITS, BOS_EOS, ["right", "left"], ["right", "left"], [np.int32, np.int64]):
            a = (bos is not None) + (eos is not None)
            for L in row_lens(a):
                out = np.full((len(offs) - 1, L, 2), POISON, dt)
                self.twin(ids, offs, unit=unit, dtype=dt, row_len=L, bos_id=bos, eos_id=eos, padding_side=pside, truncation_side=tside, out=out)
                want = sc.padded(ids, offs, self.lookup, unit, L, bos, eos, pside == "left", tside == "left", dt)
                assert np.array_equal(out, want), (key, unit, bos, eos, pside, tside, dt, L)


def _row_lens(offs):
    n = np.diff(offs.astype(np.int64))
    mx, med = int(n.max()), int(np.median(n[n > 0])) if (n > 0).any() else 0
    return lambda a: sorted({max(1, a), max(1, a, med + a), max(1, mx + a), mx + a + 3})


@functools.lru_cache(maxsize=None)
def _bytes_vocab():
    return Vocab(BYTE_TOKENS, [b"<s>"])


@functools.lru_cache(maxsize=None)
def _mixed_vocab():
    return Vocab(dc.mixed_tokens(), dc.MIXED_SPECIALS)


CJK_ROWS = ["你好，世界", "a\U0001f600b\U0001f4a9", "", "日本語 text é€", "\U0001f600", "x"]


def test_single_byte_vocabulary_splits_every_character():
    """Every token is one byte, so every character of more than one byte is split and cont matters: all the byte tokens of
    one character get that character.  One row holds a stray 0x80 (in the middle and at the very start)."""
    v = _bytes_vocab()
    texts = [t.encode() for t in CJK_ROWS] + ["好".encode() + b"\x80" + "好".encode(), b"\x80\x80a"]
    ids, offs = _rows_to_flat([list(t) for t in texts])
    got = v.check_flat(ids, offs)
    v.check_padded(ids, offs, _row_lens(offs))
    for i, raw in enumerate(texts[:len(CJK_ROWS)]):
        s = raw.decode()
        lo, hi = int(offs[i]), int(offs[i + 1])
        cs_prev = 0
        for j in range(lo, hi):
            (b, e), (cs, ce) = got["byte"][j], got["char"][j]
            assert e == b + 1 and ce == cs + 1 and cs >= cs_prev    # a byte token lies in exactly one character
            cs_prev = cs
            sub, before = s[cs:ce].encode(), len(s[:cs].encode())
            assert sub[b - before:e - before] == raw[b:e] == bytes([ids[j]]), (i, j)
        if hi > lo:
            assert got["char"][hi - 1][1] == len(s)
    # the stray byte is attributed to the character before it; where there is none the start is -1
    j0 = int(offs[len(CJK_ROWS)])
    assert got["char"][j0:j0 + 7].tolist() == [[0, 1]] * 3 + [[0, 1]] + [[1, 2]] * 3
    j1 = int(offs[len(CJK_ROWS) + 1])
    assert got["char"][j1:j1 + 3].tolist() == [[-1, 0], [-1, 0], [0, 1]]


@functools.lru_cache(maxsize=None)
def _spec_case():
    """the committed 32 000 vocabulary over ~8 KiB of mixed text; the ids come from the CPU oracle's encode"""
    from oracle import oracle as orc
    toks, scores, _ = synth.load_spec_vocab(32000)
    toks, scores = list(toks), np.asarray(scores, np.float64)
    flat, offs = synth.make_corpus(8 << 10, "mixed", max_len=2048, seed_offset=3)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    rows = [b""] + rows[:2] + [b"", b""] + rows[2:] + [b""]       # empty rows at the start, in the middle and at the end
    flat, offs = _lib.pack(rows)
    ids, oo = orc.OracleModel(toks, scores).encode_batch_flat(flat, offs, 0.0, 0, threads=4)
    return Vocab(toks, [b"<pad>", b"<s>"]), rows, np.asarray(ids, np.uint32), np.asarray(oo, np.uint64)


def test_spec_vocabulary_spans_index_the_text():
    v, rows, ids, offs = _spec_case()
    n = np.diff(offs.astype(np.int64))
    assert ids.size > 2 * TILE and n[0] == 0 and n[-1] == 0 and (n == 0).sum() >= 4 and n.max() > 100
    got = v.check_flat(ids, offs)
    for i, raw in enumerate(rows):
        lo, hi = int(offs[i]), int(offs[i + 1])
        sp = got["byte"][lo:hi]
        for j in range(lo, hi):
            b, e = sp[j - lo]
            assert raw[b:e] == v.tokens[ids[j]], (i, j)
        if hi > lo:   # the spans tile the row
            assert sp[0][0] == 0 and np.array_equal(sp[1:, 0], sp[:-1, 1]) and sp[-1][1] == len(raw)
            s = raw.decode()
            cs, ce = got["char"][lo:hi, 0], got["char"][lo:hi, 1]
            assert cs[0] == 0 and ce[-1] == len(s) and (cs[1:] <= ce[:-1]).all() and (ce[:-1] <= cs[1:] + 1).all()
            for j in range(lo, hi, 7):
                b, e = sp[j - lo]
                sub, before = s[cs[j - lo]:ce[j - lo]].encode(), len(s[:cs[j - lo]].encode())
                assert sub[b - before:e - before] == raw[b:e], (i, j)


def test_spec_vocabulary_padded_form():
    v, rows, ids, offs = _spec_case()
    v.check_padded(ids, offs, _row_lens(offs))


def test_random_rows_with_specials_and_invalid_bytes():
    """rows of 0, 1, a tile minus / plus one and more than a tile of tokens, of every kind the mixed vocabulary has: empty
    tokens, tokens of up to 64 bytes, split characters, invalid bytes, special tokens (one empty, one not UTF-8)"""
    v = _mixed_vocab()
    rng = np.random.default_rng(5)
    lens = [0, 0, 1, TILE - 1, 0, TILE, TILE + 1, 3, 1500, 0, 2, 0]
    rows = []
    for n in lens:
        row = rng.integers(0, v.V, n)
        sp = rng.random(n) < 0.08
        row[sp] = v.V + rng.integers(0, v.NS, int(sp.sum()))
        rows.append(row.tolist())
    ids, offs = _rows_to_flat(rows)
    v.check_flat(ids, offs)
    v.check_padded(ids, offs, lambda a: sorted({max(1, a), 2 + a, TILE + a, 1500 + a + 3}))


def test_empty_inputs():
    v = _mixed_vocab()
    for unit, dt in itertools.product(UNITS, [np.int32, np.int64]):
        # S = 0
        z = np.zeros(1, np.uint64)
        assert v.twin(np.zeros(0, np.uint32), z, unit=unit, dtype=dt).shape == (0, 2)
        assert v.twin(np.zeros(0, np.uint32), z, unit=unit, dtype=dt, row_len=4).shape == (0, 4, 2)
        # T = 0: the padded form is filled with 0
        z = np.zeros(4, np.uint64)
        assert v.twin(np.zeros(0, np.uint32), z, unit=unit, dtype=dt).shape == (0, 2)
        out = np.full((3, 5, 2), POISON, dt)
        v.twin(np.zeros(0, np.uint32), z, unit=unit, dtype=dt, row_len=5, bos_id=1, eos_id=2, out=out)
        assert (out == 0).all()


def test_arguments_are_checked():
    v = _mixed_vocab()
    ids, offs = _rows_to_flat([[1, 2], [3]])
    with pytest.raises(_lib.TokenGeeXError) as e:
        v.twin(np.array([1, v.V + v.NS], np.uint32), np.array([0, 1, 2], np.uint64))
    assert e.value.status == _lib.ERR_TOKEN_ID_OOB and e.value.sample == 1
    for kw in ({"row_len": 1, "bos_id": 1, "eos_id": 2}, {"row_len": 4, "bos_id": 2**31}):
        with pytest.raises(_lib.TokenGeeXError) as e:
            v.twin(ids, offs, **kw)
        assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        v.twin(ids, offs, unit="word")
    with pytest.raises(ValueError):
        v.twin(ids, offs, dtype=np.int16)
    st = _lib.lib.tgx_spans_host(_lib.ptr(v.vf), _lib.ptr(v.vo), v.V, _lib.ptr(v.sf), _lib.ptr(v.so), v.NS, _lib.ptr(ids), _lib.ptr(offs), 2, 0,
                                 _lib.NO_ID, _lib.NO_ID, 64, _lib.ptr(np.zeros((3, 2), np.int32)))
    assert st == _lib.ERR_INVALID     # an unknown flag
    st = _lib.lib.tgx_spans_host(_lib.ptr(v.vf), _lib.ptr(v.vo), v.V, _lib.ptr(v.sf), _lib.ptr(v.so), v.NS, _lib.ptr(ids), _lib.ptr(offs), 2, 0,
                                 _lib.NO_ID, _lib.NO_ID, _lib.LAYOUT_PAD_LEFT, _lib.ptr(np.zeros((3, 2), np.int32)))
    assert st == _lib.ERR_INVALID     # a side flag in the flat form


def test_sums_are_64_bit_and_int32_is_refused_when_a_row_does_not_fit():
    """Three special tokens that special_offs declares as 2^30 bytes each, three rows of three: the global sum passes 2^32
    and every row 2^31.  The byte unit reads no special byte, so none exists.  The character unit needs them: it gets
    real bytes in a small case of the same shape."""
    toks = [b"a", b"bc"]
    vf, vo = _lib.pack(toks)
    G = 1 << 30
    so = np.array([0, G, 2 * G, 3 * G], np.uint64)
    ids, offs = _rows_to_flat([[2, 3, 4], [4, 4, 4], [3, 0, 2]])
    none = np.zeros(0, np.uint8)
    got = _lib.spans_host(vf, vo, 2, none, so, 3, ids, offs, unit="byte", dtype=np.int64)
    want = [[0, G], [G, 2 * G], [2 * G, 3 * G]] * 2 + [[0, G], [G, G + 1], [G + 1, 2 * G + 1]]
    assert got.tolist() == want
    got = _lib.spans_host(vf, vo, 2, none, so, 3, ids, offs, unit="byte", dtype=np.int64, row_len=3, eos_id=1, truncation_side="left")
    assert got.tolist() == [[want[1], want[2], [0, 0]], [want[4], want[5], [0, 0]], [want[7], want[8], [0, 0]]]
    for kw in ({}, {"row_len": 2}):
        out = np.full((3, 2, 2) if kw else (9, 2), POISON, np.int32)
        with pytest.raises(_lib.TokenGeeXError) as e:
            _lib.spans_host(vf, vo, 2, none, so, 3, ids, offs, unit="byte", dtype=np.int32, out=out, **kw)
        assert e.value.status == _lib.ERR_UNSUPPORTED and (out == POISON).all()     # and nothing was written
    # a row of 2^31 - 1 bytes still fits int32
    so2 = np.array([0, G, 2 * G - 1], np.uint64)
    got = _lib.spans_host(vf, vo, 2, none, so2, 2, np.array([2, 3], np.uint32), np.array([0, 2], np.uint64), dtype=np.int32)
    assert got.tolist() == [[0, G], [G, 2 * G - 1]]
    # the character unit on the same shape, small: three specials of 3, 4 and 5 bytes with 1, 2 and 3 characters
    v = Vocab(toks, ["好".encode(), "éé".encode(), "aéb".encode() + b"\x80"])
    v.check_flat(ids, offs)
    v.check_padded(ids, offs, _row_lens(offs))
