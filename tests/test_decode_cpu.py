"""The decode of ids to UTF-8 text through the host twin (tgx_decode_rows_host: the index arithmetic of csrc/decode.h that
the kernels of csrc/decode.hip run, over host arrays; no device).  The offsets form is compared with the existing host decode
(tgx_decode_batch), the padded form with the plain restatement in tests/decode_checker.py, the local UTF-8 rule with
Python's bytes.decode("utf-8", "replace").  Everything is compared exactly."""
import functools
import itertools

import numpy as np
import pytest

from tokengeex_amd import _lib

import decode_checker as dc

TILE = 4096   # kDecodeTile of csrc/decode.h: raw bytes per tile of the fill kernel
ALPHABET = dc.ALPHABET

BYTE_TOKENS = [bytes([b]) for b in range(256)]


def _pack(items):
    flat, offs = _lib.pack(list(items))
    return np.ascontiguousarray(flat), offs


def _rows_to_flat(rows, dtype=np.uint32):
    offs = np.zeros(len(rows) + 1, np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    ids = np.fromiter(itertools.chain.from_iterable(rows), dtype=dtype, count=int(offs[-1]))
    return ids, offs


class Vocab:
    def __init__(self, tokens, specials):
        self.tokens, self.specials = list(tokens), list(specials)
        self.vf, self.vo = _pack(self.tokens)
        self.sf, self.so = _pack(self.specials)
        self.V, self.NS = len(self.tokens), len(self.specials)

    def twin(self, ids, offs=None, include_special=True, **kw):
        return _lib.decode_rows_host(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, include_special=include_special, **kw)

    def host(self, ids, offs, include_special=True):
        return _lib.decode_batch_flat(self.vf, self.vo, self.V, self.sf, self.so, self.NS, np.ascontiguousarray(ids, np.uint32),
                                      np.ascontiguousarray(offs, np.uint64), include_special)

    def check_rows(self, rows, include_special, key=None):
        """the offsets form through the twin == tgx_decode_batch (bytes, offsets) and the checker's n_replaced"""
        ids, offs = _rows_to_flat(rows)
        got, got_offs, n_rep = self.twin(ids, offs, include_special)
        want, want_offs = self.host(ids, offs, include_special)
        assert np.array_equal(got_offs, want_offs), key
        assert np.array_equal(got, want), key
        c_bytes, c_offs, c_rep = dc.decode_rows(rows, self.tokens, self.specials, include_special)
        assert np.array_equal(c_bytes, want) and np.array_equal(c_offs, want_offs), key   # the two ground truths agree
        assert n_rep == c_rep, key
        return got, got_offs, n_rep


@functools.lru_cache(maxsize=None)
def _bytes_vocab():
    return Vocab(BYTE_TOKENS, [b"<s>"])


@functools.lru_cache(maxsize=None)
def _mixed_vocab():
    """an empty token, tokens of 1, 15, 16, 17, 63 and 64 bytes, UTF-8 characters split across tokens, invalid bytes; an
    empty special token, one that is not UTF-8 (it must come out verbatim) and two ordinary ones"""
    toks = dc.mixed_tokens()
    assert {len(t) for t in toks} >= {0, 1, 15, 16, 17, 63, 64}
    return Vocab(toks, dc.MIXED_SPECIALS)


def _random_rows(rng, vocab, n_rows, max_len, p_special=0.08):
    rows = []
    for _ in range(n_rows):
        n = int(rng.integers(0, max_len + 1))
        row = rng.integers(0, vocab.V, n)
        sp = rng.random(n) < p_special
        row[sp] = vocab.V + rng.integers(0, vocab.NS, int(sp.sum()))
        row = row.tolist()
        kind = int(rng.integers(0, 6))
        if kind == 0:
            row = [vocab.V + int(rng.integers(0, vocab.NS))] + row      # a special at the row's start
        elif kind == 1:
            row = row + [vocab.V + int(rng.integers(0, vocab.NS))]      # ... at its end
        elif kind == 2:
            row = [vocab.V + int(k) for k in rng.integers(0, vocab.NS, min(n, 9))]  # a row of specials only
        rows.append(row)
    return rows


# ---- the local UTF-8 rule ------------------------------------------------------------------------------------------

def test_utf8_rule_exhaustively_on_the_class_boundaries():
    """every string of up to 4 bytes over the boundary alphabet, each a row of single-byte tokens (so each is a run of its
    own, and every row end is a run end inside some 16-byte slot), against Python's replace"""
    v = _bytes_vocab()
    strings = [bytes(s) for n in range(5) for s in itertools.product(ALPHABET, repeat=n)]
    assert len(strings) == sum(25 ** n for n in range(5))
    ids = np.frombuffer(b"".join(strings), np.uint8).astype(np.uint32)
    offs = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum([len(s) for s in strings], out=offs[1:])
    got, got_offs, n_rep = v.twin(ids, offs, True)
    want = [s.decode("utf-8", "replace").encode("utf-8") for s in strings]
    want_offs = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum([len(w) for w in want], out=want_offs[1:])
    assert np.array_equal(got_offs, want_offs)
    assert got.tobytes() == b"".join(want)
    # no string of the alphabet holds U+FFFD itself (EF BF BD needs BD): every one in the output was written
    assert n_rep == sum(w.decode("utf-8").count(dc.REPLACEMENT) for w in want) and n_rep > 100_000


def test_utf8_rule_on_random_rows():
    v = _bytes_vocab()
    rng = np.random.default_rng(11)
    rows = []
    for k in range(4000):
        n = int(rng.integers(0, 41))
        src = ALPHABET if k % 2 else bytes(range(256))
        rows.append([src[i] for i in rng.integers(0, len(src), n)])
    # and rows that are mostly well-formed text with a few bytes damaged
    text = "naïve café — 東京 😀 ∑".encode()
    for k in range(500):
        b = bytearray(text * int(rng.integers(1, 4)))
        for i in rng.integers(0, len(b), int(rng.integers(0, 4))):
            b[i] = int(rng.integers(0, 256))
        rows.append(list(b))
    ids, offs = _rows_to_flat(rows)
    got, got_offs, n_rep = v.twin(ids, offs, True)
    want = [bytes(r).decode("utf-8", "replace") for r in rows]
    assert got.tobytes() == "".join(want).encode("utf-8")
    assert np.array_equal(np.diff(got_offs.astype(np.int64)), [len(w.encode("utf-8")) for w in want])
    assert n_rep == sum(w.count(dc.REPLACEMENT) - bytes(r).decode("utf-8", "ignore").count(dc.REPLACEMENT) for w, r in zip(want, rows))
    assert n_rep > 0 and any("😀" in w for w in want)


# ---- the offsets form against tgx_decode_batch -----------------------------------------------------------------------

@pytest.mark.parametrize("include_special", [False, True])
def test_random_plans_against_the_host_decode(include_special):
    v = _mixed_vocab()
    rng = np.random.default_rng(5 + include_special)
    for k in range(100):
        n_rows = int(rng.integers(0, 24))
        max_len = 3000 if k % 25 == 0 else int(rng.choice([0, 1, 5, 40, 300]))
        rows = _random_rows(rng, v, n_rows, max_len)
        if k % 7 == 0:
            rows = [[]] + rows + [[], []]
        v.check_rows(rows, include_special, ("plan", k))


def _rows_with_raw_size(rng, v, target, include_special):
    """rows whose raw bytes (before from_utf8_lossy) add up to `target`: random ids, the rest filled with 1-byte tokens"""
    lens = [len(t) for t in v.tokens] + [len(s) if include_special else 0 for s in v.specials]
    flat, total = [], 0
    while True:
        x = int(rng.integers(0, len(lens)))
        if total + lens[x] > target:
            break
        flat.append(x)
        total += lens[x]
    flat += [1] * (target - total)   # token 1 is b"a"
    cuts = sorted(rng.integers(0, len(flat) + 1, 6).tolist())
    return [flat[a:b] for a, b in zip([0] + cuts, cuts + [len(flat)])]


@pytest.mark.parametrize("size", [TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 2, 2 * TILE - 1, 2 * TILE + 1, 15, 16, 17])
def test_sizes_across_the_fill_tiles_edges(size):
    v = _mixed_vocab()
    rng = np.random.default_rng(size)
    for include_special in (False, True):
        rows = _rows_with_raw_size(rng, v, size, include_special)
        v.check_rows(rows, include_special, size)
        # the same size without anything to replace: the raw bytes are the text
        flat, total = [], 0
        for x in itertools.cycle([4, 5, 1, 2]):   # "the", " and", "a", " "
            if total + len(v.tokens[x]) > size:
                break
            flat.append(x)
            total += len(v.tokens[x])
        flat += [1] * (size - total)
        ascii_rows = [flat[:len(flat) // 2], flat[len(flat) // 2:]]
        got, got_offs, n_rep = v.check_rows(ascii_rows, include_special, size)
        assert got.size == size and n_rep == 0


def test_degenerate_batches():
    v = _mixed_vocab()
    for inc in (False, True):
        got, offs, n_rep = v.check_rows([], inc)
        assert got.size == 0 and offs.tolist() == [0] and n_rep == 0
        got, offs, n_rep = v.check_rows([[], [], []], inc)
        assert got.size == 0 and offs.tolist() == [0, 0, 0, 0]
        got, offs, n_rep = v.check_rows([[v.V, v.V + 3], [], [v.V + 1], [v.V + 2] * 5, [0, 0]], inc)   # specials only, empty tokens only
        assert (got.size > 0) == inc and n_rep == 0
    got, offs, _ = v.check_rows([[v.V + 2]], True)
    assert got.tobytes() == b"\xff<bad\x80>"   # a special token's bytes are not passed through from_utf8_lossy


def test_run_separation():
    v = _bytes_vocab()
    S = v.V   # <s>
    got, offs, n_rep = v.check_rows([[0xE2, 0x82], [0xAC]], True)     # a character cut by a row end
    assert got.tobytes().decode() == "\ufffd\ufffd" and offs.tolist() == [0, 3, 6] and n_rep == 2
    got, offs, n_rep = v.check_rows([[0xE2, 0x82, S, 0xAC]], False)     # ... by a special token that is not emitted
    assert got.tobytes().decode() == "\ufffd\ufffd" and n_rep == 2
    got, offs, n_rep = v.check_rows([[0xE2, 0x82, S, 0xAC]], True)
    assert got.tobytes().decode() == "\ufffd<s>\ufffd" and n_rep == 2
    got, offs, n_rep = v.check_rows([[0xE2, 0x82, 0xAC]], True)         # three single-byte tokens of one run
    assert got.tobytes().decode() == "€" and n_rep == 0
    got, offs, n_rep = v.check_rows([[0xEF, 0xBF, 0xBD, 0x80]], True)   # U+FFFD in the input is not a replacement
    assert got.tobytes().decode() == "\ufffd\ufffd" and n_rep == 1
    # an empty row between the halves, an empty token inside a character
    m = _mixed_vocab()
    e0, e12 = m.tokens.index(b"\xe2"), m.tokens.index(b"\x82\xac")
    got, _, n_rep = m.check_rows([[e0], [], [e12]], True)
    assert n_rep == 3
    got, _, n_rep = m.check_rows([[e0, 0, 0, e12]], True)
    assert got.tobytes().decode() == "€" and n_rep == 0
    got, _, n_rep = m.check_rows([[e0, m.V + 1, e12]], True)   # the EMPTY special token still separates
    assert n_rep == 3


# ---- the padded form against the checker -----------------------------------------------------------------------------

def _padded_case(rng, v, S, L, dtype):
    ids = rng.integers(0, v.V + v.NS, (S, L)).astype(dtype)
    lengths = rng.integers(-1, L + 2, S).astype(np.int32)    # negative and beyond L included
    mask = (rng.random((S, L)) < 0.7).astype(np.uint8)
    return ids, lengths, mask


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("L", [1, 7, 64])
def test_padded_form_against_the_checker(L, dtype):
    v = _mixed_vocab()
    rng = np.random.default_rng(100 + L)
    garbage = -7 if dtype == np.int32 else 2 ** 40 + 1
    for S in (0, 1, 5, 70):
        ids, lengths, mask = _padded_case(rng, v, S, L, dtype)
        skip = v.V + v.NS + 11       # out of bounds otherwise: skipping it is no error
        left = np.zeros((S, L), np.uint8)   # left-padded: the last n_i elements of a row are live
        for i in range(S):
            left[i, L - int(rng.integers(0, L + 1)):] = 1
        cases = {"plain": {}, "lengths": dict(lengths=lengths), "mask": dict(mask=mask), "both": dict(mask=mask, lengths=lengths),
                 "left": dict(mask=left), "skip": dict(skip_id=int(ids[0, 0]) if S else 3)}
        for name, kw in cases.items():
            for inc in (False, True):
                got = v.twin(ids, None, inc, **kw)
                want = dc.decode_padded(ids, v.tokens, v.specials, inc, **kw)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == want[2], (S, L, name, inc)
        if S == 0:
            continue
        # elements that are not live are not checked
        dirty = ids.copy()
        dirty[mask == 0] = garbage
        got = v.twin(dirty, None, True, mask=mask)
        want = dc.decode_padded(ids, v.tokens, v.specials, True, mask=mask)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        dirty = ids.copy()
        dirty[rng.random((S, L)) < 0.3] = skip
        dirty.flat[int(rng.integers(0, dirty.size))] = skip
        got = v.twin(dirty, None, True, skip_id=skip)
        want = dc.decode_padded(dirty, v.tokens, v.specials, True, skip_id=skip)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        with pytest.raises(_lib.TokenGeeXError) as e:
            v.twin(dirty, None, True)
        assert e.value.status == _lib.ERR_TOKEN_ID_OOB and str(e.value) == f"token id {skip} is out of bounds"
        with pytest.raises(dc.OutOfBounds) as c:
            dc.decode_padded(dirty, v.tokens, v.specials, True)
        assert (e.value.sample, e.value.pos) == (c.value.row, c.value.value)


def test_bool_mask_and_bad_shapes():
    v = _mixed_vocab()
    ids = np.arange(12, dtype=np.int64).reshape(3, 4)
    mask = ids % 3 != 0
    assert np.array_equal(v.twin(ids, None, True, mask=mask)[0], dc.decode_padded(ids, v.tokens, v.specials, True, mask=mask)[0])
    with pytest.raises(ValueError):
        v.twin(ids, None, True, mask=mask[:2])
    with pytest.raises(ValueError):
        v.twin(ids, None, True, lengths=np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        v.twin(ids.astype(np.int16), None, True)


# ---- out of bounds -----------------------------------------------------------------------------------------------------

def test_out_of_bounds_names_the_lowest_row_and_its_first_id():
    v = _mixed_vocab()
    rng = np.random.default_rng(8)
    bad = v.V + v.NS
    rows = [rng.integers(0, bad, 30).tolist() for _ in range(12)]
    rows[5][7] = bad + 4     # the first of row 5
    rows[5][20] = bad
    rows[9][0] = bad
    ids, offs = _rows_to_flat(rows)
    with pytest.raises(_lib.TokenGeeXError) as want:
        v.host(ids, offs, True)
    for inc in (False, True):
        with pytest.raises(_lib.TokenGeeXError) as got:
            v.twin(ids, offs, inc)
        assert got.value.status == want.value.status == _lib.ERR_TOKEN_ID_OOB
        assert str(got.value) == str(want.value) == f"token id {bad + 4} is out of bounds"
        assert (got.value.sample, got.value.pos) == (want.value.sample, want.value.pos) == (5, bad + 4)
    rows[5][7] = bad         # the issue's case: V + n_specials itself, twice in row 5 and once in row 9
    ids, offs = _rows_to_flat(rows)
    with pytest.raises(_lib.TokenGeeXError) as want:
        v.host(ids, offs, True)
    with pytest.raises(_lib.TokenGeeXError) as got:
        v.twin(ids, offs, True)
    assert str(got.value) == str(want.value) == f"token id {bad} is out of bounds"
    assert (got.value.status, got.value.sample, got.value.pos) == (_lib.ERR_TOKEN_ID_OOB, 5, bad)
    # the same rows as a padded tensor
    for dtype in (np.int32, np.int64):
        with pytest.raises(_lib.TokenGeeXError) as got:
            v.twin(np.asarray(rows, dtype), None, True)
        assert (got.value.status, got.value.sample, got.value.pos) == (_lib.ERR_TOKEN_ID_OOB, 5, bad)
    # and the twin still decodes
    rows[5][7] = rows[5][20] = rows[9][0] = 1
    v.check_rows(rows, True)


@pytest.mark.parametrize("value, dtype", [(-1, np.int64), (2 ** 32 + 3, np.int64), (-1, np.int32), (-(2 ** 31), np.int32), (-(2 ** 63), np.int64)])
def test_values_outside_u32_are_refused_with_their_value(value, dtype):
    v = _mixed_vocab()
    ids = np.ones((4, 5), dtype)
    ids[2, 3] = value
    ids[3, 0] = v.V + v.NS
    with pytest.raises(_lib.TokenGeeXError) as e:
        v.twin(ids, None, True)
    assert e.value.status == _lib.ERR_TOKEN_ID_OOB and str(e.value) == f"token id {value} is out of bounds"
    assert e.value.sample == 2 and e.value.pos == value % 2 ** 64   # the two's complement
    assert v.twin(ids, None, True, lengths=np.array([5, 5, 3, 0], np.int32))[0].tobytes() == b"a" * 13


def test_argument_checks():
    v = _mixed_vocab()
    with pytest.raises(_lib.TokenGeeXError) as e:
        v.twin(np.zeros(3, np.uint32), np.array([0, 2, 1], np.uint64))
    assert e.value.status == _lib.ERR_INVALID and "monotone" in str(e.value)
    long_vocab = Vocab([b"a", b"b" * 65], [])
    with pytest.raises(_lib.TokenGeeXError) as e:
        long_vocab.twin(np.zeros(3, np.uint32), np.array([0, 3], np.uint64))
    assert e.value.status == _lib.ERR_UNSUPPORTED
