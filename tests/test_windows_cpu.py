"""Overflow windows through the host twins (tgx_layout_windows_host, tgx_window_spans_host: the window mapping of
csrc/layout.h and csrc/spans.h that the kernels run, over host arrays; no device) against the plain restatement in
tests/windows_checker.py, against the padded twins where the two must agree, and against HuggingFace `tokenizers`'
truncation with a stride where that package is installed.  Everything is compared exactly: this is integer data
movement."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tokengeex_amd import _lib

import decode_checker as dc
import layout_checker as lc
import spans_checker as sc
import windows_checker as wc

PAD = 7
POISON = -77     # what a destination holds before the call: an element that was skipped or written shows
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]
SIDES = ["right", "left"]
LONG = 3001      # the long row: three tiles of 1024 elements at L = 1, and windows that straddle tile ends above


def _a(bos, eos):
    return (bos is not None) + (eos is not None)


def _row_lens(a):
    return sorted({a + 1, 5, 8, 13})


def _strides(room):
    return sorted(s for s in {0, 1, room // 2, room - 1} if 0 <= s < room)


def _flat(ns, rng, hi=5000):
    offs = np.zeros(len(ns) + 1, np.uint64)
    np.cumsum(ns, out=offs[1:])
    return rng.integers(10, hi, int(offs[-1])).astype(np.uint32), offs


def _row_sizes(room, step, long_row=True):
    """every size at which the window count or a window's length changes, an empty row first, in the middle and last"""
    return [0, room - 1, room, room + 1, 0, room + step, room + step + 1] + ([LONG] if long_row else []) + [2 * room + 3 * step, 0]


def _twin(ids, offs, L, stride, bos, eos, pside, tside, dt, **kw):
    got = _lib.layout_windows_host(ids, offs, L, stride, PAD, bos_id=bos, eos_id=eos, padding_side=pside, truncation_side=tside, dtype=dt, **kw)
    return got["input_ids"], got["attention_mask"], got["lengths"], got["overflow_to_sample_mapping"], got["window_first"]


def _same(got, want, key):
    assert len(got) == len(want) == 5
    for name, g, w in zip(("ids", "mask", "lengths", "row", "first"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (key, name)


def test_checker_forms_agree_and_cover_every_token():
    """The whole-array checker against the per-row one, and what the definition promises: the windows of a row cover its
    tokens in order, consecutive ones share exactly `stride` tokens (fewer only where the last one is short), and
    truncation on the left is the mirror image."""
    rng = np.random.default_rng(5)
    for (bos, eos), pl, tl in itertools.product(BOS_EOS, [False, True], [False, True]):
        a = _a(bos, eos)
        for L in _row_lens(a):
            for stride in _strides(L - a):
                room, step = L - a, L - a - stride
                ids, offs = _flat(_row_sizes(room, step, long_row=False) + [97], rng)
                slow = wc.windows_by_row(ids, offs, L, stride, PAD, bos, eos, pl, tl)
                _same(wc.windows(ids, offs, L, stride, PAD, bos, eos, pl, tl), slow, (bos, eos, pl, tl, L, stride))
                assert wc.n_windows(offs, L, stride, bos, eos) == slow[0].shape[0]
    for room, stride, n in itertools.product(range(1, 9), range(8), range(40)):
        if stride >= room:
            continue
        right, left = wc.row_windows(n, room, stride), wc.row_windows(n, room, stride, True)
        assert left == [(n - f - k, k) for f, k in right]
        assert right[0] == (0, min(n, room)) and right[-1][0] + right[-1][1] == n
        assert len(right) == 1 or right[-2][0] + right[-2][1] < n           # no window after the one that reaches the end
        for (f0, k0), (f1, k1) in zip(right, right[1:]):
            assert k0 == room and f1 == f0 + room - stride and 1 <= k1 <= room


def test_twin_against_the_checker():
    rng = np.random.default_rng(6)
    n_cases = 0
    for (bos, eos), pside, tside, dt in itertools.product(BOS_EOS, SIDES, SIDES, [np.int32, np.int64]):
        a = _a(bos, eos)
        for L in _row_lens(a):
            for stride in _strides(L - a):
                ids, offs = _flat(_row_sizes(L - a, L - a - stride), rng)
                want = wc.windows(ids, offs, L, stride, PAD, bos, eos, pside == "left", tside == "left", dt)
                _same(_twin(ids, offs, L, stride, bos, eos, pside, tside, dt), want, (bos, eos, pside, tside, dt, L, stride))
                n_cases += 1
    assert n_cases >= 4 * 4 * 2 * 3 * 2
    # the per-row form on the long row itself, at the window sizes where it owns whole tiles and where it does not
    for L, stride, (bos, eos), tside in [(1, 0, (None, None), "right"), (3, 0, (1, 2), "left"), (8, 3, (None, 2), "right"), (13, 12, (None, None), "left")]:
        ids, offs = _flat([2, LONG, 0, 5], rng)
        want = wc.windows_by_row(ids, offs, L, stride, PAD, bos, eos, False, tside == "left")
        _same(_twin(ids, offs, L, stride, bos, eos, "right", tside, np.int32), want, (L, stride))
    # no rows at all, and rows without a token
    got = _twin(np.zeros(0, np.uint32), np.zeros(1, np.uint64), 4, 1, 1, None, "right", "right", np.int32)
    assert got[0].shape == (0, 4) and got[3].shape == (0,)
    got = _twin(np.zeros(0, np.uint32), np.zeros(4, np.uint64), 4, 1, 1, None, "left", "right", np.int64)
    _same(got, wc.windows_by_row([], [0, 0, 0, 0], 4, 1, PAD, 1, None, True, False, np.int64), "empty rows")


def test_no_long_row_is_the_padded_form_and_window_0_is_the_padded_row():
    rng = np.random.default_rng(7)
    for (bos, eos), pside, tside, dt in itertools.product(BOS_EOS, SIDES, SIDES, [np.int32, np.int64]):
        a = _a(bos, eos)
        for L in _row_lens(a):
            room = L - a
            for stride in _strides(room):
                kw = dict(bos_id=bos, eos_id=eos, padding_side=pside, truncation_side=tside, dtype=dt)
                # (1) nothing longer than room: W = S and every output is the padded twin's
                ids, offs = _flat([0, room, room - 1, 1 if room > 1 else 0, 0, room, 0], rng)
                got = _twin(ids, offs, L, stride, bos, eos, pside, tside, dt)
                pad = _lib.layout_pad_host(ids, offs, L, PAD, **kw)
                S = len(offs) - 1
                assert got[0].shape[0] == S and pad["n_truncated"] == 0
                assert np.array_equal(got[0], pad["input_ids"]) and np.array_equal(got[1], pad["attention_mask"])
                assert np.array_equal(got[2], pad["lengths"]) and np.array_equal(got[3], np.arange(S)) and not got[4].any()
                # (2) any input: window k = 0 of row i is row i of the padded form
                ids, offs = _flat(_row_sizes(room, room - stride), rng)
                got = _twin(ids, offs, L, stride, bos, eos, pside, tside, dt)
                pad = _lib.layout_pad_host(ids, offs, L, PAD, **kw)
                w0 = np.flatnonzero(np.diff(got[3], prepend=-1))          # the first window of every row
                assert np.array_equal(got[3][w0], np.arange(len(offs) - 1))
                assert np.array_equal(got[0][w0], pad["input_ids"]) and np.array_equal(got[1][w0], pad["attention_mask"])
                assert np.array_equal(got[2][w0], pad["lengths"])
                assert pad["n_truncated"] == int((np.bincount(got[3]) > 1).sum())


class _Vocab:
    def __init__(self):
        self.tokens, self.specials = dc.mixed_tokens(), dc.MIXED_SPECIALS
        self.vf, self.vo = _lib.pack(self.tokens)
        self.sf, self.so = _lib.pack(self.specials)
        self.V, self.NS = len(self.tokens), len(self.specials)
        self.lookup = sc.vocab_lookup(self.tokens, self.specials)

    def windows(self, ids, offs, **kw):
        return _lib.window_spans_host(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, **kw)

    def padded(self, ids, offs, **kw):
        return _lib.spans_host(self.vf, self.vo, self.V, self.sf, self.so, self.NS, ids, offs, **kw)


@functools.lru_cache(maxsize=None)
def _vocab():
    return _Vocab()


def test_span_twin_against_the_checker_and_the_padded_twin():
    v = _vocab()
    rng = np.random.default_rng(8)
    for unit, (bos, eos), pside, tside, dt in itertools.product(["byte", "char"], BOS_EOS, SIDES, SIDES, [np.int32, np.int64]):
        a = _a(bos, eos)
        b, e = (None if bos is None else v.V), (None if eos is None else v.V + 3)    # two of the special tokens
        for L in _row_lens(a):
            room = L - a
            for stride in _strides(room):
                ids, offs = _flat(_row_sizes(room, room - stride, long_row=(L in (a + 1, 8) and dt == np.int32)), rng, hi=v.V + v.NS)
                ids[ids < 10] = 10
                kw = dict(unit=unit, dtype=dt, bos_id=b, eos_id=e, padding_side=pside, truncation_side=tside)
                got = v.windows(ids, offs, row_len=L, stride=stride, **kw)
                flat_spans = sc.flat(ids, offs, v.lookup, unit)
                want = wc.window_spans(offs, flat_spans, L, stride, b, e, pside == "left", tside == "left", dt)
                key = (unit, bos, eos, pside, tside, dt, L, stride)
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), key
                # the pairs line up with the ids of the same arguments: a kept token has its own span, the rest (0, 0)
                ids_w, mask_w, _, row_w, first_w = _twin(ids, offs, L, stride, b, e, pside, tside, dt)
                assert got.shape[:2] == ids_w.shape
                assert not got[mask_w == 0].any()
                # window 0 of every row is the padded twin's row
                w0 = np.flatnonzero(np.diff(row_w, prepend=-1))
                assert np.array_equal(got[w0], v.padded(ids, offs, row_len=L, **kw)), key
    # rows without a token: all (0, 0)
    out = v.windows(np.zeros(0, np.uint32), np.zeros(3, np.uint64), row_len=4, stride=2, dtype=np.int64)
    assert out.shape == (2, 4, 2) and not out.any()


# ---- errors: the status, and a poisoned destination that stays as it was ---------------------------------------------

def _raw_layout(ids, offs, L, stride, pad=PAD, bos=_lib.NO_ID, eos=_lib.NO_ID, flags=0, n_windows=0, room_for=64, want_out=True, count=True):
    """tgx_layout_windows_host itself -> (status, n_windows_out, destinations that were poisoned before the call)"""
    ids = np.ascontiguousarray(ids, np.uint32)
    offs = np.ascontiguousarray(offs, np.uint64)
    out = np.full(room_for * max(L, 1), POISON, np.int64)
    mask = np.full(room_for * max(L, 1), 9, np.uint8)
    i32 = [np.full(room_for, POISON, np.int32) for _ in range(3)]
    got = C.c_uint64(12345)
    st = _lib.lib.tgx_layout_windows_host(_lib.ptr(ids) if ids.size else None, _lib.ptr(offs), len(offs) - 1, L, stride, pad, bos, eos, flags,
                                          n_windows, _lib.ptr(out) if want_out else None, _lib.ptr(mask), *[_lib.ptr(x) for x in i32],
                                          C.byref(got) if count else None)
    return st, got.value, [out, mask] + i32


def _untouched(dests):
    return all((d == (9 if d.dtype == np.uint8 else POISON)).all() for d in dests)


def test_errors_leave_the_destinations_untouched():
    ids, offs = np.arange(10, 30, dtype=np.uint32), np.array([0, 3, 3, 20], np.uint64)
    W = wc.n_windows(offs, 5, 1, 1, None)
    st, got, dests = _raw_layout(ids, offs, 5, 1, bos=1, n_windows=W)       # the good call first
    assert st == _lib.OK and got == W and not _untouched(dests)
    bad = [dict(L=0, stride=0), dict(L=2, stride=0, bos=1, eos=2),          # no room for a token
           dict(L=5, stride=5), dict(L=5, stride=4, bos=1), dict(L=5, stride=3, bos=1, eos=2), dict(L=1, stride=1),   # stride >= room
           dict(L=5, stride=2**32 - 1),
           dict(L=5, stride=1, flags=64), dict(L=5, stride=1, flags=_lib.SPAN_CHARS),
           dict(L=5, stride=1, pad=2**31), dict(L=5, stride=1, bos=2**31), dict(L=5, stride=1, eos=2**31 + 5),
           dict(L=5, stride=1, bos=1, n_windows=W + 1), dict(L=5, stride=1, bos=1, n_windows=W - 1), dict(L=5, stride=1, bos=1, n_windows=0),
           dict(L=5, stride=1, count=False)]
    for kw in bad:
        st, _, dests = _raw_layout(ids, offs, **kw)
        assert st == _lib.ERR_INVALID and _untouched(dests), kw
    # a NULL destination only asks for W, whatever n_windows says
    st, got, dests = _raw_layout(ids, offs, 5, 1, bos=1, n_windows=999, want_out=False)
    assert st == _lib.OK and got == W and _untouched(dests)
    # offsets that go down, and ids that are missing
    assert _raw_layout(ids, np.array([0, 5, 3], np.uint64), 5, 1)[0] == _lib.ERR_INVALID
    assert _raw_layout(np.zeros(0, np.uint32), offs, 5, 1)[0] == _lib.ERR_INVALID
    # the limits: a row of 2^31 tokens, and 2^31 windows (nothing is read or written before they are refused)
    st, _, dests = _raw_layout(ids, np.array([0, 2**31], np.uint64), 5, 1, want_out=False)
    assert st == _lib.ERR_UNSUPPORTED and _untouched(dests)
    st, _, dests = _raw_layout(ids, np.array([0, 2**31 - 1], np.uint64), 2, 1, want_out=False)
    assert st == _lib.OK                                                    # 2^31 - 2 windows
    st, _, dests = _raw_layout(ids, np.array([0, 2**31 - 1, 2**32 - 2], np.uint64), 2, 1, n_windows=2**32 - 4)
    assert st == _lib.ERR_UNSUPPORTED and _untouched(dests)
    # an id that is not below 2^31 is refused when it is reached
    big = ids.copy()
    big[12] = 2**31
    assert _raw_layout(big, offs, 5, 1, n_windows=wc.n_windows(offs, 5, 1))[0] == _lib.ERR_INVALID
    # the wrappers raise what the ABI returns
    with pytest.raises(_lib.TokenGeeXError) as e:
        _lib.layout_windows_host(ids, offs, 5, 5, PAD)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.TokenGeeXError) as e:
        _lib.layout_windows_host(ids, offs, 5, 1, PAD, n_windows=3)
    assert e.value.status == _lib.ERR_INVALID


def test_span_twin_errors():
    v = _vocab()
    ids, offs = np.arange(10, 30, dtype=np.uint32), np.array([0, 3, 3, 20], np.uint64)
    W = wc.n_windows(offs, 5, 1)

    def raw(L, stride, bos=_lib.NO_ID, eos=_lib.NO_ID, flags=0, n_windows=W, i=ids, want_out=True):
        out = np.full((64, max(L, 1), 2), POISON, np.int64)
        got = C.c_uint64(0)
        st = _lib.lib.tgx_window_spans_host(_lib.ptr(v.vf), _lib.ptr(v.vo), v.V, _lib.ptr(v.sf), _lib.ptr(v.so), v.NS, _lib.ptr(i), _lib.ptr(offs), 3, L,
                                            stride, bos, eos, flags | _lib.LAYOUT_I64, n_windows, _lib.ptr(out) if want_out else None, C.byref(got))
        return st, got.value, out

    st, got, out = raw(5, 1)
    assert st == _lib.OK and got == W and (out[:W] != POISON).all() and (out[W:] == POISON).all()
    assert raw(5, 1, n_windows=77, want_out=False)[:2] == (_lib.OK, W)
    for kw in [dict(L=0, stride=0), dict(L=5, stride=5), dict(L=2, stride=0, bos=v.V, eos=v.V), dict(L=5, stride=1, flags=64),
               dict(L=5, stride=1, bos=2**31), dict(L=5, stride=1, n_windows=W + 1), dict(L=5, stride=1, n_windows=0)]:
        st, _, out = raw(**kw)
        assert st == _lib.ERR_INVALID and (out == POISON).all(), kw
    oob = ids.copy()
    oob[4] = v.V + v.NS
    st, _, out = raw(5, 1, i=oob)
    assert st == _lib.ERR_TOKEN_ID_OOB and (out == POISON).all()
    with pytest.raises(_lib.TokenGeeXError) as e:
        v.windows(oob, offs, row_len=5, stride=1)
    assert e.value.status == _lib.ERR_TOKEN_ID_OOB and e.value.sample == 2


# ---- HuggingFace tokenizers: truncation with a stride, both directions -----------------------------------------------

def test_window_rule_is_huggingface_truncation_with_stride():
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import WhitespaceSplit
    N = 40
    tk = tokenizers.Tokenizer(WordLevel({f"t{j}": j for j in range(N)}, unk_token="t0"))
    tk.pre_tokenizer = WhitespaceSplit()
    texts = [" ".join(f"t{j}" for j in range(n)) for n in range(N)]
    ids, offs = np.concatenate([np.arange(n, dtype=np.uint32) for n in range(N)]), np.cumsum([0] + list(range(N))).astype(np.uint64)
    n_cases = 0
    for direction, room in itertools.product(SIDES, range(1, 9)):
        for stride in range(room):          # (stride >= max_length makes HF panic: the TGX_ERR_INVALID case)
            tk.enable_truncation(max_length=room, stride=stride, direction=direction)
            hf = []
            for n in range(N):
                enc = tk.encode(texts[n])
                hf.append([list(enc.ids)] + [list(o.ids) for o in enc.overflowing])
            out, mask, lengths, row, first = _twin(ids, offs, room, stride, None, None, "right", direction, np.int32)
            for n in range(N):
                mine = [out[w, :lengths[w]].tolist() for w in np.flatnonzero(row == n)]
                assert mine == hf[n], (direction, room, stride, n)
                assert mine == [list(range(f, f + k)) for f, k in wc.row_windows(n, room, stride, direction == "left")]
                n_cases += 1
    assert n_cases == 2 * 1440
