"""The host twin of the device front end (tgx_front_host: the kernels' tiles, thread slots and index arithmetic of
csrc/front.h on host memory) against the host route, split_specials_flat + pack_segments.  Everything is compared exactly:
this is byte and integer movement.  No device is needed."""
import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import front_cases as fc


def _check(samples, specials, crlf, key):
    want = fc.truth(samples, specials, crlf)
    flat, offs = _lib.pack(samples)
    got = _lib.front_host(flat, offs, specials, crlf)
    for name, w, g in zip(("seg_offs", "seg_special", "segments' bytes", "segments' offsets"), want, got):
        assert w.dtype == g.dtype and np.array_equal(w, g), (key, crlf, name)


@pytest.mark.parametrize("crlf", [False, True])
def test_fixed_cases(crlf):
    names = set()
    for name, samples, specials in fc.fixed_cases():
        assert name not in names
        names.add(name)
        _check(samples, specials, crlf, name)


def test_past_cap_corpus_reaches_every_threshold():
    """the arithmetic of csrc/front.hip's launchers on the corpus, from the mirrored constants, and the twin on it"""
    cap, tile, slot, block = 4096, 4096, 16, 256     # kFrontMaxBlocks, kFrontTile, kFrontGroup, kFrontBlock
    flat, offs, specials = fc.past_cap_corpus()
    n, S = flat.size, offs.size - 1
    n_tiles = -(-n // tile)
    lens = np.diff(offs.astype(np.int64))
    begin = offs[:-1].astype(np.int64)
    assert n > cap * tile + 2 * tile and n_tiles > cap and S > block * cap
    for crlf in (False, True):
        want = fc.truth_flat(flat, offs, specials, crlf)
        got = _lib.front_host(flat, offs, specials, crlf)
        for name, w, g in zip(("seg_offs", "seg_special", "segments' bytes", "segments' offsets"), want, got):
            assert w.dtype == g.dtype and np.array_equal(w, g), (crlf, name)
        seg_offs, ss, pflat, poffs = want
        accepted, n_enc = int((ss >= 0).sum()), poffs.size - 1     # (every accepted special was a candidate)
        print(f"crlf {crlf}: bytes {n}, tiles {n_tiles}, rows {S}, accepted candidates {accepted}, segments {ss.size}, to encode {n_enc}")
        assert accepted > block * cap and ss.size > block * cap and n_enc + 1 > block * cap
    # the two rows of three tiles lie in the second trip's tiles, each over at least two whole tiles
    long = np.flatnonzero(lens == 3 * tile)
    assert long.size == 2 and begin[long[0]] >= cap * tile and lens.max() == 3 * tile
    plain, only = (flat[begin[k]:begin[k] + lens[k]].tobytes() for k in long)
    assert not {sp[0] for sp in specials} & set(plain) and only == b"<s>" * tile
    seg_offs, ss, _, _ = fc.truth_flat(flat, offs, specials, False)
    assert seg_offs[long[0] + 1] - seg_offs[long[0]] == 1 and (ss[int(seg_offs[long[1]]):int(seg_offs[long[1] + 1])] == 1).all()
    # over the rounds, the row that is one 11-byte special begins at every byte of a slot and at the last ten of a tile
    starts = begin[np.flatnonzero(lens == fc.M)]
    assert all(flat[b:b + fc.M].tobytes() == fc.SP for b in starts[:50])
    assert set(starts % slot) == set(range(slot)) and set(range(tile - 10, tile)) <= set(starts % tile)
    cr = np.flatnonzero((flat[:-1] == 13) & (flat[1:] == 10))
    assert (cr % slot == slot - 1).any() and (cr % tile == tile - 1).any() and np.isin(cr + 1, begin).any()
    assert (lens == 0).sum() > S // 8 and {len(r) for r in fc.PAST_POOL} >= {0, 3, fc.M}


def test_the_cases_say_what_they_are_meant_to():
    """the ground truth itself, on the cases whose outcome the split rule states in words"""
    assert fc.segments([b"ababababa"], [b"aba"]) == [[(b"aba", 0), (b"b", -1), (b"aba", 0), (b"ba", -1)]]
    assert fc.segments([b"x<abx"], [b"<a", b"<ab"]) == [[(b"x", -1), (b"<a", 0), (b"bx", -1)]]
    assert fc.segments([b"x<abx"], [b"<ab", b"<a"]) == [[(b"x", -1), (b"<ab", 0), (b"x", -1)]]
    assert fc.segments([b"ababa"], [b"ab", b"ba"]) == [[(b"ab", 0), (b"ab", 0), (b"a", -1)]]
    assert fc.segments([b"aaaaa"], [b"aa"]) == [[(b"aa", 0), (b"aa", 0), (b"a", -1)]]
    for j in range(1, fc.M):   # a special never matches across a sample's end
        assert fc.segments([b"ab" + fc.SP[:j], fc.SP[j:] + b"cd"], [fc.SP]) == [[(b"ab" + fc.SP[:j], -1)], [(fc.SP[j:] + b"cd", -1)]]
    # a '\r' that ends a segment is kept and the special behind it matched; a '\r' and a '\n' of two samples are both kept
    assert fc.segments([b"ab\r\n<x>cd"], [b"\n<x>"], True) == [[(b"ab\r", -1), (b"\n<x>", 0), (b"cd", -1)]]
    assert fc.segments([b"ab\r", b"\ncd"], [b"<s>"], True) == [[(b"ab\r", -1)], [(b"\ncd", -1)]]
    assert fc.segments([b"a\r\r\nb", b"\r\n\r\n"], [], True) == [[(b"a\r\nb", -1)], [(b"\n\n", -1)]]
    assert fc.segments([b"a<\r\n>b\r\n"], [b"<\r\n>"], True) == [[(b"a", -1), (b"<\r\n>", 0), (b"b\n", -1)]]


def test_random_small_batches():
    rng = np.random.default_rng(20240607)
    seen_specials = seen_crlf = 0
    for it in range(200):
        samples, specials = fc.random_batch(rng)
        assert sum(len(s) for s in samples) <= 64 << 10
        crlf = bool(it & 1)
        _check(samples, specials, crlf, ("random", it))
        seen_specials += int((fc.truth(samples, specials, crlf)[1] >= 0).sum())
        seen_crlf += sum(s.count(b"\r\n") for s in samples)
    assert seen_specials > 1000 and seen_crlf > 1000   # the batches do exercise the split and the CRLF pass


def test_argument_checks():
    flat, offs = _lib.pack([b"ab<s>", b"cd"])

    def refused(flat_, offs_, specials, status=_lib.ERR_INVALID):
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.front_host(flat_, offs_, specials, True)
        assert e.value.status == status, e.value
        return str(e.value)

    bad = offs.copy()
    bad[0] = 1
    assert "offs[0]" in refused(flat, bad, [b"<s>"])
    bad = offs.copy()
    bad[1], bad[2] = offs[2], offs[1]
    assert "monotone" in refused(flat, bad, [b"<s>"])
    # an empty special token: the host function's refusal, word for word
    with pytest.raises(tgx.TokenGeeXError) as want:
        _lib.split_specials_flat(flat, offs, [b"<s>", b""])
    assert refused(flat, offs, [b"<s>", b""]) == str(want.value) and want.value.status == _lib.ERR_INVALID
    # NULL outputs and unknown flags, through the C ABI
    import ctypes as C
    so = np.zeros(3, np.uint64)
    ss, ot, oo, k, e = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    soffs = np.zeros(1, np.uint64)
    args = [_lib.ptr(flat), _lib.ptr(offs), 2, None, _lib.ptr(soffs), 0, 0, _lib.ptr(so), C.byref(ss), C.byref(k), C.byref(ot), C.byref(oo), C.byref(e)]
    assert _lib.lib.tgx_front_host(*args) == _lib.OK and k.value == 2 and e.value == 2
    for p in (ss, ot, oo):
        _lib.lib.tgx_free(p)
    for hole in (7, 8, 9, 10, 11, 12):
        a = list(args)
        a[hole] = None
        assert _lib.lib.tgx_front_host(*a) == _lib.ERR_INVALID, hole
    a = list(args)
    a[6] = 2
    assert _lib.lib.tgx_front_host(*a) == _lib.ERR_INVALID
    a = list(args)
    a[0] = None
    assert _lib.lib.tgx_front_host(*a) == _lib.ERR_INVALID   # text is NULL although there are bytes
    # no samples, and samples without bytes
    got = _lib.front_host(np.zeros(0, np.uint8), np.zeros(1, np.uint64), [b"<s>"], True)
    assert [x.tolist() for x in got] == [[0], [], [], [0]]
    got = _lib.front_host(np.zeros(0, np.uint8), np.zeros(4, np.uint64), [b"<s>"], False)
    assert [x.tolist() for x in got] == [[0, 0, 0, 0], [], [], [0]]


def test_the_limits_on_the_special_tokens():
    """1024 special tokens and 32 KiB of them are taken; beyond 4096 tokens or 64 KiB the twin refuses as the device entry
    point does (the kernels' tables), with TGX_ERR_UNSUPPORTED"""
    specials = [b"<%04d|" % k + b"x" * 26 for k in range(1024)]   # 1024 x 32 bytes = 32 KiB
    samples = [b"ab" + specials[1023] + b"cd" + specials[0] + specials[512][:-1], specials[7]]
    want = fc.truth(samples, specials, False)
    got = _lib.front_host(*_lib.pack(samples), specials, False)
    assert all(np.array_equal(w, g) for w, g in zip(want, got)) and want[1].tolist() == [-1, 1023, -1, 0, -1, 7]
    flat, offs = _lib.pack([b"abc"])
    for too_many in ([b"<%05d>" % k for k in range(4097)], [b"<%d>" % k + b"y" * 700 for k in range(100)]):
        with pytest.raises(tgx.TokenGeeXError) as e:
            _lib.front_host(flat, offs, too_many, False)
        assert e.value.status == _lib.ERR_UNSUPPORTED and "special tokens" in str(e.value)
    at_the_limit = [b"<%05d>" % k for k in range(4096)]
    assert _lib.front_host(flat, offs, at_the_limit, False)[1].tolist() == [-1]
