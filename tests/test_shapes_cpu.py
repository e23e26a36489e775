"""Shapes without a device (include/tgx_shapes.h): the host twins, which walk the kernels' chunks, halo, doubling steps,
guards and windows through csrc/shape.h, against the header's definition in plain Python on the case table of
tests/shape_cases.py; compile_shapes against re; every refusal of compiler and ABI; the header against the symbol table.
Everything is compared exactly: this is integer work."""
import ctypes
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from shape_cases import CASE_IDS, CASES, SETS, SMALL, TWO_TILES, reference, shapes, text, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_twins_equal_the_reference(case):
    flat, offs = text(case[1])
    count, ends = _lib.shape_hits_host(flat, offs, shapes(case[0]))
    covered, mask = _lib.shape_cover_host(flat, offs, shapes(case[0]))
    for got, wanted in zip((count, ends, covered, mask), want(case)):
        assert np.array_equal(got, wanted)


def test_the_table_holds_what_it_is_for():
    ends = {c: np.flatnonzero(want(c)[1]).tolist() for c in CASES}
    assert ends["l64", "edges"] == [63, 192, 318, 463] and ends["l64", "edges_one_row"] == [63, 192, 318, 463, 563]
    assert want(("l63", "edges"))[0].tolist() == [6, 2, 1] and want(("l64x2", "edges"))[1][[63, 192, 318, 463]].tolist() == [3] * 4
    assert want(("l40x2", "edges"))[1][[39, 63, 192]].tolist() == [3] * 3 and want(("three", "edges"))[1][318] == 7
    assert want(("l64", "edges"))[3][[254, 255, 318, 319]].tolist() == [0, 1, 1, 0], "lane 63 is covered by the end on lane 62 of the next chunk"
    assert want(("a4", "a6"))[0].tolist() == [3] and want(("a4", "a6"))[3].tolist() == [1] * 6
    assert want(("adjacent", "empties"))[1].tolist() == [0, 7, 2, 0, 0, 0, 7] and want(("one", "empties"))[0].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 1, 0]
    # the guarded copy is bit 0: of the 9-byte runs it takes nothing, of the 8-byte ones all four
    assert [(p, int(want(("guarded", "guards"))[1][p])) for p in ends["guarded", "guards"]] == [(70, 2), (71, 2), (135, 3), (191, 2), (192, 2), (255, 3), (263, 3), (299, 3)]
    assert want(("bytes", "all_bytes"))[0].tolist() == [260] and want(("bytes", "all_bytes"))[1][[0, 1, 2, 3, 4]].tolist() == [2, 2, 2, 3, 4]
    keys = want(("keys", "two_tiles"))[1]
    assert text("two_tiles")[0].size == TWO_TILES and [int(keys[p]) for p in (219, 265, 285, 531, 1026 * 256 + 23, TWO_TILES - 1)] == [1, 1, 1, 4, 2, 2]
    assert want(("l64x2", "two_tiles"))[1][803] == 3 and all(want((s, "mixed"))[0].any() for s in ("eight", "adjacent", "three", "a4"))


@pytest.mark.parametrize("case", SMALL, ids=[f"{s}-{t}" for s, t in SMALL])
def test_compiler_against_re(case):
    """the guards as look-behind and look-ahead, every overlapping match through a look-ahead group, row by row"""
    flat, offs = text(case[1])
    got = np.zeros(flat.size, np.uint8)
    for k, p in enumerate(SETS[case[0]]):
        pat, before, after = p if isinstance(p, tuple) else (p, "", "")
        reg = re.compile(((f"(?<!{before})" if before else "") + f"(?=({pat})" + (f"(?!{after})" if after else "") + ")").encode())
        for r0, r1 in zip(offs[:-1].tolist(), offs[1:].tolist()):
            for m in reg.finditer(bytes(flat[r0:r1])):
                got[r0 + m.end(1) - 1] |= 1 << k
    assert np.array_equal(got, want(case)[1])


def test_compiler_folds_and_refuses():
    folded = tgx.compile_shapes([("ab[c-d]", "[x]", "")], fold_case=True)
    assert reference(folded, *tgx.pack([b"yAbD", b"XaBc", b"abe"]))[0].tolist() == [1, 0, 0]
    for bad, name in (("a|b", "alternation"), ("ab*", r"quantifier \*"), ("a+", r"quantifier \+"), ("a?b", r"quantifier \?"), ("a{2,3}", r"\{2,3\}"),
                      ("a{2,}", r"\{2,\}"), ("(ab){2}", "group around 2 atoms"), ("x(ab)", "group around 2 atoms"), ("a{65}", "65"), ("a{0}", "length of 0"),
                      ([("a", "ab", "")], "guard"), (["a"] * 9, "9 patterns"), (["a{64}", "a{64}", "a"], "129 positions"), ("^a", "anchor")):
        with pytest.raises(ValueError, match=name) as err:
            tgx.compile_shapes(bad)
        assert name in ("guard", "9 patterns", "129 positions", "anchor") or "fixed-length sequence of byte classes" in str(err.value) or "1 to 64" in str(err.value)
    assert tgx.compile_shapes("(a){3}[b-c]").len[:1].tolist() == [4]
    for served in ("AKIA[0-9A-Z]{16}", "ghp_[0-9a-zA-Z]{36}", "[0-9a-f]{32}"):  # what the automata of 16 states refuse
        with pytest.raises(ValueError, match="states"):
            tgx.compile_pattern(served)
        assert tgx.compile_shapes(served).n_patterns == 1


def test_bad_shapes_are_refused_with_nothing_written():
    flat, offs = text("empties")
    count, ends = np.full(len(offs) - 1, -7, np.int64), np.full(flat.size, 7, np.uint8)

    def broken(**fields):
        d = _lib.shapes_struct(shapes("adjacent"))
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    long_sum, empty_class, zero_len, long_len = broken(n_patterns=3), broken(), broken(), broken()
    ctypes.memset(long_sum.cls, 0xFF, ctypes.sizeof(long_sum.cls))
    long_sum.len[0], long_sum.len[1], long_sum.len[2] = 64, 64, 1
    ctypes.memset(empty_class.cls[3], 0, 32)
    zero_len.len[1], long_len.len[2] = 0, 65
    for fn in (_lib.lib.tgx_shape_hits_host, _lib.lib.tgx_shape_cover_host):
        def call(d, c=count, e=ends):
            return fn(_lib.ptr(flat), _lib.ptr(offs), len(offs) - 1, ctypes.byref(d) if d else None, _lib.ptr(c) if c is not None else None,
                      _lib.ptr(e) if e is not None else None)
        for d in (broken(n_patterns=0), broken(n_patterns=9), long_sum, empty_class, zero_len, long_len, None):
            assert call(d) == _lib.ERR_INVALID and "tgx_shape_" in _lib.lib.tgx_last_error().decode()
        assert call(broken(), None, None) == _lib.ERR_INVALID
        assert (count == -7).all() and (ends == 7).all()
    spare = broken()
    spare.len[5] = 99  # an entry beyond those in use is ignored
    assert _lib.lib.tgx_shape_hits_host(_lib.ptr(flat), _lib.ptr(offs), len(offs) - 1, ctypes.byref(spare), _lib.ptr(count), None) == _lib.OK
    assert np.array_equal(count, want(("adjacent", "empties"))[0]) and (ends == 7).all()


def test_header_and_symbol_table_agree():
    """every function the header declares is in SHAPE_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_shapes.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    assert declared == set(_lib.SHAPE_SYMBOLS) and not declared & (set(_lib.SYMBOLS) | set(_lib.PATTERN_SYMBOLS) | set(_lib.REDACT_SYMBOLS))
    assert ctypes.sizeof(_lib.TgxShapes) == 4 + 8 * 4 + 128 * 32 + 2 * 8 * 32
    import tokengeex
    assert all(getattr(tokengeex, n) is getattr(tgx, n) for n in ("compile_shapes", "ShapePattern", "shape_hits", "shape_rows", "shape_cover"))
