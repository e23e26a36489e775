"""Byte patterns of up to 64 states without a device: the host twin (tgx_dfa64_hits_host: the kernels' chunks, segments,
row-start masks, fold, scan, chain and store / add rule through csrc/dfa64.h) against the header's definition, the
compiler's max_states=64 against Python's re on the small cases, and the refusals.  The case table is
tests/patterns64_cases.py.  Everything is integer work and compared exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from patterns64_cases import AUTOMATA, CASE_IDS, CASES, N_SEAMS, PHONE_17, SEAMS, SMALL, pattern, text, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_twin_equals_the_reference(case):
    flat, offs = text(case)
    count, ends = _lib.dfa64_hits_host(flat, offs, pattern(case[0]))
    assert np.array_equal(count, want(case)[0]) and np.array_equal(ends, want(case)[1])
    if pattern(case[0]).n_states <= 16:  # through the 16-state call the same automaton gives the same answers
        old = _lib.dfa_hits_host(flat, offs, pattern(case[0]))
        assert np.array_equal(old[0], count) and np.array_equal(old[1], ends)


def test_the_table_holds_what_it_is_for():
    assert want(("a{63}", "long_row"))[0].tolist() == [66_000 - 62] and pattern("a{63}").next.max() == 63, "state 63 is in use"
    for a in AUTOMATA:
        assert want((a, "edges"))[0].tolist() == [0, 1, 1, 2] and want((a, "rows"))[0].tolist() == [0, 0, 1, 0, 0, 0, 0, a == "two_tags", 0, 0, 1, 0], a  # (its four digits alone survive the cut)
    assert want(("two_tags", "rows"))[1].max() == 3 and want(("phone17", "no_bytes"))[0].tolist() == [0, 0, 0]
    flat, offs = text(("phone17", "seams"))
    assert flat.size == N_SEAMS and all(want(("phone17", "seams"))[1][min(s + 8, N_SEAMS - 1)] == 1 for s in SEAMS)
    assert 0 in np.diff(offs) and np.diff(offs).max() > 60_000


@pytest.mark.parametrize("case", SMALL, ids=[f"{p}-{t}" for p, t in SMALL])
def test_compiler_against_re(case):
    """bit k at end j iff some s <= j has re.fullmatch(pattern k, row[s : j + 1])"""
    flat, offs = text(case)
    regs = [re.compile(p.encode()) for p in AUTOMATA[case[0]][0]]
    for i in range(len(offs) - 1):
        row = bytes(flat[int(offs[i]):int(offs[i + 1])])
        got = want(case)[1][int(offs[i]):int(offs[i + 1])].tolist()
        for j in range(len(row)):
            assert got[j] == sum(1 << k for k, r in enumerate(regs) if any(r.fullmatch(row, s, j + 1) for s in range(j + 1))), (case, i, j)


def test_max_states_counts_and_refuses():
    wide = tgx.compile_pattern(PHONE_17, max_states=64)
    assert wide.next.shape == (256, 64) and wide.tag.shape == (64,) and tgx.compile_pattern("ab", max_states=64).next.shape == (256, 16)
    with pytest.raises(ValueError, match="65 states"):
        tgx.compile_pattern("a{64}", max_states=64)
    with pytest.raises(ValueError, match="17 states"):
        tgx.compile_pattern(PHONE_17)
    for bad in (0, 17, 32, 65, 128):
        with pytest.raises(ValueError, match="max_states"):
            tgx.compile_pattern("ab", max_states=bad)
    with pytest.raises(ValueError, match="cover=True keeps"):
        tgx.compile_pattern("ab", cover=True, max_states=64)


def test_bad_automata_are_refused_with_nothing_written():
    flat, offs = text(("ab", "rows"))
    count, ends = np.full(len(offs) - 1, -7, np.int64), np.full(flat.size, 7, np.uint8)

    def call(d, c=count, e=ends):
        return _lib.lib.tgx_dfa64_hits_host(_lib.ptr(flat), _lib.ptr(offs), len(offs) - 1, ctypes.byref(d) if d else None, _lib.ptr(c) if c is not None else None,
                                            _lib.ptr(e) if e is not None else None)

    def broken(**fields):
        d = _lib.dfa64_struct(pattern("ab"))
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    bad_next, bad_tag = broken(), broken()
    bad_next.next[200][2] = 3
    bad_tag.tag[pattern("ab").start] = 1
    for d in (broken(n_states=0), broken(n_states=65), broken(start=3), bad_next, bad_tag, None):
        assert call(d) == _lib.ERR_INVALID and "tgx_dfa64_hits_host" in _lib.lib.tgx_last_error().decode()
    assert call(broken(), None, None) == _lib.ERR_INVALID
    assert (count == -7).all() and (ends == 7).all()
    spare = broken()
    spare.next[200][63] = 99  # an entry at or above n_states is ignored
    assert call(spare) == _lib.OK and np.array_equal(count, want(("ab", "rows"))[0])


def test_header_and_symbol_table_agree():
    """every function the header declares is in PATTERN64_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_patterns64.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    assert declared == set(_lib.PATTERN64_SYMBOLS) and not declared & (set(_lib.SYMBOLS) | set(_lib.PATTERN_SYMBOLS))
    assert ctypes.sizeof(_lib.TgxDfa64) == 8 + 256 * 64 + 64 and _lib.lib.tgx_abi_version() == 1
