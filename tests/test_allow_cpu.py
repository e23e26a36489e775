"""The allow filter of the document-frequency pass without a device (include/tgx_allow.h): the host twin, which walks the
kernels' header (csrc/allow.h), against the per-position reference of tests/allow_cases.py on every geometry of
tests/generate_cases.py; the header's table, the 37-state fixture, BytePattern.fullmatch and the refusals.  All integer
work, compared exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib
from tokengeex_amd.generate import VocabularyGenerator

import allow_cases as ac
import generate_cases as gc


@pytest.mark.parametrize("prob", [1.0, 0.3])
@pytest.mark.parametrize("mtl", [1, 7, 32])
@pytest.mark.parametrize("which", ["A", "B"])
def test_twin_equals_reference(which, mtl, prob):
    for name in gc.GEOMETRY_NAMES:
        c = gc.case(name)
        flat, pb, pe, ps, po = gc.arrays(c)
        want_mask, _, want_windows = ac.reference(c, which, mtl, prob, 9)
        mask, n_windows = _lib.allow_masks_host(flat, pb, pe, ps, mtl, ac.automaton(which), prob, 9, part_origin=po)
        assert np.array_equal(mask, want_mask) and n_windows == want_windows, name


@pytest.mark.parametrize("which", ["A", "B"])
def test_twin_on_the_chunk_edges(which):
    for c in ac.chunk_cases():
        flat, pb, pe, ps, po = gc.arrays(c)
        want_mask, _, want_windows = ac.reference(c, which, 32)
        mask, n_windows = _lib.allow_masks_host(flat, pb, pe, ps, 32, ac.automaton(which))
        assert np.array_equal(mask, want_mask) and n_windows == want_windows and (mask >> 31).any(), c["name"]  # (walks live to 32 bytes)


def test_placed_parts_hash_the_offset_in_the_sample():
    c = gc.place((0, 3, 5), 33, 7)
    flat, pb, pe, ps, po = gc.arrays(c)
    want_mask, _, want_windows = ac.reference(c, "A", gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED)
    mask, n_windows = _lib.allow_masks_host(flat, pb, pe, ps, gc.PLACE_MTL, ac.automaton("A"), gc.PLACE_PROB, gc.PLACE_SEED, part_origin=po)
    assert np.array_equal(mask, want_mask) and n_windows == want_windows and 0 < n_windows


def test_header_and_symbol_table_agree():
    """every function the header declares is in ALLOW_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ac.ROOT, "include", "tgx_allow.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS") and name != "ALLOW_SYMBOLS"]
    assert declared == set(_lib.ALLOW_SYMBOLS) and not any(declared & set(t) for t in others) and all(hasattr(_lib.lib, name) for name in declared)


def test_the_fixture_fits_and_fullmatch_walks_it():
    small, exact = ac.automaton("A"), ac.automaton("B")
    assert exact.n_states == 37 and small.n_states <= 16 and small.next.shape == (256, 16)
    for data, want in [(b"return", True), (b"Return", True), (b"RETURN", True), (b"reTurn", False), (b" +=", True), (b"+= ", True), (b" += x", False),
                       (b"'ll", True), (b"    ", True), (b" \t", False), ("中文".encode(), True), ("é".encode(), True), (b"\n", False), (b":\n", False),
                       (b":", True), (b"", False), (b"ab", True)]:
        assert exact.fullmatch(data) is want and ac.allows(exact, data) is want, data
    assert small.fullmatch(b"abba") and small.fullmatch(" éé".encode()) and not small.fullmatch(b"abc") and not small.fullmatch("𝒳".encode())


def test_refusals():
    c = gc.case("gaps")
    flat, pb, pe, ps, _ = gc.arrays(c)
    good, empty = _lib.dfa64_struct(ac.automaton("A")), _lib.dfa64_struct(ac.automaton("A"))
    empty.tag[empty.start] = 1
    mask = np.full(flat.size, 7, np.uint32)
    outs = [ctypes.c_void_p() for _ in range(3)] + [ctypes.c_uint64() for _ in range(4)] + [ctypes.c_uint32()]

    def twin(d, mtl):
        return _lib.lib.tgx_allow_masks_host(_lib.ptr(flat), flat.size, _lib.ptr(pb), _lib.ptr(pe), _lib.ptr(ps), None, pb.size, mtl, 1.0, 0,
                                             None if d is None else ctypes.byref(d), _lib.ptr(mask), None)

    def device(d, mtl):  # (refused before a device is asked for)
        return _lib.lib.tgx_substring_df_allow(0, _lib.ptr(flat), flat.size, _lib.ptr(pb), _lib.ptr(pe), _lib.ptr(ps), None, pb.size, mtl, 1.0, 0,
                                               None if d is None else ctypes.byref(d), 0, *(ctypes.byref(o) for o in outs))

    for call in (twin, device):
        assert call(None, 8) == call(empty, 8) == _lib.ERR_INVALID and call(good, 0) == call(good, 33) == _lib.ERR_UNSUPPORTED
    assert (mask == 7).all() and twin(good, 32) == _lib.OK and not (mask == 7).all()
    for kind in (dict(find=True), dict(cover=True)):
        with pytest.raises(ValueError, match="anchored"):
            VocabularyGenerator(8, 1.0, allow=tgx.compile_pattern("ab+", **kind))
