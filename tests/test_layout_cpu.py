"""Padded and packed layouts without a GPU: the host twins (tgx_layout_pad_host / tgx_layout_pack_host), which go
through the row mapping of csrc/layout.h that the kernels of csrc/layout.hip use, against the plain-numpy checker
(tests/layout_checker.py) over a grid of shapes and options; the checker itself against hand-written cases; every
error case, NULL handed to the device entry points included; and `import tokengeex_amd` staying torch-free."""
import ctypes as C
import itertools
import subprocess
import sys

import numpy as np
import pytest

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import layout_checker as lc

PAD = 9
BOS_EOS = [(None, None), (1, None), (None, 2), (1, 2)]


def _offs(lens):
    o = np.zeros(len(lens) + 1, np.uint64)
    if len(lens):
        np.cumsum(np.asarray(lens, np.uint64), out=o[1:])
    return o


def _case(lens, seed=0):
    rng = np.random.default_rng(seed)
    offs = _offs(lens)
    ids = rng.integers(10, 60000, size=int(offs[-1]), dtype=np.uint32)
    return ids, offs


def _inputs():
    rng = np.random.default_rng(7)
    cases = {
        "S0": [],
        "S1": [5],
        "S1_empty": [0],
        "all_empty": [0, 0, 0],
        "plain": [3, 1, 4, 1, 5],
        "empty_rows": [2, 0, 3, 0, 1],
        "empty_runs": [0, 0, 0, 4, 0, 0, 6, 2, 0, 0, 0, 0, 3, 0, 0],   # runs at the start, in the middle and at the end
        "one_long": [1, 3000, 2],                                      # a row that spans several 1024-element tiles
        "random": rng.integers(0, 40, size=200).tolist(),
        "random_sparse": (rng.integers(0, 6, size=3000) * (rng.random(3000) < 0.3)).astype(int).tolist(),  # mostly empty: tiles of many rows
    }
    return {k: _case(v, seed=i) for i, (k, v) in enumerate(cases.items())}


INPUTS = _inputs()


def _row_lens(offs, a):
    """L in {1 (if allowed), A, shorter than most rows, exactly max_row_len, longer}"""
    n = np.diff(offs.astype(np.int64))
    mx = (int(n.max()) if n.size else 0) + a
    short = max(1, a, (int(np.median(n)) if n.size else 0) // 2 + a)
    return sorted({max(1, a), short, max(1, mx), max(1, mx) + 3})


# ---- the checker is pinned by hand-written cases -------------------------------------------------------------

def test_checker_hand_cases():
    ids = np.array([5, 6, 7, 8, 9], np.uint32)
    offs = np.array([0, 0, 3, 3, 5], np.uint64)
    out, mask, ln, nt = lc.padded(ids, offs, 4, 0, bos=1, eos=2)
    assert out.tolist() == [[1, 2, 0, 0], [1, 5, 6, 2], [1, 2, 0, 0], [1, 8, 9, 2]]
    assert mask.tolist() == [[1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 1, 1]]
    assert ln.tolist() == [2, 4, 2, 4] and nt == 1
    out, mask, ln, nt = lc.padded(ids, offs, 4, 0, bos=1, eos=2, pad_left=True, trunc_left=True)
    assert out.tolist() == [[0, 0, 1, 2], [1, 6, 7, 2], [0, 0, 1, 2], [1, 8, 9, 2]]
    assert mask.tolist() == [[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1]] and nt == 1
    out, mask, ln, nt = lc.padded(ids, offs, 2, 0)
    assert out.tolist() == [[0, 0], [5, 6], [0, 0], [8, 9]] and ln.tolist() == [0, 2, 0, 2] and nt == 1
    out, mask, ln, nt = lc.padded(ids, offs, 2, 0, trunc_left=True, pad_left=True)
    assert out.tolist() == [[0, 0], [6, 7], [0, 0], [8, 9]]
    out, mask, ln, nt = lc.padded(ids, offs, 1, 0, eos=2)   # L = A: only the eos survives
    assert out.tolist() == [[2], [2], [2], [2]] and mask.tolist() == [[1]] * 4 and nt == 2

    out, doc, pos = lc.packed(ids, offs, 4, 0, eos=2)
    assert out.tolist() == [[2, 5, 6, 7], [2, 2, 8, 9], [2, 0, 0, 0]]
    assert doc.tolist() == [[0, 1, 1, 1], [1, 2, 3, 3], [3, -1, -1, -1]]
    assert pos.tolist() == [[0, 0, 1, 2], [3, 0, 0, 1], [2, 0, 0, 0]]
    out, doc, pos = lc.packed(ids, offs, 3, 0)   # A = 0: the empty rows own no position
    assert out.tolist() == [[5, 6, 7], [8, 9, 0]] and doc.tolist() == [[1, 1, 1], [3, 3, -1]] and pos.tolist() == [[0, 1, 2], [0, 1, 0]]
    out, doc, pos = lc.packed(ids, offs, 7, 0, bos=1)
    assert out.tolist() == [[1, 1, 5, 6, 7, 1, 1], [8, 9, 0, 0, 0, 0, 0]] and doc.tolist() == [[0, 1, 1, 1, 1, 2, 3], [3, 3, -1, -1, -1, -1, -1]]
    out, doc, pos = lc.packed(np.zeros(0, np.uint32), np.zeros(1, np.uint64), 4, 0, bos=1)
    assert out.shape == (0, 4) and doc.shape == (0, 4)


def test_fast_checker_agrees_with_the_checker():
    for name, (ids, offs) in INPUTS.items():
        for (bos, eos), L in itertools.product(BOS_EOS, [1, 7, 512]):
            a, b = lc.packed(ids, offs, L, PAD, bos, eos), lc.packed_fast(ids, offs, L, PAD, bos, eos)
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y), (name, bos, eos, L)


# ---- host twins against the checker ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(INPUTS))
def test_pad_host_against_the_checker(name):
    ids, offs = INPUTS[name]
    for (bos, eos), pside, tside, dt in itertools.product(BOS_EOS, ["right", "left"], ["right", "left"], [np.int32, np.int64]):
        a = (bos is not None) + (eos is not None)
        for L in _row_lens(offs, a):
            got = _lib.layout_pad_host(ids, offs, L, PAD, bos_id=bos, eos_id=eos, padding_side=pside, truncation_side=tside, dtype=dt)
            out, mask, ln, nt = lc.padded(ids, offs, L, PAD, bos, eos, pside == "left", tside == "left", dt)
            key = (name, bos, eos, pside, tside, dt, L)
            assert got["input_ids"].dtype == np.dtype(dt) and got["input_ids"].shape == out.shape, key
            assert np.array_equal(got["input_ids"], out), key
            assert np.array_equal(got["attention_mask"], mask), key
            assert np.array_equal(got["lengths"], ln), key
            assert got["n_truncated"] == nt, key


@pytest.mark.parametrize("name", list(INPUTS))
def test_pack_host_against_the_checker(name):
    ids, offs = INPUTS[name]
    for (bos, eos), dt in itertools.product(BOS_EOS, [np.int32, np.int64]):
        a = (bos is not None) + (eos is not None)
        n_stream = int(offs[-1]) + (len(offs) - 1) * a
        for L in [1, 7, 512, n_stream + 5]:
            got = _lib.layout_pack_host(ids, offs, L, PAD, bos_id=bos, eos_id=eos, dtype=dt)
            out, doc, pos = lc.packed(ids, offs, L, PAD, bos, eos, dt)
            key = (name, bos, eos, dt, L)
            assert got["input_ids"].dtype == np.dtype(dt) and got["input_ids"].shape == out.shape == (-(-n_stream // L), L), key
            assert np.array_equal(got["input_ids"], out), key
            assert np.array_equal(got["doc_ids"], doc), key
            assert np.array_equal(got["positions"], pos), key


def test_optional_outputs_may_be_null():
    ids, offs = INPUTS["empty_runs"]
    n = offs.size - 1
    out = np.empty((n, 5), np.int32)
    _lib.check(_lib.lib.tgx_layout_pad_host(_lib.ptr(ids), _lib.ptr(offs), n, 5, PAD, 1, _lib.NO_ID, 0, _lib.ptr(out), None, None, None))
    assert np.array_equal(out, lc.padded(ids, offs, 5, PAD, bos=1)[0])
    nb = C.c_uint64()
    n_stream = int(offs[-1]) + n
    out = np.empty(-(-n_stream // 4) * 4, np.int64)
    _lib.check(_lib.lib.tgx_layout_pack_host(_lib.ptr(ids), _lib.ptr(offs), n, 4, PAD, 1, _lib.NO_ID, _lib.LAYOUT_I64, _lib.ptr(out), None, None,
                                             C.byref(nb)))
    assert nb.value * 4 == out.size and np.array_equal(out.reshape(-1, 4), lc.packed(ids, offs, 4, PAD, bos=1, dtype=np.int64)[0])


# ---- errors -------------------------------------------------------------------------------------------------

def _invalid(fn, *a, **kw):
    with pytest.raises(tgx.TokenGeeXError) as e:
        fn(*a, **kw)
    assert e.value.status == _lib.ERR_INVALID, e.value
    return e.value


def test_host_errors():
    ids, offs = INPUTS["plain"]
    _invalid(_lib.layout_pad_host, ids, offs, 0, PAD)                              # L = 0
    _invalid(_lib.layout_pad_host, ids, offs, 1, PAD, bos_id=1, eos_id=2)          # L < A
    _lib.layout_pad_host(ids, offs, 2, PAD, bos_id=1, eos_id=2)                    # L = A is fine
    _invalid(_lib.layout_pack_host, ids, offs, 0, PAD)                             # block_len = 0
    for bad in (2**31, 2**32 - 1):
        _invalid(_lib.layout_pad_host, ids, offs, 4, bad)                          # pad_id (TGX_NO_ID is no pad id either)
        _invalid(_lib.layout_pack_host, ids, offs, 4, bad)
    _invalid(_lib.layout_pad_host, ids, offs, 4, PAD, bos_id=2**31)
    _invalid(_lib.layout_pad_host, ids, offs, 4, PAD, eos_id=2**31 + 5)
    _invalid(_lib.layout_pack_host, ids, offs, 4, PAD, bos_id=2**31)
    _invalid(_lib.layout_pack_host, ids, offs, 4, PAD, eos_id=2**32 - 2)
    big = ids.copy()
    big[5] = 2**31                                                                  # a token id that does not fit i32
    _invalid(_lib.layout_pad_host, big, offs, 8, PAD)
    _invalid(_lib.layout_pack_host, big, offs, 8, PAD)
    _lib.layout_pad_host(big, offs, 1, PAD)                                         # ... is only refused where it is written
    # unknown flags, offsets that do not start at 0 or go down
    n = offs.size - 1
    out, nb = np.empty((n, 4), np.int32), C.c_uint64()
    call_pad = lambda i, o, flags=0, dst=out: _lib.check(_lib.lib.tgx_layout_pad_host(
        i, o, n, 4, PAD, _lib.NO_ID, _lib.NO_ID, flags, dst, None, None, None))
    call_pack = lambda i, o, flags=0, dst=np.empty(64, np.int32), nbp=C.byref(nb): _lib.check(_lib.lib.tgx_layout_pack_host(
        i, o, n, 4, PAD, _lib.NO_ID, _lib.NO_ID, flags, None if dst is None else _lib.ptr(dst), None, None, nbp))
    _invalid(call_pad, _lib.ptr(ids), _lib.ptr(offs), 8, _lib.ptr(out))
    _invalid(call_pack, _lib.ptr(ids), _lib.ptr(offs), _lib.LAYOUT_PAD_LEFT)        # the packed form has no sides
    shifted = offs + np.uint64(1)
    _invalid(call_pad, _lib.ptr(ids), _lib.ptr(shifted), 0, _lib.ptr(out))
    down = offs.copy()
    down[2] = 0
    _invalid(call_pack, _lib.ptr(ids), _lib.ptr(down))
    # NULL arguments
    _invalid(call_pad, None, _lib.ptr(offs), 0, _lib.ptr(out))
    _invalid(call_pad, _lib.ptr(ids), None, 0, _lib.ptr(out))
    _invalid(call_pad, _lib.ptr(ids), _lib.ptr(offs), 0, None)
    _invalid(call_pack, None, _lib.ptr(offs))
    _invalid(call_pack, _lib.ptr(ids), None)
    _invalid(call_pack, _lib.ptr(ids), _lib.ptr(offs), 0, None)
    _invalid(call_pack, _lib.ptr(ids), _lib.ptr(offs), 0, np.empty(64, np.int32), None)


def test_device_entry_points_refuse_null_before_any_device_call():
    """A NULL result is TGX_ERR_INVALID on a machine with or without a GPU: nothing of the HIP runtime is asked first
    (without a GPU a device call would give TGX_ERR_DEVICE)."""
    L = _lib.lib
    a, b = C.c_uint64(), C.c_uint64()
    dst = np.empty(16, np.int32)   # never written: the result is checked first
    assert L.tgx_result_layout_info(None, 1, 2, C.byref(a), C.byref(b)) == _lib.ERR_INVALID
    assert L.tgx_result_pad_device(None, 4, PAD, 1, 2, 0, None, _lib.ptr(dst), None, None, C.byref(a)) == _lib.ERR_INVALID
    assert L.tgx_result_pad_device(None, 4, PAD, 1, 2, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.tgx_result_pack_device(None, 4, PAD, 1, 2, 0, None, _lib.ptr(dst), None, None, C.byref(a)) == _lib.ERR_INVALID
    assert L.tgx_result_pack_device(None, 4, PAD, 1, 2, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"NULL" in L.tgx_last_error()
    assert L.tgx_result_device(None) == -1


def test_python_argument_checks():
    ids, offs = INPUTS["plain"]
    with pytest.raises(ValueError):
        _lib.layout_pad_host(ids, offs, 4, PAD, padding_side="middle")
    with pytest.raises(ValueError):
        _lib.layout_pad_host(ids, offs, 4, PAD, dtype=np.int16)
    _invalid(_lib.layout_pad_host, ids, offs, 4, -1)
    _invalid(_lib.layout_pad_host, ids, offs, 2**32, PAD)
    assert _lib.layout_flags("left", "left", np.int64) == _lib.LAYOUT_PAD_LEFT | _lib.LAYOUT_TRUNC_LEFT | _lib.LAYOUT_I64 == 7
    assert _lib.NO_ID == 0xFFFFFFFF


def test_tokenizer_resolves_layout_ids_without_a_device():
    tk = tgx.Tokenizer([(b"a", -1.0, False)], special_tokens=["<pad>", "<s>", "</s>"])
    got = tk._layout_ids({"pad": "<pad>", "bos": "<s>", "eos_id": "</s>", "max_length": 8})
    assert got == {"pad_id": 1, "bos_id": 2, "eos_id": 3, "max_length": 8}
    assert tk._layout_ids({"pad_id": 0}) == {"pad_id": 0}
    with pytest.raises(tgx.TokenGeeXError):
        tk._layout_ids({"pad": "<nope>"})
    with pytest.raises(TypeError):
        tk._layout_ids({"bos": "<s>"})           # pad is required
    with pytest.raises(TypeError):
        tk._layout_ids({"pad": 0, "pad_id": 0})


def test_import_does_not_import_torch():
    code = ("import sys, tokengeex_amd, tokengeex_amd.tensors; "
            "assert 'torch' not in sys.modules, 'import tokengeex_amd pulled torch in'; "
            "assert callable(tokengeex_amd.to_padded) and callable(tokengeex_amd.to_packed)")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
