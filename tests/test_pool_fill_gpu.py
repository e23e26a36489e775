"""Every device call of tests/dirty_runs.py on hostile memory: with TGX_POOL_FILL every buffer the library's pool hands out
(scratch, results, plans, texts, corpora; recycled or fresh) holds one byte over its whole pooled size before its owner
sees it.  0 is the control.  255 is a NaN in every float width, the largest index and every flag bit set; 1 gives the
small wrong counts and true flags that a sum would swallow under 255.  A kernel that reads a scratch byte, a flag or a
partial sum that nothing wrote in its call, an atomic path whose pre-set covers less than the array, or a tail behind a
buffer's end, gives different outputs under the three; with a pool that happens to hold zeros it gives the right ones.

Per entry: the outputs of each run pass the entry's check (the subsystem's own reference, dirty_runs.py), a deterministic
entry's outputs under 255 and 1 are bit for bit the control's, and tgx_pool_filled_bytes() grew in every run: a filled
run that filled nothing does not pass."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dirty_runs

KNOB = "TGX_POOL_FILL"
FILLS = ("0", "255", "1")


def same_outputs(e, got, control, fill):
    """a deterministic entry: every output the same bits; else every output but the atomically summed ones"""
    keys = [k for k in control if not k.startswith("_") and (e.deterministic or k not in e.summed)]
    assert sorted(k for k in got if not k.startswith("_")) == sorted(k for k in control if not k.startswith("_")), fill
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(control[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (e.name, k, fill)


@pytest.mark.parametrize("name", sorted(dirty_runs.ENTRIES))
def test_entry_on_filled_memory(monkeypatch, name):
    e = dirty_runs.ENTRIES[name]
    for k, v in e.env.items():
        monkeypatch.setenv(k, v)
    ctx = dirty_runs.Ctx()
    tgx.pool_trim()
    runs = {}
    for fill in FILLS:
        monkeypatch.setenv(KNOB, fill)
        before = _lib.pool_filled_bytes()
        out = e.run(ctx)
        assert _lib.pool_filled_bytes() > before, (name, fill, "nothing was filled")
        e.check(out)
        runs[fill] = out
    for fill in FILLS[1:]:
        same_outputs(e, runs[fill], runs["0"], fill)


def _small_call():
    res = _lib.NativeResult.from_ids(np.arange(5, dtype=np.uint32), np.array([0, 2, 5], np.uint64), 10)
    got = res.select([1, 0, 1])
    ids = got.ids()
    got.free()
    res.free()
    return ids


def test_without_the_knob_the_counter_does_not_move(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    before = _lib.pool_filled_bytes()
    assert _small_call().tolist() == [2, 3, 4, 0, 1, 2, 3, 4]
    tgx.pool_trim()
    assert _small_call().tolist() == [2, 3, 4, 0, 1, 2, 3, 4]
    assert _lib.pool_filled_bytes() == before
    for bad in ("", "256", "-1", "x", "1x"):   # values outside 0 .. 255 are no fill
        monkeypatch.setenv(KNOB, bad)
        _small_call()
        assert _lib.pool_filled_bytes() == before, bad
    monkeypatch.setenv(KNOB, "7")
    _small_call()
    assert _lib.pool_filled_bytes() > before


@pytest.mark.parametrize("recycled", [False, True])
def test_the_bytes_behind_a_results_one_id_hold_the_fill(monkeypatch, recycled):
    """memory the library allocates and does not write, read through a pointer the surface exposes: the ids of a result
    of one id are 4 bytes of a pooled buffer; the 252 behind them hold the fill, in a fresh buffer and in a recycled one"""
    monkeypatch.setenv(KNOB, "90")
    tgx.pool_trim()
    if recycled:   # the same sizes, freed into the pool with another byte in them
        _lib.NativeResult.from_ids(np.array([3], np.uint32), np.array([0, 1], np.uint64), 10).free()
    monkeypatch.setenv(KNOB, "165")
    before = _lib.pool_filled_bytes()
    res = _lib.NativeResult.from_ids(np.array([9], np.uint32), np.array([0, 1], np.uint64), 10)
    try:
        assert _lib.pool_filled_bytes() >= before + 512   # the ids' buffer and the offsets', 256 bytes at least each
        host = np.zeros(256, np.uint8)
        hip_memcpy = _lib.lib.hipMemcpy   # (the runtime libtgx.so is linked against)
        hip_memcpy.restype, hip_memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip_memcpy(_lib.ptr(host), res.ids_device_ptr(), 256, 2) == 0   # hipMemcpyDeviceToHost
        assert host[:4].tolist() == [9, 0, 0, 0] and (host[4:] == 165).all(), host[:16]
    finally:
        res.free()
