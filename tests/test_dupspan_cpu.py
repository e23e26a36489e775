"""Duplicate spans across rows without a device: the host twin (tgx_dup_spans_host, through csrc/dupspan.h) against the
plain checker of tests/dupspan_cases.py for every key_bits (4 and 1 make runs of different grams that share a masked key)
and the answers the batches are built for; the header's table; the refusals before a device is asked for; span_keep."""
import os
import re

import numpy as np
import pytest

from tokengeex_amd import _lib, tensors

import dupspan_cases as dsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,kind,w", dsc.ALL)
def test_twin_matches_checker(name, kind, w):
    c = dsc.checked_case(name, kind, w)
    for key_bits in dsc.key_bits_of(c["data"].size):
        table, mask = _lib.dup_spans_host(c["data"], c["offs"], w, key_bits, seed=key_bits)
        assert np.array_equal(table, c["want"][0]) and np.array_equal(mask, c["want"][1]), key_bits
    assert (mask[c.get("repeat_at", [])] & 1).all(), "a repeat planted inside a row is a duplicate"
    o, where = c["offs"].astype(np.int64), c.get("where", {})
    if name in ("paste", "short_share"):   # exactly the w + 3 pasted elements, neither neighbour; w - 1 shared elements: nothing
        assert np.flatnonzero(mask).tolist() == list(range(where["first"], where["first"] + (where["span"] if name == "paste" else 0)))
        assert where["span"] == (w + 3 if name == "paste" else w - 1)
    if name == "twins":   # the second row wholly covered, the first not at all
        assert c["rows"][1] == c["rows"][2] and not mask[:o[2]].any() and (mask[o[2]:] & 2).all() and table[1:, 2].tolist() == [o[3] - o[2] - w + 1, o[3] - o[2]]
    if name == "five_tiles":
        assert table[:, where["row"]].tolist() == [5 * 256 - w + 1, 5 * 256 - w, 5 * 256 - 1]


def test_outputs_alone_and_refusals():
    c = dsc.checked_case("edges_chunk", "bytes", 5)
    lib, p = _lib.lib, _lib.ptr
    S, N = len(c["offs"]) - 1, c["data"].size
    table, mask = np.full((3, S), -7, np.int64), np.full(N, 7, np.uint8)
    assert lib.tgx_dup_spans_host(p(c["data"]), 1, p(c["offs"]), S, 5, 4, 0, p(table), None) == 0 and np.array_equal(table, c["want"][0])
    assert lib.tgx_dup_spans_host(p(c["data"]), 1, p(c["offs"]), S, 5, 4, 0, None, p(mask)) == 0 and np.array_equal(mask, c["want"][1])
    table[:], mask[:] = -7, 7
    for eb, w, kb in ((3, 2, 64), (1, 0, 64), (1, 65, 64), (4, 17, 64), (1, 5, 0), (1, 5, 65)):
        assert lib.tgx_dup_spans_host(p(c["data"]), eb, p(c["offs"]), S, w, kb, 0, p(table), p(mask)) == _lib.ERR_INVALID, (eb, w, kb)
    assert lib.tgx_dup_spans_host(p(c["data"]), 1, p(c["offs"]), S, 5, 64, 0, None, None) == _lib.ERR_INVALID
    assert lib.tgx_dup_spans_host(None, 1, p(c["offs"]), S, 5, 64, 0, p(table), p(mask)) == _lib.ERR_INVALID
    assert lib.tgx_dup_spans_host(p(c["data"]), 1, p(c["offs"]), 0, 5, 64, 0, p(table), p(mask)) == 0, "no row: nothing is written"
    # the device calls refuse these before a device is asked for: no handle is needed to be told
    out = p(table)
    for call, w_max in ((lib.tgx_corpus_dup_spans_device, 64), (lib.tgx_result_dup_spans_device, 16)):
        for w, kb, flags, outs, said in ((0, 64, 0, (out, out), "width"), (w_max + 1, 64, 0, (out, out), "width"), (5, 0, 0, (out, out), "key_bits"),
                                        (5, 65, 0, (out, out), "key_bits"), (5, 64, 1, (out, out), "flags"), (5, 64, 0, (None, None), "both NULL")):
            assert call(None, w, kb, 0, flags, None, *outs) == _lib.ERR_INVALID and said in lib.tgx_last_error().decode(), (w, kb, flags)
    assert (table == -7).all() and (mask == 7).all(), "a refused call writes nothing"
    with pytest.raises(ValueError):
        _lib.dupspan_check_key_bits(65)
    names, ms = (_lib.C.c_char_p * 8)(), (_lib.C.c_float * 8)()
    assert lib.tgx_dupspan_last_times(names, ms, 8) == 4 and [names[k].decode() for k in range(4)] == dsc.STAGES


def test_header_and_symbol_table_agree():
    """every function the header declares is in DUPSPAN_SYMBOLS and exported, and none of them is in another table"""
    with open(os.path.join(ROOT, "include", "tgx_dupspans.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"^(?:tgx_status|int) (tgx_[a-z_0-9]+)\(", f.read(), re.M))
    others = [getattr(_lib, name) for name in dir(_lib) if name.endswith("SYMBOLS") and name != "DUPSPAN_SYMBOLS"]
    assert declared == set(_lib.DUPSPAN_SYMBOLS) and len(declared) == 4
    assert not any(declared & set(t) for t in others) and all(hasattr(_lib.lib, name) for name in declared)


def test_span_keep_rule():
    import torch
    covered, elems = torch.tensor([0, 0, 1, 5, 10, 3]), torch.tensor([0, 9, 10, 10, 10, 10])
    for max_frac, want in ((0.0, [0, 1]), (0.1, [0, 1, 2]), (0.5, [0, 1, 2, 3, 5]), (1.0, [0, 1, 2, 3, 4, 5])):
        assert tensors.span_keep(covered, elems, max_frac).nonzero().reshape(-1).tolist() == want, max_frac
    s = tensors.DupSpans(torch.tensor([[1, 2], [0, 1], [0, 3]]), torch.tensor([0, 4]), 3)
    assert s.grams.tolist() == [1, 2] and s.dup.tolist() == [0, 1] and s.covered_frac.tolist() == [0.0, 0.75] and s.mask is None
