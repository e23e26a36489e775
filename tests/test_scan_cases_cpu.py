"""What tests/test_scans_edges_gpu.py relies on, established without a GPU from the oracle's ids alone: every case of
tests/scan_cases.py encodes to the ids it was built from and sits on the edge it claims (the largest id in pairs, the
listed sample lengths, every residue of the token total mod 4, ties across the cuts of count_pairs_top), and the numpy
reduction that serves as the reference equals the oracle's own counting passes."""
import os
import time

import numpy as np
import pytest

from oracle import oracle as orc

import scan_cases as sc


def test_grid_sizes_sit_on_the_key_geometry():
    """shift per vocabulary size, key widths of 19 .. 35 bits crossing 32 between 32 768 and 32 769, the histogram's
    limit between 36 864 and 36 865; 39 bits for the 500 000-entry vocabulary."""
    assert [sc.shift_of(v) for v in sc.SIZES] == [9, 9, 10, 15, 16, 16, 16, 16, 16, 17]
    assert all(sc.shift_of(v) == s for v, s in sc.SHIFTS.items())
    widths = [2 * sc.shift_of(v) + 1 for v in sc.SIZES]
    assert min(widths) == 19 and max(widths) == 35
    assert 2 * sc.shift_of(32768) + 1 == 31 and 2 * sc.shift_of(32769) + 1 == 33
    assert 36864 in sc.SIZES and 36865 in sc.SIZES and sc.HIST_MAX_VOCAB == 36864
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tokengeex_amd", "csrc", "kernels.h"), encoding="utf-8") as f:
        assert "constexpr uint32_t kHistMaxVocab = 36864;" in f.read()   # the crossover the cases sit on is the library's
    assert 2 * sc.shift_of(500000) + 1 == 39 and len(sc.vocab("500k")[0]) == 500000
    # the largest pair key stays below the sentinel 1 << 2 shift, the sentinel below 1 << end_bit
    for v in sc.SIZES + (500000, sc.LONG_BASE + 1):
        s = sc.shift_of(v)
        assert (((v - 1) << s) | (v - 1)) < (1 << 2 * s) < (1 << (2 * s + 1)) and (1 << s) >= v > (1 << (s - 1))


def test_grid_65537_builds_quickly_and_holds_the_largest_pair():
    toks, scores = sc.grid(65537)
    assert len(toks) == 65537 == len(set(toks)) and toks[65536] == b"\xff\x00" and toks[256] == b"\x00\x00"
    t0 = time.perf_counter()
    om = orc.OracleModel(toks, scores)
    built = time.perf_counter() - t0
    assert built < 1.0, built
    flat, offs = orc.pack([toks[65536] * 3, toks[65536] + toks[256]])
    ids, id_offs = om.encode_batch_flat(flat, offs)
    assert ids.tolist() == [65536, 65536, 65536, 65536, 256] and id_offs.tolist() == [0, 3, 5]
    keys, counts = sc.pairs_numpy(ids, id_offs)
    assert dict(zip(keys.tolist(), counts.tolist())) == {(65536 << 32) | 65536: 2, (65536 << 32) | 256: 1}


def test_long_token_vocabularies():
    for n in (24, 40):
        toks, scores = sc.vocab(f"4096+{n}")
        assert len(toks) == 4097 and len(toks[-1]) == n == max(map(len, toks)) and sc.shift_of(4097) == 13
        flat, offs, ids, id_offs = sc.corpus(f"4096+{n}", "edges", 1)
        assert flat.tobytes().count(toks[-1]) >= 300  # the long token occurs in the text


def test_pairs_numpy_by_hand():
    ids = np.array([5, 5, 5, 7, 5, 5, 9], np.uint32)
    offs = np.array([0, 0, 3, 3, 4, 6, 7, 7], np.uint64)  # samples: (), (5 5 5), (), (7), (5 5), (9), ()
    keys, counts = sc.pairs_numpy(ids, offs)
    assert keys.tolist() == [(5 << 32) | 5] and counts.tolist() == [3]
    assert sc.pairs_numpy(ids[:1], offs[:3])[0].size == 0
    keys, counts = sc.pairs_numpy(ids, np.array([0, 7], np.uint64))
    assert dict(zip(keys.tolist(), counts.tolist())) == {(5 << 32) | 5: 3, (5 << 32) | 7: 1, (7 << 32) | 5: 1, (5 << 32) | 9: 1}
    c = np.array([9, 4, 4, 4, 2, 1, 1], np.uint64)
    assert sc.top_ks(c) == {"1": 1, "2": 2, "tie": 3, "total-1": 6, "total": 7, "total+1": 8}
    assert sc.cut_is_tied(c, 2) and sc.cut_is_tied(c, 6) and not sc.cut_is_tied(c, 1) and not sc.cut_is_tied(c, 7)
    assert sc.top_ks(c[:1]) == {"1": 1, "2": 2, "total": 1, "total+1": 2} and sc.top_ks(c[:0]) == {"1": 1, "2": 2, "total+1": 1}
    assert sc.top_ks(np.array([3, 3], np.uint64))["tie"] == 1


GROUPS = tuple(dict.fromkeys((name, kind) for name, kind, _ in sc.CASES)) + (("4096+24", "edges"), ("4096+40", "edges"))


@pytest.mark.parametrize("name,kind", GROUPS, ids=lambda v: v)
def test_case_is_as_designed(name, kind):
    residues = set()
    for tail in sc.TAILS:
        residues.add(_check_case(name, kind, tail) % 4)
    # over the tail variants the token total takes every residue mod 4 (the n - 4 n4 tail of the histogram's uint4 loop)
    assert residues == {0, 1, 2, 3}


def _check_case(name, kind, tail) -> int:
    toks, _ = sc.vocab(name)
    V = len(toks)
    om = sc.oracle_model(name)
    flat, offs, plan_ids, plan_offs = sc.corpus(name, kind, tail)
    ref = sc.reference(name, kind, tail)
    ids, id_offs = ref["ids"], ref["offs"]
    if plan_ids is not None:  # the text encodes to exactly the ids it was built from
        np.testing.assert_array_equal(id_offs, plan_offs)
        np.testing.assert_array_equal(ids, plan_ids)
    n_tok = np.diff(id_offs.astype(np.int64))
    assert n_tok.size == offs.size - 1
    if tail:
        assert (n_tok[-tail:] == 1).all()
    T = int(ids.size)
    pairs = dict(zip(ref["keys"].tolist(), ref["counts"].tolist()))
    mx = V - 1
    if kind == "edges":
        assert {(mx << 32) | mx, (mx << 32) | sc.LO, (sc.LO << 32) | mx} <= set(pairs) and ref["freq"][mx] > 0
        assert set(sc.N_TOKENS) <= set(n_tok.tolist())
        e = n_tok[:len(n_tok) - tail] == 0
        assert e[0] and e[-1] and any(e[i:i + 3].all() for i in range(1, e.size - 3))
        # odd-length runs of single bytes
        assert all(any(n == k and (ids[int(a):int(a) + k] == 255).all() for a, n in zip(id_offs[:-1], n_tok)) for k in sc.ODD_BYTES)
        assert max(n_tok) == 257
    elif kind == "bulk":
        assert T == sc.BULK_TOKENS + tail and n_tok.max() == sc.BULK_MAX_SAMPLE and n_tok.min() >= 1
        assert ref["freq"][mx] > 0 and ref["freq"][:256].sum() == 0
    else:
        assert V == 500000 and ids.max() >= 1 << 16 and abs(int(flat.size) - (1 << 20)) < 4096 + tail and len(pairs) > 100000
    # the reference: numpy against the oracle's own passes
    np.testing.assert_array_equal(ref["freq"], om.count_tokens_flat(flat, offs, threads=8))
    wk, wc = om.count_pairs_flat(flat, offs, threads=8)
    np.testing.assert_array_equal(ref["keys"], wk)
    np.testing.assert_array_equal(ref["counts"], wc)
    assert int(ref["freq"].sum()) == T and int(ref["counts"].sum()) == T - int((n_tok > 0).sum())
    # the top order: descending counts, ascending keys inside a run of equal counts
    tk, tc = ref["top_keys"], ref["top_counts"].astype(np.int64)
    assert (np.diff(tc) <= 0).all() and (np.diff(tk.astype(np.int64))[np.diff(tc) == 0] > 0).all()
    ks = sc.top_ks(ref["top_counts"])
    if "tie" in ks:
        assert sc.cut_is_tied(ref["top_counts"], ks["tie"])
    return T


def test_every_cutting_k_cuts_through_a_tie_somewhere():
    """A million uniform pairs over 65 281^2 values: about a hundred occur twice, hardly any three times, the rest once.
    So k = 1, 2, the tie k and total - 1 all cut through a run of equal counts in this case."""
    ref = sc.reference("65537", "bulk", 0)
    ks = sc.top_ks(ref["top_counts"])
    assert set(ks) == {"1", "2", "tie", "total-1", "total", "total+1"}
    assert all(sc.cut_is_tied(ref["top_counts"], ks[kind]) for kind in ("1", "2", "tie", "total-1"))
    assert ref["top_counts"][0] >= 2 and ref["top_counts"][-1] == 1
