"""tgx_assemble_host — the host twin of the device assembly (csrc/assemble.hip), which walks the kernel's tiles through
the same index arithmetic (csrc/assemble.h) — against the plain-numpy checker (tests/assemble_checker.py) and against
tgx_assemble_ids, the serial host loop it replaces.  Everything is compared exactly: this is integer data movement.

Plans are random, with the number of output ids drawn around the edges of the kernel's 1024-position tile and with runs
of special tokens, of encoded segments without ids and of samples without segments, each kind also as the very first and
the very last thing of a plan."""
import itertools
import os
import re

import numpy as np
import pytest

from tokengeex_amd import _lib

import assemble_checker as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, N_SPECIALS = 1000, 5
T_OUT = [0, 1, 1023, 1024, 1025, 2048, 4097]
KINDS = ["special", "empty", "none", "encoded"]   # a run of specials / of empty encoded segments / of segment-less samples / ids


def _runs(rng, n, max_runs):
    """n split into at most max_runs positive run lengths (two at least when n allows it)"""
    if n == 0:
        return []
    k = int(rng.integers(min(n, 2), min(n, max_runs) + 1))
    cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(int).tolist()


def random_plan(rng, t_out, head, tail):
    """-> (ids, id_offs, seg_offs, seg_special, what really is at the head, at the tail) with t_out output ids"""
    n_sp = int(rng.integers(0, min(t_out, int(rng.choice([3, 40, 3000]))) + 1))
    if t_out and "special" in (head, tail):
        n_sp = max(n_sp, min(t_out, 2))
    if "encoded" in (head, tail):
        n_sp = min(n_sp, max(0, t_out - 2))
    T = t_out - n_sp
    blocks = [[("s", 1)] * n for n in _runs(rng, n_sp, 6)]                  # runs of specials
    blocks += [[("e", n)] for n in _runs(rng, T, 9)]                        # encoded segments with ids
    blocks += [[("e", 0)] * int(rng.integers(1, 5)) for _ in range(int(rng.integers(0, 4)))]   # runs of empty ones
    order = rng.permutation(len(blocks)).tolist()
    blocks = [blocks[i] for i in order]

    def pull(kind, to_front):
        want = {"special": lambda b: b[0][0] == "s", "encoded": lambda b: b[0] != ("e", 0) and b[0][0] == "e"}[kind]
        for i in range(0 if to_front else 1, len(blocks)):   # (the block pulled to the front stays there)
            if want(blocks[i]):
                blocks.insert(0 if to_front else len(blocks), blocks.pop(i))
                return
    for kind, front in ((head, True), (tail, False)):
        if kind in ("special", "encoded"):
            pull(kind, front)
    if head == "empty":
        blocks.insert(0, [("e", 0)] * 3)
    if tail == "empty":
        blocks.append([("e", 0)] * 2)
    segs = [x for b in blocks for x in b]
    K = len(segs)
    seg_special = np.array([int(rng.integers(0, N_SPECIALS)) if k == "s" else -int(rng.integers(1, 4)) for k, _ in segs], np.int32)
    lens = [n for k, n in segs if k == "e"]
    id_offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=id_offs[1:])
    ids = rng.integers(0, V, size=T).astype(np.uint32)
    S = int(rng.integers(1, 8))
    cuts = np.sort(rng.integers(0, K + 1, size=S - 1)).tolist()   # equal cuts: samples without segments
    seg_offs = [0] * (3 if head == "none" else 0) + [0] + cuts + [K] + [K] * (2 if tail == "none" else 0)
    seg_offs = np.array(seg_offs, np.uint64)

    def kind_at(k):
        return "special" if segs[k][0] == "s" else ("empty" if segs[k][1] == 0 else "encoded")
    at_head = "none" if head == "none" else (kind_at(0) if K else None)
    at_tail = "none" if tail == "none" else (kind_at(K - 1) if K else None)
    return ids, id_offs, seg_offs, seg_special, at_head, at_tail


def _check(ids, id_offs, seg_offs, seg_special):
    want_ids, want_offs = ac.assemble(ids, id_offs, seg_offs, seg_special, V)
    got_ids, got_offs = _lib.assemble_host(seg_offs, seg_special, ids, id_offs, V, N_SPECIALS)
    assert np.array_equal(got_offs, want_offs) and np.array_equal(got_ids, want_ids)
    old_ids, old_offs = _lib.assemble_ids(seg_offs, seg_special, ids, id_offs, V)
    assert np.array_equal(old_offs, want_offs) and np.array_equal(old_ids, want_ids)
    return got_ids, got_offs


def test_random_plans_around_the_tile_edges():
    rng = np.random.default_rng(20240611)
    seen_head, seen_tail, n_plans = set(), set(), 0
    for t_out, head, tail, _ in itertools.product(T_OUT, KINDS, KINDS, range(2)):
        ids, id_offs, seg_offs, seg_special, at_head, at_tail = random_plan(rng, t_out, head, tail)
        got_ids, got_offs = _check(ids, id_offs, seg_offs, seg_special)
        assert got_ids.size == t_out == int(got_offs[-1])
        if t_out >= 1023:
            assert at_head == head and at_tail == tail, (t_out, head, tail, at_head, at_tail)
            seen_head.add((t_out, at_head))
            seen_tail.add((t_out, at_tail))
        n_plans += 1
    assert n_plans >= 200
    big = [t for t in T_OUT if t >= 1023]
    assert seen_head == seen_tail == set(itertools.product(big, KINDS))


def test_all_special_plan_and_plan_without_specials():
    rng = np.random.default_rng(5)
    # every segment special: no result over encoded segments at all (None), or one without rows
    sp = rng.integers(0, N_SPECIALS, size=2500).astype(np.int32)
    seg_offs = np.array([0, 0, 1, 1024, 1024, 2049, 2500, 2500], np.uint64)
    for id_offs in (None, np.zeros(1, np.uint64)):
        got_ids, got_offs = _lib.assemble_host(seg_offs, sp, np.zeros(0, np.uint32), id_offs, V, N_SPECIALS)
        assert np.array_equal(got_ids, V + sp.astype(np.uint32)) and np.array_equal(got_offs, seg_offs)
    assert np.array_equal(ac.assemble(np.zeros(0, np.uint32), None, seg_offs, sp, V)[0], got_ids)
    # no special at all, the segments regrouped into fewer samples: the ids unchanged, the offsets regrouped
    lens = rng.integers(0, 700, size=12)
    id_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ids = rng.integers(0, V, size=int(id_offs[-1])).astype(np.uint32)
    seg_offs = np.array([0, 0, 5, 5, 6, 12, 12], np.uint64)
    got_ids, got_offs = _check(ids, id_offs, seg_offs, np.full(12, -1, np.int32))
    assert np.array_equal(got_ids, ids) and np.array_equal(got_offs, id_offs[seg_offs.astype(np.int64)])
    # no sample: an empty result with offsets [0]
    got_ids, got_offs = _lib.assemble_host(np.zeros(1, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.uint32), None, V, N_SPECIALS)
    assert got_ids.size == 0 and got_offs.tolist() == [0]


def test_one_segment_over_many_tiles():
    """a segment of 17 000 ids between specials: most tiles lie inside one segment, lo == hi"""
    rng = np.random.default_rng(6)
    ids = rng.integers(0, V, size=17_000 + 3).astype(np.uint32)
    id_offs = np.array([0, 3, 3, 17_003], np.uint64)
    seg_special = np.array([2, -1, 0, 0, -1, -1, 4], np.int32)
    _check(ids, id_offs, np.array([0, 3, 7], np.uint64), seg_special)


def _invalid(**kw):
    args = dict(seg_offs=np.array([0, 2, 3], np.uint64), seg_special=np.array([-1, 1, -1], np.int32), ids=np.arange(5, dtype=np.uint32),
                id_offs=np.array([0, 2, 5], np.uint64), vocab_size=V, n_specials=N_SPECIALS)
    args.update(kw)
    with pytest.raises(_lib.TokenGeeXError) as e:
        _lib.assemble_host(**args)
    assert e.value.status == _lib.ERR_INVALID, e.value
    return str(e.value)


def test_validation_errors_by_status():
    good = _lib.assemble_host(np.array([0, 2, 3], np.uint64), np.array([-1, 1, -1], np.int32), np.arange(5, dtype=np.uint32),
                              np.array([0, 2, 5], np.uint64), V, N_SPECIALS)
    assert good[0].tolist() == [0, 1, V + 1, 2, 3, 4] and good[1].tolist() == [0, 3, 6]
    assert "seg_offs[0]" in _invalid(seg_offs=np.array([1, 2, 3], np.uint64))
    assert "monotone" in _invalid(seg_offs=np.array([0, 4, 3], np.uint64))
    assert "special token" in _invalid(seg_special=np.array([-1, N_SPECIALS, -1], np.int32))
    assert "special token" in _invalid(n_specials=1)
    assert "rows" in _invalid(seg_special=np.array([-1, 1, 1], np.int32))                    # one encoded segment, two rows
    assert "rows" in _invalid(seg_special=np.array([-1, -1, -1], np.int32))                  # three, two rows
    assert "rows" in _invalid(id_offs=np.array([0, 1, 2, 2, 4, 5, 5], np.uint64))            # an n-best result: E * nbest rows
    assert "no result" in _invalid(id_offs=None, ids=np.zeros(0, np.uint32))                 # E > 0 and nothing over them
    assert "no room" in _invalid(vocab_size=0xFFFFFFFE - N_SPECIALS + 1)
    assert "no room" in _invalid(vocab_size=0xFFFFFFFF, n_specials=0, seg_special=np.array([-1, -1], np.int32),
                                 seg_offs=np.array([0, 1, 2], np.uint64))
    assert "offs[0]" in _invalid(id_offs=np.array([1, 2, 5], np.uint64))
    assert "room for 5" in _invalid(ids_cap=5)                                               # six ids
    assert _lib.assemble_host(np.array([0, 2, 3], np.uint64), np.array([-1, 1, -1], np.int32), np.arange(5, dtype=np.uint32),
                              np.array([0, 2, 5], np.uint64), 0xFFFFFFFE - N_SPECIALS, N_SPECIALS)[0][2] == 0xFFFFFFFE - N_SPECIALS + 1


def test_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "tgx.h"), encoding="utf-8") as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(tgx_[a-z_0-9]+)\s*\(", hdr))
    for name in ("tgx_assemble_result", "tgx_assemble_host", "tgx_result_vocab_size"):
        assert name in declared and name in _lib.SYMBOLS and getattr(_lib.lib, name) is not None
    assert _lib.lib.tgx_abi_version() == 1
