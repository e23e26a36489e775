"""Vocabularies, texts and references for the edge tests of the integer counting passes (tests/test_scan_cases_cpu.py,
tests/test_scans_edges_gpu.py): the token histogram, the pair scan and its top-k head.  Nothing here calls the library's
kernels: ids come from the CPU oracle's encoder, expectations from those ids reduced with plain numpy.

The vocabulary family grid(V): the 256 single bytes at -10, then the first V - 256 two-byte strings bytes([k >> 8, k & 255])
at -1.  A text that concatenates two-byte tokens encodes to exactly those ids (any other segmentation pays -10 for a byte
at least twice), so a sample's token count and the ids in it are chosen directly — the largest id included."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as orc
from tokengeex_amd import synth

import util

LO = 256
SIZES = (257, 512, 513, 32768, 32769, 36864, 36865, 65535, 65536, 65537)
SHIFTS = {257: 9, 512: 9, 513: 10, 32768: 15, 32769: 16, 36864: 16, 36865: 16, 65535: 16, 65536: 16, 65537: 17, 500000: 19}
HIST_MAX_VOCAB = 36864  # csrc/kernels.h: kHistMaxVocab
N_TOKENS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ODD_BYTES = (1, 3, 5, 63, 65)
TAILS = (0, 1, 2, 3)
BULK_TOKENS = (1 << 20) + 3
BULK_MAX_SAMPLE = 4096
LONG_BASE = 4096  # grid(4096) and one long token: the vocabularies of the long-token and the generic encode kernels

VOCABS = tuple(str(v) for v in SIZES) + ("500k", "4096+24", "4096+40")


def shift_of(vocab_size: int) -> int:
    """The pair scan's key geometry (tgx_api.cpp: count_pairs_impl): bits of the largest id; the key has 2 shift + 1."""
    s = 1
    while s < 32 and (1 << s) < vocab_size:
        s += 1
    return s


def grid(V: int):
    assert 257 <= V <= 65536 + 256
    k = np.arange(V - 256)
    toks = [bytes([c]) for c in range(256)] + [bytes([int(a), int(b)]) for a, b in zip(k >> 8, k & 255)]
    return toks, np.concatenate([np.full(256, -10.0), np.full(V - 256, -1.0)])


def grid_long(n_bytes: int):
    """grid(4096) and, as the largest id, one token of n_bytes bytes at -1: the concatenation of the grid tokens 300, 301,
    ... (which would cost -1 each)."""
    toks, scores = grid(LONG_BASE)
    long_tok = b"".join(toks[300 + i] for i in range(n_bytes // 2))
    assert len(long_tok) == n_bytes
    return toks + [long_tok], np.concatenate([scores, [-1.0]])


@functools.lru_cache(maxsize=None)
def vocab(name: str):
    if name == "500k":
        return util.load_vocab_500k()
    if name.startswith("4096+"):
        return grid_long(int(name[5:]))
    return grid(int(name))


@functools.lru_cache(maxsize=None)
def oracle_model(name: str):
    return orc.OracleModel(*vocab(name))


def cases_of(name: str):
    return ("synth",) if name == "500k" else ("edges", "bulk")


CASES = tuple((name, case, tail) for name in VOCABS[:len(SIZES) + 1] for case in cases_of(name) for tail in TAILS)


def case_id(c) -> str:
    return f"V={c[0]}-{c[1]}-tail{c[2]}"


# ---- texts ------------------------------------------------------------------------------------------------------------
def edges_plan(vocab_size: int):
    """-> list of id arrays, one per sample.  An empty sample first, last and three in a row in the middle; per n of
    N_TOKENS a sample of n times the largest id, one alternating the largest id and LO, one uniform over [256, V); then
    odd-length runs of the byte 0xFF (0xFF 0xFF is no token of any of these vocabularies: ids 255)."""
    mx = vocab_size - 1
    rng = np.random.default_rng(7919 * vocab_size)
    plan = [np.zeros(0, np.int64)]
    for j, n in enumerate(N_TOKENS):
        alt = np.full(n, mx, np.int64)
        alt[1::2] = LO
        plan += [np.full(n, mx, np.int64), alt, rng.integers(256, vocab_size, size=n)]
        if j == len(N_TOKENS) // 2:
            plan += [np.zeros(0, np.int64)] * 3
    plan += [np.full(n, 255, np.int64) for n in ODD_BYTES]
    plan.append(np.zeros(0, np.int64))
    return plan


def bulk_plan(vocab_size: int):
    """2^20 + 3 ids uniform over [256, V), cut into samples of 1 .. 4096 tokens (the first has 4096)."""
    rng = np.random.default_rng(104729 * vocab_size)
    ids = rng.integers(256, vocab_size, size=BULK_TOKENS)
    lens = [BULK_MAX_SAMPLE]
    while sum(lens) < BULK_TOKENS:
        lens.append(int(rng.integers(1, BULK_MAX_SAMPLE + 1)))
    lens[-1] -= sum(lens) - BULK_TOKENS
    assert min(lens) >= 1 and max(lens) == BULK_MAX_SAMPLE and sum(lens) == BULK_TOKENS
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [ids[cuts[i]:cuts[i + 1]] for i in range(len(lens))]


def _pack_plan(toks, plan):
    """-> (flat u8, offs u64, planned ids u32, planned id offsets u64)."""
    ids = np.concatenate(plan).astype(np.int64) if plan else np.zeros(0, np.int64)
    id_offs = np.concatenate([[0], np.cumsum([len(p) for p in plan])]).astype(np.uint64)
    tok_len = np.fromiter((len(t) for t in toks), np.int64, len(toks))
    offs = np.concatenate([[0], np.cumsum([int(tok_len[p].sum()) for p in plan])]).astype(np.uint64)
    if ids.size and int(tok_len[ids].min()) == 2 == int(tok_len[ids].max()):  # two-byte tokens only: without a Python loop
        k = ids - 256
        flat = np.stack([k >> 8, k & 255], axis=1).astype(np.uint8).ravel()
    else:
        flat = np.frombuffer(b"".join(toks[int(i)] for i in ids), np.uint8).copy()
    assert flat.size == int(offs[-1])
    return flat, offs, ids.astype(np.uint32), id_offs


@functools.lru_cache(maxsize=2)
def _base(name: str, case: str):
    toks, _ = vocab(name)
    if case == "synth":
        flat, offs = synth.make_corpus(1 << 20, "mixed", seed_offset=41)
        texts = [bytes(flat[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]
        return texts, None
    plan = edges_plan(len(toks)) if case == "edges" else bulk_plan(len(toks))
    return None, plan


def tail_ids(name: str):
    """The one-token sample that the tail wrapper appends: b"a" under the 500 000-entry vocabulary, else the token LO."""
    return None if name == "500k" else np.array([LO], np.int64)


def corpus(name: str, case: str, tail: int):
    """-> (flat, offs, planned ids or None, planned id offsets or None) of a case with `tail` one-token samples appended."""
    texts, plan = _base(name, case)
    if plan is None:
        flat, offs = orc.pack(texts + [b"a"] * tail)
        return flat, offs, None, None
    return _pack_plan(vocab(name)[0], plan + [tail_ids(name)] * tail)


# ---- the reference: the oracle's ids, reduced with numpy ----------------------------------------------------------------
def pairs_numpy(ids: np.ndarray, offs: np.ndarray):
    """Adjacent pairs inside samples -> (keys a << 32 | b ascending, counts), both u64."""
    if ids.size < 2:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    keys = (ids[:-1].astype(np.uint64) << np.uint64(32)) | ids[1:].astype(np.uint64)
    keep = np.ones(ids.size - 1, bool)
    cut = offs.astype(np.int64)
    cut = cut[(cut > 0) & (cut < ids.size)]
    keep[cut - 1] = False  # the pair (last token of a sample, first of the next)
    k, c = np.unique(keys[keep], return_counts=True)
    return k.astype(np.uint64), c.astype(np.uint64)


def top_order(keys: np.ndarray, counts: np.ndarray):
    """The order of tgx_count_pairs_top: descending count, ascending key among equal counts."""
    return np.lexsort((keys, -counts.astype(np.int64)))


def top_ks(sorted_counts: np.ndarray) -> dict:
    """kind -> k for count_pairs_top, from the reference's counts in top order.  'tie': the smallest k > 2 (else the
    smallest k >= 1) with equal counts on both sides of the cut, when there is one."""
    total = int(sorted_counts.size)
    ks = {"1": 1, "2": 2}
    tied = np.flatnonzero(sorted_counts[:-1] == sorted_counts[1:]) + 1 if total >= 2 else np.zeros(0, np.int64)
    if tied.size:
        ks["tie"] = int(tied[tied > 2][0]) if (tied > 2).any() else int(tied[0])
    if total - 1 >= 1:
        ks["total-1"] = total - 1
    if total >= 1:
        ks["total"] = total
    ks["total+1"] = total + 1
    return ks


def cut_is_tied(sorted_counts: np.ndarray, k: int) -> bool:
    return 1 <= k < sorted_counts.size and sorted_counts[k - 1] == sorted_counts[k]


def reference_of(om, flat, offs, vocab_size: int) -> dict:
    ids, id_offs = om.encode_batch_flat(flat, offs, threads=8)
    freq = np.bincount(ids, minlength=vocab_size).astype(np.uint64)
    keys, counts = pairs_numpy(ids, id_offs)
    order = top_order(keys, counts)
    return dict(ids=ids, offs=id_offs, freq=freq, keys=keys, counts=counts, top_keys=keys[order], top_counts=counts[order])


@functools.lru_cache(maxsize=2)
def reference(name: str, case: str, tail: int) -> dict:
    """-> ids, offs (the oracle's), freq u64[V], keys / counts (ascending key), top_keys / top_counts (top order)."""
    flat, offs, _, _ = corpus(name, case, tail)
    return reference_of(oracle_model(name), flat, offs, len(vocab(name)[0]))
