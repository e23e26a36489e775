"""Python restatement of n-best segmentation (tgx_encode_batch_nbest), the checker of tests/test_nbest_cpu.py and
tests/test_nbest_gpu.py.  Matches come from the CPU oracle's common prefix search (sample_checker.incoming); nothing here
calls the library's kernels.

Per sample: L[0] = [(0.0, -, -)]; L[p] = the top k of (L[q][r].score + s, q, r) over the matches (q, len), q + len = p,
and every r < |L[q]|, in the order score descending, then q ascending, then r ascending (f64 adds); row r is the
back-trace from L[n][r]."""
from __future__ import annotations

import itertools


def nbest(inc, scores, n: int, k: int):
    """-> (rows, row_scores): up to k id lists, best first, and their scores ([] when n is unreachable)."""
    L = [[] for _ in range(n + 1)]
    L[0] = [(0.0, -1, -1, -1)]  # (score, q, r, id)
    for p in range(1, n + 1):
        cands = [(L[q][r][0] + float(scores[tid]), q, r, tid) for q, tid in inc[p] for r in range(len(L[q]))]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        L[p] = cands[:k]
    rows, row_scores = [], []
    for r0 in range(len(L[n])):
        ids, p, r = [], n, r0
        while p > 0:
            _, q, rr, tid = L[p][r]
            ids.append(tid)
            p, r = q, rr
        rows.append(ids[::-1])
        row_scores.append(L[n][r0][0])
    return rows, row_scores


def path_score(ids, scores) -> float:
    """The left-to-right f64 sum of a row's token scores (what encode forms)."""
    acc = 0.0
    for t in ids:
        acc += float(scores[t])
    return acc


def brute_force(inc, scores, n: int):
    """Every segmentation of a short string as (ids, score), sorted by the pinned order: score descending, then the last
    token's start ascending, then the prefix by the same order (its rank in L[q])."""
    paths = {0: [((), (), 0.0)]}  # p -> [(ids, key, score)]
    for p in range(1, n + 1):
        out = []
        for q, tid in inc[p]:
            for ids, key, sc in paths.get(q, []):
                s = sc + float(scores[tid])
                out.append((ids + (tid,), (-s, q, key), s))
        paths[p] = out
    full = sorted(paths[n], key=lambda t: t[1])
    return [list(ids) for ids, _, _ in full], [sc for _, _, sc in full]


def combine_brute(seg_lists, k: int):
    """The k-best product of per-segment lists [(rows, scores)] by enumeration: candidates ordered by score descending,
    then the prefix combination's rank, then the segment row's rank.  -> (rows, scores)."""
    combos = [((), 0.0, ())]  # (row index per segment, score, key)
    for rows, scs in seg_lists:
        nxt = []
        for idx, sc, key in combos:
            for j in range(len(rows)):
                s = sc + scs[j]
                nxt.append((idx + (j,), s, (-s, key, j)))
        combos = nxt
    combos.sort(key=lambda t: t[2])
    out_rows, out_scores = [], []
    for idx, sc, _ in combos[:k]:
        out_rows.append(list(itertools.chain.from_iterable(seg_lists[m][0][j] for m, j in enumerate(idx))))
        out_scores.append(sc)
    return out_rows, out_scores
