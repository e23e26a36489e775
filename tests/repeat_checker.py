"""An independent restatement of the repetition statistics (include/tgx.h: the repeated n-grams block): per row the
n-grams are Python tuples in a dict that remembers each gram's first position, coverage is a boolean array per row.
No hashing decides anything here.  row_keys_are_distinct then checks, from dedup_checker's hash, that no two distinct
(row, gram) pairs of a case share a row key: with that the device and the twin, which see keys only, must equal this
exactly.  Nothing here goes through the library or csrc/repeat.h."""
import numpy as np

import dedup_checker as dc
import gram_checker as gc

NAMES = ("grams", "repeated", "multi", "top", "covered", "covered_all")
GOLDEN = 0x9E3779B97F4A7C15
GOPHER_TOP = ((2, .20), (3, .18), (4, .16))
GOPHER_DUP = ((5, .15), (6, .14), (7, .13), (8, .12), (9, .11), (10, .10))


def row_stats(r: tuple, w: int):
    """-> ([grams, repeated, multi, top, covered, covered_all], mask uint8[len(r)]) of one row"""
    n = len(r)
    grams = max(0, n - w + 1)
    count = {}
    mask = np.zeros(n, np.uint8)
    cov, cov_all = np.zeros(n, bool), np.zeros(n, bool)
    for t in range(grams):
        g = r[t:t + w]
        if g in count:          # an earlier position of the row holds it: a repeat
            mask[t] |= 1
            cov[t:t + w] = True
        count[g] = count.get(g, 0) + 1
    for t in range(grams):
        if count[r[t:t + w]] >= 2:
            mask[t] |= 2
            cov_all[t:t + w] = True
    top = max(count.values()) if count else 0
    return [grams, int((mask & 1).sum()), int((mask >> 1).sum()), top, int(cov.sum()), int(cov_all.sum())], mask


def stats(data: np.ndarray, offs: np.ndarray, w: int):
    """-> (table int64[6, S], mask uint8[n_elems])"""
    rows = gc.rows_of(data, offs)
    table = np.zeros((6, len(rows)), np.int64)
    masks = [np.zeros(0, np.uint8)]
    memo = {}
    for i, r in enumerate(rows):
        if r not in memo:
            memo[r] = row_stats(r, w)
        table[:, i], m = memo[r]
        masks.append(m)
    return table, np.concatenate(masks)


def row_keys_are_distinct(data: np.ndarray, offs: np.ndarray, w: int, seed: int) -> bool:
    """rkey = mix(key ^ ((row + 1) · golden)) of every valid gram: as many distinct row keys as distinct (row, gram) pairs"""
    valid, keys = gc.keys_at(data, offs, w, seed)
    row = gc.row_of_element(offs)[valid].astype(np.uint64)
    with np.errstate(over="ignore"):
        rkeys = dc.mix_np(keys ^ ((row + np.uint64(1)) * np.uint64(GOLDEN)))
    pairs = {(i, r[t:t + w]) for i, r in enumerate(gc.rows_of(data, offs)) for t in range(len(r) - w + 1)}
    return np.unique(rkeys).size == len(pairs)


def fracs(table: np.ndarray, elems: np.ndarray, w: int):
    """-> (top_frac, covered_frac, covered_all_frac), float64[S], as RepeatStats defines them"""
    per = np.maximum(elems, 1).astype(np.float64)
    top = np.where(table[3] >= 2, (table[3] * w).astype(np.float64) / per, 0.0)
    return top, table[4].astype(np.float64) / per, table[5].astype(np.float64) / per


def keep_rows(data: np.ndarray, offs: np.ndarray, top=GOPHER_TOP, dup=GOPHER_DUP, literal: bool = False) -> np.ndarray:
    """-> the ascending indices of the rows that repetition_rows keeps, row by row in plain Python"""
    elems = np.diff(offs.astype(np.int64))
    tables = {w: stats(data, offs, w)[0] for w in {w for w, _ in tuple(top) + tuple(dup)}}
    keep = []
    for i in range(elems.size):
        n = max(int(elems[i]), 1)
        bad = any(tables[w][3, i] >= 2 and float(tables[w][3, i] * w) / n > limit for w, limit in top)
        bad = bad or any(float(tables[w][5 if literal else 4, i]) / n > limit for w, limit in dup)
        if not bad:
            keep.append(i)
    return np.asarray(keep, np.int64)


def line_keep_rows(texts: list, max_dup_lines: float = 0.30, max_dup_bytes: float = 0.20):
    """texts: the rows as bytes -> (keep, dup_lines, dup_bytes, lines): a line ends with its '\\n' and keeps it, a trailing
    '\\n' opens no empty last line, and a line is a duplicate iff an earlier line of the same row has exactly its bytes"""
    keep, dl, db, nl = [], [], [], []
    for i, t in enumerate(texts):
        parts = t.split(b"\n")
        lines = [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
        seen, d_lines, d_bytes = set(), 0, 0
        for ln in lines:
            if ln in seen:
                d_lines += 1
                d_bytes += len(ln)
            seen.add(ln)
        dl.append(d_lines)
        db.append(d_bytes)
        nl.append(len(lines))
        if float(d_lines) <= max_dup_lines * float(len(lines)) and float(d_bytes) <= max_dup_bytes * float(len(t)):
            keep.append(i)
    return np.asarray(keep, np.int64), np.asarray(dl, np.int64), np.asarray(db, np.int64), np.asarray(nl, np.int64)
