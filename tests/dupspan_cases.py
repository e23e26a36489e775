"""The batches of tests/test_dupspan_cpu.py (host twin) and tests/test_dupspan_gpu.py (kernels), and the checker both
compare with.  The geometry is tests/repeat_cases.py's, by import: the same chunks, tiles and runs, and a repeat planted
inside a row is a duplicate here too (past_cap: the batch past the grid's cap).  What differs is ACROSS rows, so batches
of elements that are all different but for what is planted are added: paste, a span of w + 3 elements of row 1 pasted
into row 3 (exactly those are covered); short_share, w - 1 elements shared the same way (nothing is flagged); twins, two
identical adjacent rows (the second wholly covered, the first not at all, the opposite of the row mix); no_rows and
empty_rows.  The checker is plain Python: a set of the tuples seen so far in global element order.  No hashing."""
import functools

import numpy as np

import repeat_cases
from repeat_cases import KINDS, pack, widths

OWN = ("paste", "short_share", "twins", "no_rows", "empty_rows")
NAMES = tuple(n for n in repeat_cases.NAMES if n not in OWN) + OWN
ALL = [(name, kind, w) for name in NAMES + ("past_cap",) for kind in KINDS for w in widths(kind)]
STAGES = ["dupspan_keys_kernel", "dupspan_sort", "dupspan_match_kernel", "dupspan_cover_kernel"]
SMALL = 4096   # key_bits 4 and 1 only below this many elements: the walk back is quadratic in a mixed run by design


def case(name, kind, w):
    if name == "past_cap":
        return repeat_cases.past_cap_case(kind, w)
    if name not in OWN:
        return repeat_cases.case(name, kind, w)
    rng = np.random.default_rng(9500 + 100 * OWN.index(name) + 10 * KINDS.index(kind) + w)
    pool = [int(x) for x in rng.permutation(np.arange(1, 256))[:2 * w + 44]]   # all different: no accidental match
    if name in ("no_rows", "empty_rows"):
        rows, where = [[]] * (5 if name == "empty_rows" else 0), {}
    elif name == "twins":
        row = pool[:max(w + 5, 40)]
        rows, where = [pool[-2:], row, row, [], row[:w], row], {}
    else:
        span, at = (w + 3 if name == "paste" else w - 1), 5
        donor, target = pool[:w + 12], pool[w + 12:-2]
        target[at:at + span] = donor[4:4 + span]
        rows = [pool[-2:], donor, [], target, []]
        where = dict(first=len(rows[0]) + len(donor) + at, span=span)
    data, offs = pack(rows, kind)
    return dict(name=name, kind=kind, width=w, data=data, offs=offs, rows=[tuple(r) for r in rows], where=where)


def key_bits_of(n_elems):
    return (64, 20, 4, 1) if n_elems < SMALL else (64, 20)


def check(data, offs, w):
    """-> (table int64[3, S], mask uint8[N]) by the definitions alone"""
    o = [int(x) for x in offs]
    S, elems = len(o) - 1, data.tolist()
    table, mask, covered, seen = np.zeros((3, S), np.int64), np.zeros(len(elems), np.uint8), np.zeros(len(elems), bool), set()
    for i in range(S):
        for e in range(o[i], o[i + 1] - w + 1):
            gram = tuple(elems[e:e + w])
            if gram in seen:
                mask[e] |= 1
                covered[e:e + w] = True
                table[1, i] += 1
            seen.add(gram)
        table[0, i] = max(0, o[i + 1] - o[i] - w + 1)
        table[2, i] = covered[o[i]:o[i + 1]].sum()
    mask[covered] |= 2
    return table, mask


@functools.lru_cache(maxsize=None)
def checked_case(name, kind, w):
    """a case with the checker's answer as c["want"]: computed once, shared by the tests, never changed"""
    c = case(name, kind, w)
    c["want"] = check(c["data"], c["offs"], w)
    for a in (c["data"], c["offs"]) + c["want"]:
        a.setflags(write=False)
    return c
