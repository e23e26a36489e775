"""The batches that tests/test_repeat_cpu.py hands the host twin and tests/test_repeat_gpu.py the kernels: seeded, so both
see the same ones, for both kinds ("bytes": the rows of a corpus, "ids": the rows of a result) and for every width of
WIDTHS (1, 2, 5, 13 and the widest: 16 ids, 64 bytes).

The kernels lay the ELEMENTS of all rows end to end, a wave takes a chunk of 64, a block a tile of 256 and, past the
grid's cap, a run of consecutive tiles; the cover kernel looks one chunk back for the repeats that reach into its own,
cuts that window at the row's start, and a row's sums leave the wave by a plain store when the row lies inside the
chunk and by an atomic add otherwise.  So the shapes are:
  short        rows of 0 .. w + 2 elements over two symbols, between runs of empty rows at the start, in the middle and at the end
  all_short    every row shorter than w: no gram at all
  one_element  rows of one repeated element, of w + 1 and of w + 40 elements
  period3      a row of period 3
  twins        two identical adjacent rows without an internal repeat: nothing may be flagged (the row mix)
  lanes        a repeat that begins on the last lane of a chunk and one that begins on the first lane of the next
  reach        a repeat that begins exactly w - 1 elements before a chunk's first element (63 at the widest byte width):
               that element is covered, the one after it is not
  row_end      a row whose last valid gram is a repeat, followed at once by a row without repeats, whose first w - 1
               elements must not be covered
  edges_*      rows that end one to three elements on either side of a chunk's edge, a tile's and two tiles', each with
               a repeat astride the edge it crosses and one as its last gram
  alignments   rows over two symbols that start at each of the four byte alignments
  five_tiles   a row of five tiles of one element among short ones: one run of about 1 280
past_cap_case has more tiles than the grid has blocks.  c["repeat_at"] lists elements at which a repeat begins for
certain, c["clean_rows"] rows in which nothing may be flagged or covered."""
import numpy as np

import gram_cases
from gram_cases import CAP, CHUNK, DTYPE, KINDS, RUN, TILE, V, W_MAX, pack

NAMES = ("short", "all_short", "one_element", "period3", "twins", "lanes", "reach", "row_end", "edges_chunk", "edges_tile", "edges_two_tiles",
         "alignments", "five_tiles")
EDGES = {"edges_chunk": CHUNK, "edges_tile": TILE, "edges_two_tiles": 2 * TILE}


def widths(kind):
    return (1, 2, 5, 13, W_MAX[kind])


def _row(rng, kind, n):
    return [int(x) for x in (rng.integers(1, 256, n) if kind == "bytes" else rng.integers(1, V, n))]


def _two(rng, kind, n):
    return [int(x) for x in rng.choice([7, 9], n)]


def _distinct(rng, kind, n):
    """n different elements in a seeded order"""
    assert n <= 255
    return [int(x) for x in rng.permutation(np.arange(1, 256 if kind == "bytes" else V))[:n]]


def _copy(row, src, dst, w):
    """afterwards row[dst : dst + w] == row[src : src + w], also where the two overlap (src < dst)"""
    assert 0 <= src < dst and dst + w <= len(row)
    for t in range(w):
        row[dst + t] = row[src + t]


class _Batch:
    def __init__(self):
        self.rows, self.cum, self.plants, self.clean = [], 0, [], []

    def add(self, row, clean=False):
        self.rows.append(list(row))
        self.cum += len(row)
        if clean:
            self.clean.append(len(self.rows) - 1)
        return len(self.rows) - 1

    def repeat(self, r, src, dst, w):
        _copy(self.rows[r], src, dst, w)
        self.plants.append((r, src, dst))


def case(name, kind, w):
    """-> dict(name, kind, width, data, offs, rows (tuples), repeat_at, clean_rows, where)"""
    rng = np.random.default_rng(9100 + 1000 * NAMES.index(name) + 100 * KINDS.index(kind) + w)
    b, where = _Batch(), {}
    if name == "short":
        a = [_two(rng, kind, n) for n in range(1, w + 3)]
        half = len(a) // 2
        for r in [[], [], []] + a[:half] + [[], []] + a[half:] + [[]] + [_two(rng, kind, n) for n in range(w + 2, 0, -1)] + [[], []]:
            b.add(r)
    elif name == "all_short":
        for n in (0, 0, w - 1, 1, w // 2, 0, 2, w - 1, w - 1, 0):
            b.add(_two(rng, kind, min(n, w - 1)))
    elif name == "one_element":
        b.add(_row(rng, kind, 3))
        where["short"] = b.add([5] * (w + 1))
        b.add([])
        where["long"] = b.add([5] * (w + 40))
        b.add(_row(rng, kind, 2))
    elif name == "period3":
        b.add(_row(rng, kind, 4))
        where["row"] = b.add([(11, 12, 13)[t % 3] for t in range(50 + w)])
        b.add(_row(rng, kind, 1))
    elif name == "twins":
        b.add(_row(rng, kind, 2))
        row = _distinct(rng, kind, max(w + 5, 40))
        b.add(row, clean=True)
        b.add(row, clean=True)
        b.add([])
        b.add(row[:w], clean=True)
        b.add(row, clean=True)
    elif name == "lanes":           # one row from element 0 on, so a row's element t is lane t % 64
        r = b.add(_row(rng, kind, 4 * CHUNK + w + 10))
        b.repeat(r, 3, CHUNK - 1, w)                    # begins on the last lane of chunk 0
        b.repeat(r, CHUNK + w + 3, 3 * CHUNK, w)        # begins on the first lane of chunk 3
        b.add(_row(rng, kind, 5))
    elif name == "reach":           # distinct elements but for the one repeat, so `covered` is w exactly where 2 w + 2 <= 255 fits
        b.add(_row(rng, kind, 7))
        start = b.cum
        edge = (start // CHUNK + 3) * CHUNK
        n = edge - start + 3
        base = _distinct(rng, kind, min(n, 255))
        r = b.add((base * (n // len(base) + 1))[:n])    # (period 255 when longer: no gram of the row's first part repeats before the plant)
        b.repeat(r, 1, edge - (w - 1) - start, w)
        where["row"], where["edge"] = r, edge
        b.add(_row(rng, kind, 3))
    elif name == "row_end":
        b.add(_row(rng, kind, 9))
        n = 3 * w + 20
        r = b.add(_row(rng, kind, n))
        b.repeat(r, 2, n - w, w)                        # the row's last valid gram
        where["after"] = b.add(_distinct(rng, kind, w + 3), clean=True)
        b.add(_row(rng, kind, 4))
    elif name.startswith("edges_"):
        edge = EDGES[name]
        for d in (-3, -2, -1, 0, 1, 2, 3):
            for n in (0, 2, w, w + 1):
                b.add(_row(rng, kind, n))
            crossed = (b.cum // edge + 2) * edge
            start = b.cum
            r = b.add(_row(rng, kind, crossed + (1 if 2 * w <= edge else 2) * edge + d - start))   # (room for both repeats)
            b.repeat(r, 1, crossed - max(1, w // 2) - start, w)     # astride the edge
            b.repeat(r, 5, len(b.rows[r]) - w, w)                   # the row's last gram, d elements from the edge
        b.add(_row(rng, kind, 3))
    elif name == "alignments":
        for n in (9, 10, 11, 13, 8, 7, 9, 10, 5, 4, 6):
            b.add(_two(rng, kind, n + w))
    elif name == "five_tiles":
        for n in (0, 7, 3, 12):
            b.add(_row(rng, kind, n))
        where["row"] = b.add([9] * (5 * TILE))
        for n in (1, 0, 9, 30):
            b.add(_row(rng, kind, n))
    else:
        raise KeyError(name)
    data, offs = pack(b.rows, kind)
    # (a later plant may have written over an earlier one: what still holds at the end is a repeat for certain)
    repeat_at = np.asarray([int(offs[r]) + dst for r, src, dst in b.plants if b.rows[r][dst:dst + w] == b.rows[r][src:src + w]], np.int64)
    return dict(name=name, kind=kind, width=w, data=data, offs=offs, rows=[tuple(r) for r in b.rows], repeat_at=repeat_at,
                clean_rows=np.asarray(b.clean, np.int64), where=where)


def all_cases():
    return [(name, kind, w) for name in NAMES for kind in KINDS for w in widths(kind)]


def past_cap_case(kind, w):
    """tests/gram_cases.py's past-cap geometry (2048·256 + 2·256 + 70 elements: a block takes two tiles) with repeats planted
    in its three marked rows: where["inside"], a row from a run's first tile into its second, with a repeat astride the
    tile's edge; where["straddle"], a row from one block's run into the next, so that two blocks add to one row's sums, with
    repeats on either side of the run's edge and astride it; where["long"], a row over the runs of four blocks with a
    repeat astride every tile edge inside it.  Every fifth filler row is over two symbols."""
    c = gram_cases.past_cap_case(kind)
    rng = np.random.default_rng(9900 + 100 * KINDS.index(kind) + w)
    data, offs = c["data"].copy(), c["offs"]
    o = offs.astype(np.int64)
    for i in range(0, o.size - 1, 5):
        data[o[i]:o[i + 1]] = rng.choice([7, 9], int(o[i + 1] - o[i]))
    repeat_at = []
    for key in ("inside", "straddle", "long"):
        a, z = int(o[c["where"][key]]), int(o[c["where"][key] + 1])
        row = [int(x) for x in data[a:z]]
        dsts = [e - max(1, w // 2) - a for e in range((a // TILE + 1) * TILE, z - w, TILE)]
        if key == "straddle":       # before the run's edge, astride it and behind it, none over another
            e = (a // RUN + 1) * RUN - a
            dsts = [max(2, e - max(1, w // 2) - w - 2), e - max(1, w // 2), e + w + 3]
        done = []
        for k, dst in enumerate(dsts):
            if dst > 1 + k and dst + w <= len(row):
                _copy(row, 1 + k, dst, w)
                done.append((1 + k, dst))
        repeat_at += [a + dst for src, dst in done if row[dst:dst + w] == row[src:src + w]]   # (what a later plant left standing)
        data[a:z] = row
    return dict(name="past_cap", kind=kind, width=w, data=data, offs=offs, repeat_at=np.asarray(repeat_at, np.int64),
                clean_rows=np.zeros(0, np.int64), where=c["where"])
