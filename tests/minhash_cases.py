"""The batches that tests/test_minhash_cpu.py hands the host twins and tests/test_minhash_gpu.py the kernels: seeded, so
both see the same ones, for both kinds ("bytes": the rows of a corpus, "ids": the rows of a result).

The signature kernel lays the rows' shingle positions end to end (a row of n elements has max(1, n - w + 1) of them), a
wave takes a chunk of 64 positions, a block a tile of 256, and a row's minima leave the wave by a plain store when the
row lies inside the chunk and by an atomic minimum otherwise.  So the shapes are: rows of 0 .. w + 2 elements for w = 1, 5
and the widest (16 ids, 64 bytes) between runs of empty rows at the start, in the middle and at the end; rows that END one
to three positions on either side of a chunk's edge, of a tile's and of four tiles'; one row that owns about five tiles
among short rows; a row of one repeated element; rows that differ only in trailing zero elements; two rows equal but for
one element; permuted copies; the smallest and the largest element values.  K is 1, 64, 65, 128 or 250, so the lanes'
permutations are a part of one group, whole groups and a group with a tail; the bands are 1, K and 25 of 250."""
import numpy as np

KINDS = ("bytes", "ids")
CHUNK, TILE = 64, 256
V = 1000
W_MAX = {"bytes": 64, "ids": 16}
TOP = {"bytes": 255, "ids": V - 1}
EDGES = (CHUNK, TILE, 4 * TILE)
NAMES = ("short_w1", "short_w5", "short_wmax", "edges_chunk", "edges_tile", "edges_four_tiles", "long_among_short", "contents", "extremes")
# name -> (width or None for the widest, K, bands)
SHAPE = {"short_w1": (1, 64, (1, 64)), "short_w5": (5, 65, (1, 65, 5)), "short_wmax": (None, 1, (1,)), "edges_chunk": (5, 128, (32,)),
         "edges_tile": (3, 65, (13,)), "edges_four_tiles": (5, 64, (16,)), "long_among_short": (5, 250, (1, 250, 25)),
         "contents": (5, 128, (1, 128, 32)), "extremes": (2, 250, (25,))}


def _row(rng, kind, n):
    return [int(x) for x in (rng.integers(1, 256, n) if kind == "bytes" else rng.integers(1, V, n))]


def positions(n, w):
    return max(1, n - w + 1)


def width_of(name, kind):
    return SHAPE[name][0] or W_MAX[kind]


def case(name, kind):
    """-> dict(name, kind, data, offs, rows (tuples), width, n_perm, bands (a tuple), vocab_size)"""
    rng = np.random.default_rng(5300 + 100 * NAMES.index(name) + KINDS.index(kind))
    w = width_of(name, kind)
    _, K, bands = SHAPE[name]
    if name.startswith("short_"):   # every length 0 .. w + 2 twice, the second time in another order, between runs of empty rows
        a = [_row(rng, kind, n) for n in range(1, w + 3)]
        half = len(a) // 2
        rows = [[], [], []] + a[:half] + [[], []] + a[half:] + [[]] + a[::-1] + [[], []]
    elif name.startswith("edges_"):  # fillers of a few positions, then a row that ends at edge + d
        edge = EDGES[("edges_chunk", "edges_tile", "edges_four_tiles").index(name)]
        rows, cum = [], 0
        for d in (-3, -2, -1, 0, 1, 2, 3):
            for n in (0, 2, w, w + 1):
                rows.append(_row(rng, kind, n))
                cum += positions(n, w)
            target = (cum // edge + 2) * edge + d
            m = target - cum
            rows.append(_row(rng, kind, m + w - 1))
            cum = target
        rows.append(_row(rng, kind, 3))
    elif name == "long_among_short":
        long_row = _row(rng, kind, 5 * TILE + 37 + w - 1)
        rows = [_row(rng, kind, n) for n in (0, 7, 3, 12)] + [long_row] + [_row(rng, kind, n) for n in (1, 0, 9, 30)] + [long_row[:700]]
    elif name == "contents":
        x, y = _row(rng, kind, 3), _row(rng, kind, 40)
        one = _row(rng, kind, 1) * 300                         # one distinct shingle
        z = _row(rng, kind, 200)
        z1 = list(z)
        z1[100] = z[100] % 200 + 1                             # equal but for one element
        blocks = [_row(rng, kind, 25) for _ in range(8)]
        perm = [blocks[i] for i in (3, 0, 7, 1, 6, 2, 5, 4)]   # a permuted copy: most shingles are shared
        rows = [x, x + [0], x + [0, 0], y, y + [0], y + [0, 0], one, one[:77], z, z1, sum(blocks, []), sum(perm, []), z, [], x, one, []]
    elif name == "extremes":
        top = TOP[kind]
        rows = [[0] * 9, [top] * 9, [0, top] * 6, [top, 0] * 6, [0], [top], [0, 0], [], [top] * 130, [0] * 130, [0, top] * 6]
    else:
        raise KeyError(name)
    dtype = np.uint8 if kind == "bytes" else np.uint32
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    data = np.asarray([x for r in rows for x in r], dtype=dtype)
    return dict(name=name, kind=kind, data=data, offs=offs, rows=[tuple(r) for r in rows], width=w, n_perm=K, bands=bands, vocab_size=V)


def all_cases():
    return [(name, kind) for name in NAMES for kind in KINDS]
