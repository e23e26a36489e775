"""The batches that tests/test_dedup_cpu.py hands the host twin and tests/test_dedup_gpu.py the kernels: seeded, so both
see the same ones, for both kinds ("bytes": the rows of a corpus, "ids": the rows of a result).

The hash kernel tiles the rows' bytes padded to 8-byte words in tiles of 4096 bytes and slots of 16; the compare tiles the
candidates' elements in tiles of 4096 bytes or 1024 ids.  So the shapes are: row lengths 0, 1, 7, 8, 9, 15, 16, 17
elements; rows one to three elements on either side of one tile and of four tiles; text rows that start at every byte
alignment mod 8; runs of empty rows at the start, in the middle and at the end.  The duplicate patterns: all rows equal,
all distinct, first row equal to last row, pairs adjacent and far apart, a group of 40 equal rows.  The contents that a
hash or a compare could get wrong: rows that differ only in their last element, only in their first, only in a trailing
zero (the hash pads with zeros, so there the length must be doing the work), rows that are each other's 8-byte words
swapped, and one row of 70 000 elements present three times with a fourth copy whose last element differs.

Every batch has at most 12 distinct contents, so that a run with hash_bits 0 (every row collides: one round per distinct
content) stays bounded."""
import numpy as np

KINDS = ("bytes", "ids")
SMALL_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17)
TILE = {"bytes": 4096, "ids": 1024}
V = 1000
MAX_DISTINCT = 12
NAMES = ("lengths", "tile_edges", "four_tile_edges", "alignments", "all_equal", "all_distinct", "first_last", "pairs", "group40",
         "last_element", "first_element", "trailing_zero", "word_swap", "long")


def _row(rng, kind, n):
    """n fresh random elements, none of them zero (so a trailing zero is always one that a case put there)"""
    return [int(x) for x in (rng.integers(1, 256, n) if kind == "bytes" else rng.integers(1, V, n))]


def _case(name, kind, rows):
    dtype = np.uint8 if kind == "bytes" else np.uint32
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    data = np.asarray([x for r in rows for x in r], dtype=dtype)
    return dict(name=name, kind=kind, data=data, offs=offs, rows=[tuple(r) for r in rows], n_distinct=len({tuple(r) for r in rows}),
                vocab_size=V)


def case(name, kind):
    """-> dict(name, kind, data, offs, rows (tuples, for the generator's own test), n_distinct, vocab_size)"""
    rng = np.random.default_rng(4200 + 100 * NAMES.index(name) + KINDS.index(kind))
    tile = TILE[kind]
    if name == "lengths":        # every small length twice, far apart and not in the same order, between runs of empty rows
        a = [_row(rng, kind, n) for n in SMALL_LENGTHS if n]
        rows = [[], []] + a[:4] + [[], [], []] + a[4:] + a[::-1] + [[], []]
    elif name == "tile_edges":   # one tile -3 .. +3 (and the tile itself); five of them present twice
        a = [_row(rng, kind, tile + d) for d in range(-3, 4)]
        rows = a + [_row(rng, kind, 5)] + a[1::2] + a[:2]
    elif name == "four_tile_edges":
        a = [_row(rng, kind, 4 * tile + d) for d in (-3, -2, -1, 1, 2, 3)]
        rows = [[]] + a + [a[0], a[5], a[3]]
    elif name == "alignments":   # rows of 9 and 17 elements back to back: text rows start at every residue mod 8, their copies at another
        a9 = [_row(rng, kind, 9) for _ in range(3)]
        a17 = [_row(rng, kind, 17) for _ in range(3)]
        rows = [a9[i % 3] for i in range(9)] + [_row(rng, kind, 3)] + [a17[i % 3] for i in range(10)] + [a9[i % 3] for i in range(4)]
    elif name == "all_equal":
        rows = [_row(rng, kind, 21)] * 30
    elif name == "all_distinct":
        rows = [_row(rng, kind, n) for n in (0, 1, 2, 8, 16, 16, 23, 24, 25, 100, 100, 4100)]
    elif name == "first_last":
        a = _row(rng, kind, 37)
        rows = [a] + [_row(rng, kind, n) for n in (37, 37, 0, 5, 64, 37, 1, 12, 37)] + [a]
    elif name == "pairs":        # adjacent pairs, and pairs with the whole batch between them
        a = [_row(rng, kind, n) for n in (30, 8, 41, 16, 130, 9)]
        rows = [a[0], a[1], a[1], a[2], a[3], a[3], a[4], a[5], a[5], a[2], a[4], a[0]]
    elif name == "group40":
        g, b, c = _row(rng, kind, 45), _row(rng, kind, 45), _row(rng, kind, 6)
        rows = [[], c, g] + [g if i % 5 else b for i in range(12)] + [[], []] + [g] * 30 + [c, []]
    elif name in ("last_element", "first_element"):
        rows = []
        at = -1 if name == "last_element" else 0
        for n in (1, 8, 9, 16, 17, tile + 1):
            a = _row(rng, kind, n)
            b = list(a)
            b[at] = a[at] % 200 + 1   # another value, not zero
            rows += [a, b]
        rows += rows[2:6] + rows[-1:]
    elif name == "trailing_zero":  # x, x + [0], x + [0, 0] hash to the same sum of terms when they have the same words
        rows = []
        for n in (0, 7, 14, 16):
            a = _row(rng, kind, n)
            rows += [a, a + [0], a + [0, 0]]
        rows += [rows[1], rows[0], rows[5], rows[11]]
    elif name == "word_swap":    # three 8-byte words in three orders (two ids are a word), and a copy of each
        per = 8 if kind == "bytes" else 2
        w = [_row(rng, kind, per) for _ in range(3)]
        a = [w[0] + w[1] + w[2], w[1] + w[0] + w[2], w[2] + w[1] + w[0], w[0] + w[2] + w[1]]
        rows = a + [w[0] + w[1], w[1] + w[0]] + a[::-1] + [w[1] + w[0]]
    elif name == "long":         # about 17 tiles of bytes, 68 of ids
        a = _row(rng, kind, 70_000)
        b = a[:-1] + [a[-1] % 200 + 1]
        rows = [[], _row(rng, kind, 5), a, [], a, _row(rng, kind, 1026), b, a, []]
    else:
        raise KeyError(name)
    return _case(name, kind, [list(r) for r in rows])


def all_cases():
    return [(name, kind) for name in NAMES for kind in KINDS]
