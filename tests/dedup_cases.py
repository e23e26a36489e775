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
content) stays bounded.  past_cap_case, the one batch that takes the capped grids past their caps, has 24 over 530 000 rows
and runs at 3 key bits instead, where its rounds stay under the same 12."""
import numpy as np

import dedup_checker as dc

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


# ---- one batch per kind that takes every capped grid of csrc/dedup.hip past its cap --------------------------------------

HASH_CAP = 2048        # csrc/dedup.hip: kDedupMaxBlocks, of the hash, of the compare and of the kernels with a thread per row
HASH_TILE = 4096       # csrc/dedup.h: kDedupTile, padded bytes
ROW_BLOCK = 256        # csrc/dedup.hip: kDedupBlock, rows per block of dedup_finish / runs / resolve_kernel
BIG = 70_000
PAST_CAP_BITS = 3      # the TGX_DEDUP_HASH_BITS of the collision run over this batch: 8 keys
SHORT_A, SHORT_B = 300_000, 230_000
# the short rows: pool entries of these lengths (two contents of 1, 8 and 17 elements), cycled in this order with one row in
# sixteen drawn at random: runs of one, two and three empty rows, which over 530 000 rows fall at every place of a tile of the
# hash, its edges included (tests/test_dedup_cpu.py looks for one at the edge of a run's second tile)
POOL_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 1, 8, 17)
_LEAN = (0, 1, 0, 0, 2, 9, 0, 1, 2, 0)   # (mostly rows of a word: the padded total stays under two tiles per block)
SHORT_ORDER = (0, 0, 0, 1, 2, 0, 3, 9, 0, 0, 4, 1, 5, 0, 10, 2, 1, 0, 0, 6, 9, 7, 0, 8, 1, 11, 2, 0, 0, 0, 1) + 3 * _LEAN


def pad_bytes(n_elems, elem_bytes):
    """padded bytes of rows of n_elems elements (csrc/dedup.h: dedup_pad_len)"""
    return (np.asarray(n_elems, np.int64) * elem_bytes + 7) & ~7


def _short_part(rng, pool, n):
    """-> (idx int[n] into the pool): the order above, one row in sixteen random, three empty rows at either end"""
    idx = np.tile(np.asarray(SHORT_ORDER), n // len(SHORT_ORDER) + 1)[:n]
    swap = rng.random(n) < 1 / 16
    idx[swap] = rng.integers(0, len(pool), int(swap.sum()))
    idx[:3] = 0
    idx[-3:] = 0
    return idx


def past_cap_case(kind):
    """-> dict(name, kind, data, offs, vocab_size, low_bits, where): one batch that takes every loop of csrc/dedup.hip that a
    capped grid strides over into its second trip.  `where` names the rows the tests look at: rows (all of the long part),
    carry, two_blocks, big (the copies of the 70 000-element row), mid, first, last (copies of it with one element changed),
    edge_rows.

    The batch is SHORT_A short rows, the long part, SHORT_B short rows; more than 256·2048 = 524 288 rows, so the kernels
    with a thread per row go round twice, and the rows around row 524 288 are empty.

    The hash.  A block of dedup_hash_kernel takes per_block = ceil(n_tiles / 2048) consecutive tiles of 4096 padded bytes.
    The padded total is over 2048·4096 + 4096, so per_block = 2: block b takes tiles 2b and 2b + 1.  A last row is sized so
    that n_tiles is odd: the last working block has a run of one tile, and the blocks behind it none.  The long part begins
    with an `align` row sized so that the next row begins at padded byte 2048 of an even tile, the first of a block's run.
    That next row, `carry`, has a tile + 3 elements (4104 padded bytes, 4112 of ids): it ends at byte 6152 (6160) of the
    run's 8192, in the run's second tile, so its sum goes through s_sum[0] and the atomic of thread 0.  The row behind it,
    `two_blocks`, has a tile - 1 elements (4096 padded bytes): it begins at 6152 (6160), in the second tile of block b's
    run, and ends at 10248 (10256), in the first tile of block b + 1's, so its sum arrives by atomics from two blocks.

    The compare.  The 70 000-element row is present n_big = (2048·tile + tile) // 70 000 + 2 times (tile = 4096 bytes or
    1024 ids, the compare's), so that its copies alone, which at 64 key bits are all candidates of the first, total more
    than 2048·tile + tile elements: dedup_compare_kernel goes round twice.  Behind them lie three further copies with one
    element changed: `mid` (element 35 000), `first` and `last`.  Their changed values are chosen so that the top
    PAST_CAP_BITS bits of their hashes equal those of the row they were made from: under that knob they are candidates of
    it in the round in which it is a head, and at least n_big - 1 candidates of 70 000 elements lie before them, that is
    over 2048·tile elements, so every element of theirs is compared in the second trip.

    The collision run.  The long part lies behind SHORT_A short rows, and one of their contents has the key of the
    70 000-element row (the test checks that), so in round one that row is no head, none of its copies is resolved, and
    round two lists them all: over 8 MiB of padded bytes through a compacted list.  There are 12 short contents and 12 long ones (six of a tile -3 .. +3, the
    70 000 and its three changed copies, align and the last row) over 8 keys; the number of rounds is the twin's, and the
    test holds it to MAX_DISTINCT."""
    rng = np.random.default_rng(4900 + KINDS.index(kind))
    dtype, w = (np.uint8, 1) if kind == "bytes" else (np.uint32, 4)
    tile = TILE[kind]
    top = 256 if kind == "bytes" else V
    fresh = lambda n: rng.integers(1, top, n).astype(dtype)
    pool = [fresh(n) for n in POOL_LENGTHS]
    pool_mat = np.zeros((len(pool), max(POOL_LENGTHS)), dtype)
    for p, row in enumerate(pool):
        pool_mat[p, :row.size] = row
    pool_len = np.asarray(POOL_LENGTHS, np.int64)

    def short(n):
        idx = _short_part(rng, pool, n)
        return idx, pool_len[idx]

    def raw(a):
        return a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()

    idx_a, len_a = short(SHORT_A)
    idx_b, len_b = short(SHORT_B)
    # the long part
    big = fresh(BIG)
    want_key = dc.row_hash(raw(big)) >> (64 - PAST_CAP_BITS)

    def changed(at):
        out = big.copy()
        for v in range(1, top):
            out[at] = v
            if v != big[at] and dc.row_hash(raw(out)) >> (64 - PAST_CAP_BITS) == want_key:
                return out
        raise AssertionError("no value gives the key")

    n_big = (HASH_CAP * tile + tile) // BIG + 2
    near = {d: fresh(tile + d) for d in (-3, -2, -1, 1, 2, 3)}
    pad_a = int(pad_bytes(len_a, w).sum())
    run = 2 * HASH_TILE
    align_pad = (HASH_TILE // 2 - pad_a) % run or run
    align = fresh(align_pad // w)
    long_rows = [("align", align), ("carry", near[3]), ("two_blocks", near[-1]), ("near", near[-3]), ("near", near[-2]), ("near", near[1]),
                 ("near", near[2])]
    for q in range(n_big):
        long_rows.append(("big", big))
        if q in (1, n_big // 2):   # the rows of about a tile a second and a third time, between the copies
            long_rows += [("near", near[d]) for d in ((3, -1, -3, -2, 1, 2) if q == 1 else (2, 1, -2, -3, -1, 3))]
    long_rows += [("mid", changed(BIG // 2)), ("first", changed(0)), ("last", changed(BIG - 1)), ("big", big)]
    # the rows around row 524 288, where the kernels with a thread per row begin their second trip, are empty
    at = ROW_BLOCK * HASH_CAP - SHORT_A - (len(long_rows) + 1)
    assert 3 < at < SHORT_B - 6
    idx_b[at - 2:at + 3] = 0
    len_b = pool_len[idx_b]
    # a last long row that makes the number of tiles odd
    total = pad_a + sum(int(pad_bytes(r.size, w)) for _, r in long_rows) + int(pad_bytes(len_b, w).sum())
    n_tiles = -(-(total + 8) // HASH_TILE)
    last = fresh((8 if n_tiles % 2 else 8 + HASH_TILE) // w)
    long_rows.append(("parity", last))

    def short_data(idx, lens):
        return pool_mat[idx][np.arange(pool_mat.shape[1])[None, :] < lens[:, None]]

    lens = np.concatenate([len_a, np.asarray([r.size for _, r in long_rows], np.int64), len_b])
    offs = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = np.concatenate([short_data(idx_a, len_a)] + [r for _, r in long_rows] + [short_data(idx_b, len_b)]).astype(dtype)
    where = dict(rows=np.arange(SHORT_A, SHORT_A + len(long_rows)))
    for name in ("carry", "two_blocks", "mid", "first", "last", "align", "parity"):
        where[name] = SHORT_A + [n for n, _ in long_rows].index(name)
    where["big"] = SHORT_A + np.flatnonzero([n == "big" for n, _ in long_rows])
    pad_offs = np.concatenate([[0], np.cumsum(pad_bytes(lens, w))])
    edges = np.arange(HASH_TILE, int(pad_offs[-1]), HASH_TILE)
    owners = np.searchsorted(pad_offs, edges, side="right") - 1      # the largest row that begins at or before the edge
    where["edge_rows"] = np.unique(np.clip(np.concatenate([owners - 1, owners, owners + 1]), 0, lens.size - 1))
    return dict(name="past_cap", kind=kind, data=data, offs=offs, vocab_size=V, low_bits=PAST_CAP_BITS, where=where, pool=pool,
                n_long_contents=12)
