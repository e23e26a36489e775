"""The batches that tests/test_gram_cpu.py hands the host twins and tests/test_gram_gpu.py the kernels: seeded, so both see
the same ones, for both kinds ("bytes": the rows of a corpus, "ids": the rows of a result).  A case is a source to probe
and a small eval source whose gram set it is probed against.

The kernels lay the ELEMENTS of all rows end to end, a wave takes a chunk of 64, a block a tile of 256 and, past the
grid's cap, a run of consecutive tiles; a row's hits leave the wave by a plain store when the row lies inside the chunk
and by an atomic add otherwise.  So the shapes are: rows of 0 .. w + 2 elements for w = 1, 5, 13 and the widest (16 ids,
64 bytes) between runs of empty rows at the start, in the middle and at the end; rows that END one to three elements on
either side of a chunk's edge, of a tile's and of two tiles', each crossing an edge with a planted gram of the eval set
astride it; a batch in which every row is shorter than w (an empty set, no hit); rows that start at each of the four byte
alignments; one row of about five tiles among short ones.  past_cap_case has more tiles than the grid has blocks.
Behind them, key sets for tgx_gramset_create_from_keys that no source would give."""
import numpy as np

KINDS = ("bytes", "ids")
CHUNK, TILE = 64, 256          # csrc/gram.h: kGramChunk, kGramTile
CAP = 2048                     # csrc/gram.hip: kGramMaxBlocks
MAX_BITS = 28                  # csrc/gram.h: kGramMaxBits
V = 1000
W_MAX = {"bytes": 64, "ids": 16}
DTYPE = {"bytes": np.uint8, "ids": np.uint32}
EDGES = {"edges_chunk": CHUNK, "edges_tile": TILE, "edges_two_tiles": 2 * TILE}
# name -> width (None: the widest)
WIDTH = {"short_w1": 1, "short_w5": 5, "short_w13": 13, "short_wmax": None, "edges_chunk": 5, "edges_tile": 3, "edges_two_tiles": 13,
         "all_short": 5, "alignments": 5, "long_among_short": 13}
NAMES = tuple(WIDTH)


def _row(rng, kind, n):
    return [int(x) for x in (rng.integers(1, 256, n) if kind == "bytes" else rng.integers(1, V, n))]


def pack(rows, kind):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.asarray([x for r in rows for x in r], dtype=DTYPE[kind]), offs


def width_of(name, kind):
    return WIDTH[name] or W_MAX[kind]


def gram_count(n, w):
    return max(0, n - w + 1)


class _Batch:
    """rows of the source, rows of the eval set, and where grams of the eval set were planted in the source"""

    def __init__(self, rng, kind, w):
        self.rng, self.kind, self.w = rng, kind, w
        self.rows, self.eval_rows, self.plants, self.cum = [], [], [], 0

    def add(self, row):
        self.rows.append(list(row))
        self.cum += len(row)
        return len(self.rows) - 1

    def plant(self, r, at):
        """a fresh gram into row r at element `at` of the row, and into an eval row between other elements"""
        g = _row(self.rng, self.kind, self.w)
        assert 0 <= at and at + self.w <= len(self.rows[r])
        self.rows[r][at:at + self.w] = g
        self.eval_rows.append(_row(self.rng, self.kind, 3) + g + _row(self.rng, self.kind, 2))
        self.plants.append((r, at))

    def done(self, name):
        data, offs = pack(self.rows, self.kind)
        eval_data, eval_offs = pack(self.eval_rows, self.kind)
        planted = np.asarray([int(offs[r]) + at for r, at in self.plants], np.int64)
        return dict(name=name, kind=self.kind, data=data, offs=offs, rows=[tuple(r) for r in self.rows], width=self.w, eval_data=eval_data,
                    eval_offs=eval_offs, planted=planted, vocab_size=V)


def case(name, kind):
    """-> dict(name, kind, data, offs, rows (tuples), width, eval_data, eval_offs, planted (elements at which a gram of
    the eval set begins for certain), vocab_size)"""
    rng = np.random.default_rng(7300 + 100 * NAMES.index(name) + KINDS.index(kind))
    w = width_of(name, kind)
    b = _Batch(rng, kind, w)
    if name.startswith("short_"):    # every length 0 .. w + 2 twice, the second time in another order, between runs of empty rows
        a = [_row(rng, kind, n) for n in range(1, w + 3)]
        half = len(a) // 2
        for r in [[], [], []] + a[:half] + [[], []] + a[half:] + [[]] + a[::-1] + [[], []]:
            b.add(r)
        # the eval set: the row of exactly w elements, the longest but for its first element, a row too short, an empty one
        b.eval_rows += [list(a[w - 1]), list(a[w + 1][1:]), _row(rng, kind, w - 1), [], _row(rng, kind, w + 4)]
    elif name.startswith("edges_"):  # fillers, then a row that crosses one edge and ends at the next but one + d
        edge = EDGES[name]
        for d in (-3, -2, -1, 0, 1, 2, 3):
            for n in (0, 2, w, w + 1):
                b.add(_row(rng, kind, n))
            crossed = (b.cum // edge + 2) * edge
            start = b.cum
            r = b.add(_row(rng, kind, crossed + edge + d - start))
            b.plant(r, crossed - max(1, w // 2) - start)           # astride the edge
            b.plant(r, len(b.rows[r]) - w)                         # the row's last gram, d elements from the edge
        b.add(_row(rng, kind, 3))
        b.eval_rows += [[], _row(rng, kind, 2)]
    elif name == "all_short":
        for n in (0, 0, 4, 1, 3, 0, 2, 4, 4, 0):
            b.add(_row(rng, kind, n))
        b.eval_rows += [list(b.rows[2]), [], list(b.rows[4]), _row(rng, kind, 4)]
    elif name == "alignments":
        for n in (9, 10, 11, 13, 8, 7, 9, 10, 5, 4, 6):
            r = b.add(_row(rng, kind, n))
            if n >= w:
                b.plant(r, 0)
            if n >= 2 * w:
                b.plant(r, n - w)
    elif name == "long_among_short":
        for n in (0, 7, 3, 12):
            b.add(_row(rng, kind, n))
        start = b.cum
        r = b.add(_row(rng, kind, 5 * TILE + 37))
        for at in (0, TILE - start - 6, 2 * TILE - start - w, 3 * TILE - start, 3 * TILE + CHUNK - start - 1, len(b.rows[r]) - w):
            b.plant(r, at)
        for n in (1, 0, 9, 30):
            b.add(_row(rng, kind, n))
        b.add(b.rows[r][:700])
        b.eval_rows += [list(b.rows[r][900:960]), []]
    else:
        raise KeyError(name)
    return b.done(name)


def all_cases():
    return [(name, kind) for name in NAMES for kind in KINDS]


# ---- past the cap of csrc/gram.hip's grid ----------------------------------------------------------------------------------

PAST_W = 5
RUN = 2 * TILE                            # the elements of a block's run of per_block = 2 tiles
PAST_N = CAP * TILE + 2 * TILE + 70       # 2050 tiles and 70 elements: the last tile's third and fourth chunk are empty


def past_cap_case(kind):
    """-> a case dict with `where`: PAST_N elements, so that n_tiles = 2051 is over the grid's 2048 blocks: per_block = 2,
    block b takes tiles 2b and 2b + 1 (a run of 512 elements), block 1025 has a run of one short tile, of which two waves
    find nothing, and the blocks behind it have none.  The rows, a few thousand: fillers of 100 to 300 elements and rows
    of 0, 1, w - 1 and w; where["inside"], a row over elements 200 .. 350 of a run, so from the run's first tile into its
    second; where["straddle"], a row over elements 400 .. 700 of a run, so from one block's run into the next: two blocks
    add to one count; where["long"], a row of 5·256 + 37 elements over the runs of four blocks.  The eval set: 16 elements
    around every tile edge inside those three rows, 30 slices of 5 to 40 elements from anywhere, an empty row and one of
    three elements."""
    rng = np.random.default_rng(7900 + KINDS.index(kind))
    w = PAST_W
    lens, where, cum = [], {}, 0

    def add(n):
        nonlocal cum
        lens.append(n)
        cum += n
        return len(lens) - 1

    def fill_to(target):
        while target - cum > 420:
            add(int(rng.integers(100, 300)))
        for n in (0, 1, w - 1, w):
            add(n)
        assert target - cum >= 1
        add(target - cum)

    def next_run():
        return (cum // RUN + 2) * RUN

    for n in (0, 0, 0):
        add(n)
    fill_to(300 * RUN + 17)
    fill_to(next_run() + 200)
    where["inside"] = add(150)
    fill_to(next_run() + 400)
    where["straddle"] = add(300)
    fill_to(next_run() + 300)
    where["long"] = add(5 * TILE + 37)
    fill_to(PAST_N - 10)
    for n in (4, 3, 2, 1, 0, 0):
        add(n)
    assert cum == PAST_N
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = (rng.integers(1, 256, PAST_N) if kind == "bytes" else rng.integers(1, V, PAST_N)).astype(DTYPE[kind])
    slices = []
    for r in where.values():
        a, z = int(offs[r]), int(offs[r + 1])
        slices += [(e - 8, e + 8) for e in range((a // TILE + 1) * TILE, z, TILE)]
    for _ in range(30):
        a = int(rng.integers(0, PAST_N - 40))
        slices.append((a, a + int(rng.integers(5, 41))))
    eval_rows = [[int(x) for x in data[a:z]] for a, z in slices] + [[], [int(x) for x in data[1000:1003]]]
    eval_data, eval_offs = pack(eval_rows, kind)
    planted = np.concatenate([np.arange(a, z - w + 1) for a, z in slices[:len(slices) - 30]]).astype(np.int64)
    return dict(name="past_cap", kind=kind, data=data, offs=offs, width=w, eval_data=eval_data, eval_offs=eval_offs, planted=planted, vocab_size=V,
                where=where)


# ---- key sets that no source would give (tgx_gramset_create_from_keys) ---------------------------------------------------

HOSTILE = ("empty", "one", "ends", "n255", "n256", "n257", "one_bucket", "unsorted_dups")


def ceil_log2(n):
    return (n - 1).bit_length()


def dir_bits(n_keys):
    return 0 if n_keys <= 1 else min(MAX_BITS, ceil_log2(n_keys))


def hostile_keys(name):
    """-> uint64 keys as a caller hands them over: the empty set; one key; the keys 0 and 2^64 - 1; 2^8 - 1, 2^8 and 2^8 + 1
    keys, around which the directory's bits step from 8 to 9; 300 keys that share their top 28 bits, so one bucket holds
    them all and every other bucket is empty; unsorted keys with duplicates."""
    rng = np.random.default_rng(8100 + HOSTILE.index(name))
    rand = lambda n: rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if name == "empty":
        return np.zeros(0, np.uint64)
    if name == "one":
        return rand(1)
    if name == "ends":
        return np.asarray([0, (1 << 64) - 1], np.uint64)
    if name in ("n255", "n256", "n257"):
        keys = np.unique(rand(400))[:int(name[1:])]
        return keys[rng.permutation(keys.size)]
    if name == "one_bucket":
        low = np.unique(rng.integers(0, 1 << 36, 400, dtype=np.uint64))[:300]
        return (np.uint64(0xABCDEF1) << np.uint64(36)) | low[rng.permutation(300)]
    if name == "unsorted_dups":
        keys = rand(100)
        return keys[rng.integers(0, 100, 350)]
    raise KeyError(name)


def hostile_probes(keys):
    """-> uint64 probe keys: every stored key, every stored key + 1 and - 1 (wrapping), 0 and 2^64 - 1, and 500 keys from
    anywhere, which with few keys stored fall into empty buckets"""
    rng = np.random.default_rng(8200 + keys.size)
    keys = np.asarray(keys, np.uint64)
    with np.errstate(over="ignore"):
        near = np.concatenate([keys, keys + np.uint64(1), keys - np.uint64(1)])
    return np.concatenate([near, np.asarray([0, (1 << 64) - 1], np.uint64), rng.integers(0, 1 << 64, 500, dtype=np.uint64)])
