"""The batches that tests/test_minhash_cpu.py hands the host twins and tests/test_minhash_gpu.py the kernels: seeded, so
both see the same ones, for both kinds ("bytes": the rows of a corpus, "ids": the rows of a result).

The signature kernel lays the rows' shingle positions end to end (a row of n elements has max(1, n - w + 1) of them), a
wave takes a chunk of 64 positions, a block a tile of 256, and a row's minima leave the wave by a plain store when the
row lies inside the chunk and by an atomic minimum otherwise.  So the shapes are: rows of 0 .. w + 2 elements for w = 1, 5
and the widest (16 ids, 64 bytes) between runs of empty rows at the start, in the middle and at the end; rows that END one
to three positions on either side of a chunk's edge, of a tile's and of four tiles'; one row that owns about five tiles
among short rows; a row of one repeated element; rows that differ only in trailing zero elements; two rows equal but for
one element; permuted copies; the smallest and the largest element values.  K is 1, 64, 65, 128 or 250, so the lanes'
permutations are a part of one group, whole groups and a group with a tail; the bands are 1, K and 25 of 250.

Behind them: the WIDE names, earlier shapes under K = 257 .. 1024; past_cap_case, one batch per kind with more shingle
positions than the signature kernel's capped grid takes in one tile per block; and, for the calls that take any
signatures, signatures made with numpy past the caps of the kernels with a thread or a wave per row, chains of heads as
deep as there are rows, and heads that are no earlier row."""
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


# K = 257 .. 1024: P = ceil(K / 64) = 5 .. 16 permutations per lane, the kernel's <*, 8> and <*, 16>, with and without a tail
# (257 = 4·64 + 1, 513 = 8·64 + 1, 1000 = 15·64 + 40), and the verify's loop over the K values five to sixteen steps long.
# name -> (the shape whose rows it takes, K, bands)
WIDE = {"wide_257": ("edges_chunk", 257, (1, 257)), "wide_512": ("long_among_short", 512, (128,)), "wide_513": ("contents", 513, (1, 27)),
        "wide_1000": ("edges_chunk", 1000, (250, 8)), "wide_1024": ("contents", 1024, (32,))}
WIDE_NAMES = tuple(WIDE)


def _row(rng, kind, n):
    return [int(x) for x in (rng.integers(1, 256, n) if kind == "bytes" else rng.integers(1, V, n))]


def positions(n, w):
    return max(1, n - w + 1)


def width_of(name, kind):
    return SHAPE[name][0] or W_MAX[kind]


def case(name, kind):
    """-> dict(name, kind, data, offs, rows (tuples), width, n_perm, bands (a tuple), vocab_size)"""
    if name in WIDE:     # the rows of an earlier shape (from a seed of their own) under a wide K
        base, K, bands = WIDE[name]
        rng = np.random.default_rng(5300 + 100 * (len(NAMES) + WIDE_NAMES.index(name)) + KINDS.index(kind))
    else:
        base, (_, K, bands) = name, SHAPE[name]
        rng = np.random.default_rng(5300 + 100 * NAMES.index(name) + KINDS.index(kind))
    w = width_of(base, kind)
    rows = _rows(base, kind, rng, w)
    dtype = np.uint8 if kind == "bytes" else np.uint32
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    data = np.asarray([x for r in rows for x in r], dtype=dtype)
    return dict(name=name, kind=kind, data=data, offs=offs, rows=[tuple(r) for r in rows], width=w, n_perm=K, bands=bands, vocab_size=V)


def _rows(name, kind, rng, w):
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
    return rows


def all_cases():
    return [(name, kind) for name in NAMES for kind in KINDS]


def wide_cases():
    return [(name, kind) for name in WIDE_NAMES for kind in KINDS]


# ---- past the caps of csrc/minhash.hip's grids ---------------------------------------------------------------------------

SIG_CAP = 2048          # csrc/minhash.hip: kMinhashMaxBlocks, of minhash_sig_kernel and of the kernels with a thread per row or key
VERIFY_CAP = 16384      # csrc/minhash.hip: launch_minhash_verify's grid_for(n_rows, 4, 8 * kMinhashMaxBlocks), four rows per block
PAST_W, PAST_K = 2, 65
RUN = 2 * TILE          # the positions of a block's run of per_block = 2 tiles
PAST_M = SIG_CAP * TILE + 2 * TILE + 70   # 2050 tiles and 70 positions: the last tile's third and fourth chunk are empty


def past_cap_case(kind):
    """-> dict(name, kind, data, offs, width, n_perm, vocab_size, where): PAST_M shingle positions, so that
    minhash_sig_kernel's n_tiles = 2051 is over its 2048 blocks: per_block = 2, block b takes tiles 2b and 2b + 1 (a run of
    512 positions), block 1025 has a run of one tile, of which two waves find nothing, and the blocks behind it have none.
    In a run's second tile a wave finds its chunk's owners by galloping from the `hi` of its chunk of the first tile.

    w = 2 over 16 element values (the eight lowest and the eight highest), so there are at most 273 distinct shingles.
    The rows, a few thousand: fillers of 100 to 300 positions; at the start, before every row named below and at the end
    rows of 0 .. w + 2 elements; rows that end d = -3 .. 3 positions from position 256 of a run (the edge at which the
    second tile begins), from 320 (a chunk edge inside the second tile) and from 512 (the second tile's end, where the
    next block's run begins): where["ends"] = (row, edge, d); where["inside"], a row of 410 positions from position 30 of a
    run on, so over both tiles of one block's run (with two tiles to a run, no longer row lies inside one);
    where["straddle"], a row of 5·256 + 37 positions from position 300 of a run on, so over the runs of four blocks."""
    rng = np.random.default_rng(5900 + KINDS.index(kind))
    w = PAST_W
    lens, where = [], dict(ends=[])
    cum = 0

    def add(n):
        nonlocal cum
        lens.append(n)
        cum += positions(n, w)
        return len(lens) - 1

    def end_at(target):
        """fillers, the short rows and one row that ends at position `target`"""
        while target - cum > 420:
            add(int(rng.integers(100, 300)) + w - 1)
        for n in range(w + 3):
            add(n)
        assert target - cum >= 1
        return add(target - cum + w - 1)

    def next_run(lead=2):
        return (cum // RUN + lead) * RUN

    for n in (0, 0, 0, 1, 2, 3, 4):
        add(n)
    end_at(300 * RUN + 17)
    for edge in (TILE, TILE + CHUNK, RUN):
        for d in (-3, -2, -1, 0, 1, 2, 3):
            where["ends"].append((end_at(next_run() + edge + d), edge, d))
    end_at(next_run() + 30)
    where["inside"] = add(410 + w - 1)
    end_at(next_run() + 300)
    where["straddle"] = add(5 * TILE + 37 + w - 1)
    end_at(PAST_M - 10)
    for n in (4, 3, 2, 1, 0, 0, 0):
        add(n)
    assert cum == PAST_M
    top = TOP[kind]
    alphabet = np.asarray(list(range(8)) + list(range(top - 7, top + 1)), np.uint8 if kind == "bytes" else np.uint32)
    lens = np.asarray(lens, np.int64)
    offs = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    data = alphabet[rng.integers(0, 16, int(lens.sum()))]
    return dict(name="past_cap", kind=kind, data=data, offs=offs, width=w, n_perm=PAST_K, vocab_size=V, where=where)


def band_rows_sig():
    """-> sig uint32[S, 2], S = 256·2048 + 300: the kernels with a thread per row (iota, heads) go round twice, and with two
    bands so does the one with a thread per key.  The values come from 12, so the buckets are large; eight rows, at the
    start, on either side of row 256·2048 and at the end, have values of their own and are the only rows of their buckets."""
    rng = np.random.default_rng(6100)
    S = TILE * SIG_CAP + 300
    values = rng.integers(0, 1 << 32, 12, dtype=np.uint64).astype(np.uint32)
    sig = values[rng.integers(0, 12, (S, 2))]
    alone = np.asarray([0, 1, 70_000, TILE * SIG_CAP - 1, TILE * SIG_CAP, TILE * SIG_CAP + 1, S - 2, S - 1])
    sig[alone] = (np.arange(1, 17, dtype=np.uint32) * np.uint32(0x01000193)).reshape(8, 2)
    return sig, alone


def verify_rows_sig():
    """-> sig uint32[S, 65], S = 4·16384 + 300: minhash_verify_kernel, a wave per row on a grid of 16384 blocks of four, goes
    round twice.  A row is one of 200 signatures with 0 .. 45 of its values (at random places) replaced, so rows of one
    origin agree with each other in 0 .. 65 places and share a band where none of its values was replaced."""
    rng = np.random.default_rng(6200)
    S, K = 4 * VERIFY_CAP + 300, 65
    origin = rng.integers(0, 1 << 32, (200, K), dtype=np.uint64).astype(np.uint32)
    sig = origin[rng.integers(0, 200, S)]
    n_replaced = rng.integers(0, 46, S)
    replaced = rng.random((S, K)).argsort(axis=1) < n_replaced[:, None]
    sig[replaced] = rng.integers(0, 1 << 32, int(replaced.sum()), dtype=np.uint64).astype(np.uint32)
    return sig


CHAIN_SIZES = (1, 2, 3, 64, 65, 1025, 65537)
CHAIN_K, CHAIN_B = 4, 2


def chain_case(S):
    """-> (sig, heads, first, n_clusters, min_agree): one chain of S rows.  heads[i][0] = i - 1 (row 0: itself), the other
    band holds i, all signatures are equal and min_agree = K: first0[i] = i - 1, every root is row 0, one cluster, after
    ceil(log2 S) rounds of pointer doubling."""
    sig = np.full((S, CHAIN_K), 7, np.uint32)
    me = np.arange(S, dtype=np.int64)
    heads = np.stack([np.maximum(me - 1, 0), me], axis=1)
    return sig, heads, np.zeros(S, np.int64), 1, CHAIN_K


def forest_case():
    """-> (sig, heads, first, n_clusters, min_agree): chains of 1, 2, 3, 5, 8, .. 1597 rows laid end to end, heads as in
    chain_case.  The rows of a chain share a signature that differs in one value from the next chain's, so a chain's
    first row does not take the row before it, and first is each chain's own first row."""
    sizes = [1, 2]
    while sizes[-1] < 1597:
        sizes.append(sizes[-1] + sizes[-2])
    chain = np.repeat(np.arange(len(sizes)), sizes)
    S = chain.size
    sig = np.full((S, CHAIN_K), 7, np.uint32)
    sig[:, 2] = chain
    me = np.arange(S, dtype=np.int64)
    heads = np.stack([np.maximum(me - 1, 0), me], axis=1)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return sig, heads, starts[chain].astype(np.int64), len(sizes), CHAIN_K


ELSEWHERE = ("i", "i + 1", "S", 1 << 40, -1, -(1 << 63))


def heads_from_elsewhere(heads):
    """-> (wild, tame): heads with a third of the entries overwritten by values that are no row before i (in turn i,
    i + 1, S, 2^40, -1 and INT64_MIN), and the same with those entries set to i"""
    rng = np.random.default_rng(6300)
    S, B = heads.shape
    me = np.broadcast_to(np.arange(S, dtype=np.int64)[:, None], (S, B))
    pick = rng.random((S, B)) < 1 / 3
    turn = np.arange(S * B).reshape(S, B) % len(ELSEWHERE)
    wild, tame = heads.copy(), heads.copy()
    tame[pick] = me[pick]
    for t, v in enumerate(ELSEWHERE):
        at = pick & (turn == t)
        wild[at] = {"i": me, "i + 1": me + 1, "S": np.full((S, B), S, np.int64)}[v][at] if isinstance(v, str) else v
    return wild, tame
