"""Row lengths that drive a capped grid's loop over tiles to its edges: into a block's second tile, and to outputs that end
at the edges of a thread's slot and of a tile.

A grid is capped at `cap` blocks, each taking tiles of `tile` positions, so a block takes a second tile only when there are
more than cap * tile positions.  The kernels have two such loops.

The strided loop (csrc/tile_fill.h, and the kernels of csrc/front.hip and csrc/norm.hip): block b takes tiles b, b + cap,
b + 2 cap ..; state in LDS (the tile's owners, a block's partial sums) is rewritten per trip behind a barrier, and a trip
that `continue`s must do so for the whole block and ahead of its barriers.  lengths(cap, tile) sum to
n_out = cap * tile + tile + 1: tiles 0 .. cap + 1, the last one of a single output, so blocks 0 and 1 go round twice.  The
first three tiles and the last two are covered by rows of 0 and 1 elements in the pattern 1 0 0 1 1 0 (three outputs per
six rows, and a tile is no multiple of three, so over the tiles an owner search ends before, inside and behind a run of
empty rows); one row longer than a tile lies between them.

The consecutive run (dedup_hash_kernel, minhash_sig_kernel): block b takes the per_block = ceil(n_tiles / grid) tiles
b * per_block .. and finds a tile's owners by galloping from those of the tile before; what a block keeps between tiles (LDS
sums, running minima in registers) must be empty again when the next tile begins, the last working block has a shorter
run, and the blocks behind it none.  per_block is 2 from cap * tile + 1 positions on, and a test wants cap * tile + tile + 1
at least and an odd number of tiles, so that a short run exists; the rows that matter are those that cross from a run's
first tile into its second (the carried state) and from one block's run into the next block's (two blocks add to one
row).  Those batches have contents as well as lengths, so they are built where their subsystem's cases are:
dedup_cases.past_cap_case and minhash_cases.past_cap_case for the runs, front_cases.past_cap_corpus and
norm_cases.past_cap_corpus for the strided kernels that read text.  All of them mirror the caps and tiles as constants
beside the name of the constant they mirror, and their CPU tests compute the tile counts from those.

edge_sizes(group, tile) are the small outputs: none, one, a slot of `group` outputs less one, full and one over, a tile less
one, full and one over.  edge_lengths(n) are rows of the same pattern that sum to n."""
import numpy as np

PATTERN = (1, 0, 0, 1, 1, 0)


def _short_rows(total):
    """rows of the pattern that sum to total"""
    reps = total // 3 + 1
    rows = np.tile(np.array(PATTERN, np.uint64), reps)
    return rows[: int(np.searchsorted(np.cumsum(rows), total)) + 1]


def n_out(cap, tile):
    return cap * tile + tile + 1


def lengths(cap, tile):
    head, tail = _short_rows(3 * tile), _short_rows(2 * tile + 1)
    long_row = n_out(cap, tile) - 5 * tile - 1
    assert long_row > tile
    out = np.concatenate([head, np.array([0, long_row, 0], np.uint64), tail])
    assert int(out.sum()) == n_out(cap, tile)
    return out


def offsets(cap, tile):
    return _starts(lengths(cap, tile))


def _starts(lens):
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])


def edge_sizes(group, tile):
    return [0, 1, group - 1, group, group + 1, tile - 1, tile, tile + 1]


def edge_lengths(n):
    """rows of the pattern that sum to n, then two empty rows: the owner of the last output is found below a run of them"""
    out = np.concatenate([_short_rows(n) if n else np.zeros(1, np.uint64), np.zeros(2, np.uint64)])
    assert int(out.sum()) == n
    return out


def edge_offsets(n):
    return _starts(edge_lengths(n))


def edge_rows(n):
    """the first n rows of the pattern, for a fill in which an empty row owns one output too"""
    return np.tile(np.array(PATTERN, np.uint64), n // len(PATTERN) + 1)[:n]
