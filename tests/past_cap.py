"""Row lengths that drive a tiled fill (csrc/tile_fill.h) to the edges of its loop: into the second trip of the strided
loop, and to outputs that end at the edges of a thread's slot and of a tile.

A fill's grid is capped at `cap` blocks, each taking tiles of `tile` outputs, so a block takes a second tile only when there
are more than cap * tile outputs.  lengths(cap, tile) sum to n_out = cap * tile + tile + 1: tiles 0 .. cap + 1, the last one
of a single output, so blocks 0 and 1 go round twice.  The first three tiles and the last two are covered by rows of 0 and
1 elements in the pattern 1 0 0 1 1 0 (three outputs per six rows, and a tile is no multiple of three, so over the tiles
an owner search ends before, inside and behind a run of empty rows); one row longer than a tile lies between them.

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
