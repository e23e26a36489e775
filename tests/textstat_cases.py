"""The batches that tests/test_textstat_cpu.py hands the host twins and tests/test_textstat_gpu.py the kernels: seeded, so
both see the same ones.  A case is a corpus: text uint8[N] and offsets uint64[S + 1].

The kernels lay the BYTES of all rows end to end, a wave takes a chunk of 64, a block a tile of 256 and, past the grid's
cap, a run of consecutive tiles; a row's sums leave the wave by plain stores when the row lies inside the chunk and by
atomics otherwise; the length of a line that began before its end's chunk comes from the chunk's carry.  So the shapes
are the smallest at which that can go wrong, each named in NAMES below and described at its branch of `case`.
past_cap_case has more tiles than the grid has blocks."""
import numpy as np

CHUNK, TILE = 64, 256          # csrc/textstat.h: kTextstatChunk, kTextstatTile
CAP = 2048                     # csrc/textstat.hip: kTextstatMaxBlocks
LIMITS = (0, 5)
EDGES = {"edges_chunk": CHUNK, "edges_tile": TILE, "edges_two_tiles": 2 * TILE}
NAMES = ("short_rows", "nl_at_chunk_edges", "limit_lines", "edges_chunk", "edges_tile", "edges_two_tiles", "row_end_at_chunk_edge", "empty_rows",
         "long_line", "only_newlines", "chars_across_chunks", "stray_continuations", "byte_classes")
ALPHABET = list("abcXYZ 09.,;\t") + ["é", "€", "😀", "\n", "\n"]
ENCODED = [ch.encode("utf-8") for ch in ALPHABET]


def pack(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.frombuffer(b"".join(rows), np.uint8).copy(), offs


def _prose(rng, n):
    """n bytes of valid UTF-8 with a '\\n' about every ninth character"""
    out = b"".join(ENCODED[k] for k in rng.integers(0, len(ENCODED), n))   # n characters: n bytes or more
    cut = n
    while cut < len(out) and cut > 0 and (out[cut] & 0xC0) == 0x80:            # cut at a character's edge, fill with ASCII
        cut -= 1
    return out[:cut] + b"x" * (n - cut)


def _no_newline(buf: bytearray, a, z):
    """the bytes [a, z) of buf lose their '\\n's: one line goes through"""
    for p in range(max(a, 0), min(z, len(buf))):
        if buf[p] == 10:
            buf[p] = ord("_")


def case(name):
    """-> dict(name, text, offs, rows (bytes))"""
    rng = np.random.default_rng(9300 + 100 * NAMES.index(name))
    rows = []
    cum = lambda: sum(len(r) for r in rows)
    if name == "short_rows":      # every row of 0 .. 3 bytes over {a, '\n'}, a two-byte character, a lone continuation byte
        for n in range(4):
            for k in range(2 ** n):
                rows.append(bytes(10 if (k >> j) & 1 else ord("a") for j in range(n)))
        rows += ["é".encode(), b"\x80", b"", b"\n", b""]
    elif name == "nl_at_chunk_edges":  # '\n' on the last lane of a chunk and on the first lane of the next; on one of the two alone
        row = bytearray(b"x" * 330)
        for p in (63, 64, 127, 192, 255, 256):
            row[p] = 10
        rows += [bytes(row), b"y" * 53 + b"\n" + b"z" * 64 + b"\n" + b"w" * 10]   # the second: '\n's at bytes 383 and 448
    elif name == "limit_lines":   # lines of exactly limit and limit + 1, in bytes and in characters, ended by '\n' and by the row
        e = "é".encode()
        rows += [b"\n" + b"a\n" + b"aaaaa\n" + b"aaaaaa\n" + e * 5 + b"\n" + e * 6 + b"\n" + b"aaaaa", b"aaaaaa", e * 3 + b"\n" + e * 2 + b"a", b"a", b"\n"]
    elif name in EDGES:           # fillers, then a row that crosses one edge and ends at the next but one + d, lines astride both
        edge = EDGES[name]
        for d in (-3, -2, -1, 0, 1, 2, 3):
            rows += [b"", b"a\n", b"\n\nbc\n"]
            crossed = (cum() // edge + 2) * edge
            start = cum()
            row = bytearray(_prose(rng, crossed + edge + d - start))
            _no_newline(row, crossed - 5 - start, crossed + 5 - start)
            _no_newline(row, crossed + edge - 5 - start, len(row))
            if d == 2:
                row[-1] = 10                                            # this one ends with its terminator, just behind the edge
            rows.append(bytes(row))
        rows.append(b"end")
    elif name == "row_end_at_chunk_edge":  # a row that ends without '\n' exactly at a chunk's end; the next begins with a long line
        rows += [b"q\n" + b"r" * (2 * CHUNK - 2), b"s" * 150 + b"\n" + b"t" * 20, b"u" * 20 + b"\n", b"v" * (5 * CHUNK - 192), b"w" * 200]
    elif name == "empty_rows":    # runs of empty rows before, inside and behind the edges of a chunk and of a tile
        rows += [b"", b"", b"", _prose(rng, CHUNK), b"", b"", _prose(rng, 10), b"", _prose(rng, TILE - CHUNK - 10), b"", b"", b"",
                 _prose(rng, TILE + 7), b"", _prose(rng, CHUNK - 7), b"", b""]
    elif name == "long_line":     # one line of five tiles without a '\n', and the same with a '\n' as its last byte
        rows += [b"ab\ncd", b"L" * (5 * TILE), b"", b"\n", b"M" * (5 * TILE - 1) + b"\n", b"tail\n"]
    elif name == "only_newlines":
        rows += [b"\n" * 200, b"\n" * CHUNK, b"", b"\n" * (CHUNK - 8), b"a", b"\n" * 3]
    elif name == "chars_across_chunks":  # two-, three- and four-byte characters: the lead byte a chunk's last, the rest open the next
        row = b""
        for ch in ("é", "€", "😀"):
            row += b"k" * ((-len(row) - 1) % CHUNK) + ch.encode() + b"\n"
        rows += [row + b"end", "€".encode() * 50]
    elif name == "stray_continuations":  # a continuation byte as a row's first byte and after a '\n'
        rows += [b"\x80ab\n\x80\x80c\n\xbf", b"\xbf", b"a\n\x80", b"\x80" * 70, b"ok\n"]
    elif name == "byte_classes":  # all 256 byte values in one row, and each class's first and last member around them
        rows += [b"AZaz09 \t\r\x00\x08\x0e\x1f\x7f@[`{/:", b"\xc0\xff\xbf\x80", bytes(range(256)), bytes(range(255, -1, -1))]
    else:
        raise KeyError(name)
    text, offs = pack(rows)
    return dict(name=name, text=text, offs=offs, rows=rows)


# ---- past the cap of csrc/textstat.hip's grid ------------------------------------------------------------------------------

RUN = 2 * TILE                            # the bytes of a block's run of per_block = 2 tiles
PAST_N = CAP * TILE + 2 * TILE + 70       # 2050 tiles and 70 bytes: the last tile's third and fourth chunk are empty


def past_cap_case():
    """-> a case dict with `where`: PAST_N bytes, so that n_tiles = 2051 is over the grid's 2048 blocks: per_block = 2 and
    block b takes tiles 2b and 2b + 1 (a run of 512 bytes).  The rows, a few thousand, are prose of 100 to 300 bytes and
    rows of 0 to 3 bytes.  where["row"] is one row over bytes 150 .. 800 of a run, so over both tiles of the run and into
    the next block's; in it where["inside"] = (a, z), a line over bytes 200 .. 350 of the run (from the run's first tile
    into its second), and where["straddle"], a line over bytes 400 .. 700 (from one block's run into the next)."""
    rng = np.random.default_rng(9900)
    lens, where, cum = [], {}, 0

    def add(n):
        nonlocal cum
        lens.append(n)
        cum += n
        return len(lens) - 1

    def fill_to(target):
        while target - cum > 420:
            add(int(rng.integers(100, 300)))
        for n in (0, 1, 2, 3):
            add(n)
        assert target - cum >= 1
        add(target - cum)

    for n in (0, 0, 0):
        add(n)
    fill_to(300 * RUN + 17)
    base = (cum // RUN + 2) * RUN
    fill_to(base + 150)
    where["row"] = add(650)
    fill_to(PAST_N - 10)
    for n in (4, 3, 2, 1, 0, 0):
        add(n)
    assert cum == PAST_N
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    buf = bytearray(_prose(rng, PAST_N))
    for a, z, key in ((200, 350, "inside"), (400, 700, "straddle")):
        _no_newline(buf, base + a, base + z)
        buf[base + a - 1] = buf[base + z] = 10
        where[key] = (base + a, base + z)
    text = np.frombuffer(bytes(buf), np.uint8).copy()
    return dict(name="past_cap", text=text, offs=offs, where=where)
