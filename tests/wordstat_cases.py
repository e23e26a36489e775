"""The batches that tests/test_wordstat_cpu.py hands the host twin and tests/test_wordstat_gpu.py the kernels: seeded, so
both see the same ones.  A case is a corpus: text uint8[N] and offsets uint64[S + 1].

The kernels lay the BYTES of all rows end to end, a wave takes a chunk of 64, a block a tile of 256 and, past the grid's
cap, a run of consecutive tiles.  A word's length and flags and a line's leading non-space bytes come from the chunk's
carry when they began before it; the nine bytes a lane looks back on come from the lanes below it or, for a chunk's first
lanes, from memory; a row's sums leave the wave by plain stores when the row lies inside the chunk and by atomics
otherwise.  So the shapes are the smallest at which that can go wrong, each named in NAMES below and described at its
branch of `case`.  past_cap_case has more tiles than the grid has blocks.  Every case runs under COMBOS."""
import itertools

import numpy as np

CHUNK, TILE = 64, 256          # csrc/textstat.h: kTextstatChunk, kTextstatTile
CAP = 2048                     # csrc/textstat_walk.h: kTextstatMaxBlocks
LIMITS = (0, 5)
UNITS = ("char", "byte")
TABLE = (b"a", b"the", b"`", b"absolute", b"of", b"I")   # entries of 1, 3 and 8 bytes; "I" only where nothing is folded
EDGES = {"edges_chunk": CHUNK, "edges_tile": TILE, "edges_two_tiles": 2 * TILE}
NAMES = ("short_rows", "byte_classes", "word_at_chunk_edges", "long_words", "limit_words", "edges_chunk", "edges_tile", "edges_two_tiles",
         "rows_without_space", "stop_words", "bullets", "ellipses")


def table_for(fold: bool, with_table: bool):
    """the stop table of a run: none, or TABLE (without its entry that holds A-Z where the text is folded)"""
    return () if not with_table else tuple(w for w in TABLE if not (fold and w.lower() != w))


# (word_limit, unit, fold, with_table)
COMBOS = tuple(itertools.product(LIMITS, UNITS, (True, False), (True, False)))

PIECES = [s.encode("utf-8") for s in ("a", "b", "Z", "7", " ", " ", " ", "\n", "\t", ".", "...", "#", "-", "*", "é", "€", "😀", "…", "•", "the", "The", "of", "I", "\"", "!",
                                      "absolute", "`", "@")]


def pack(rows):
    offs = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.frombuffer(b"".join(rows), np.uint8).copy(), offs


def _prose(rng, n):
    """n bytes of valid UTF-8: words, white space, dots, bullets, stop words"""
    out = b"".join(PIECES[k] for k in rng.integers(0, len(PIECES), n))   # n pieces: n bytes or more
    cut = n
    while cut < len(out) and cut > 0 and (out[cut] & 0xC0) == 0x80:          # cut at a character's edge, fill with ASCII
        cut -= 1
    return out[:cut] + b"x" * (n - cut)


def _one_word(buf: bytearray, a, z):
    """the white space of bytes [a, z) of buf becomes letters: one word goes through"""
    for p in range(max(a, 0), min(z, len(buf))):
        if buf[p] in b" \t\n\r\x0b\x0c":
            buf[p] = ord("w")


class _Rows:
    """rows built one after the other, with the absolute position of the next byte at hand"""

    def __init__(self):
        self.rows, self.cur, self.n = [], bytearray(), 0

    def put(self, piece: bytes):
        self.cur += piece
        self.n += len(piece)
        return self

    def to(self, pos, space_last=True):
        """filler up to absolute position pos: one word of 'z', and a space as its last byte if asked"""
        gap = pos - self.n
        assert gap >= 0, (pos, self.n)
        if gap:
            self.put(b"z" * (gap - 1) + (b" " if space_last else b"z"))
        return self

    def next_edge(self, edge=CHUNK, least=12):
        """the first multiple of edge that leaves at least `least` bytes of room"""
        return -(-(self.n + least) // edge) * edge

    def end(self):
        self.rows.append(bytes(self.cur))
        self.cur = bytearray()
        return self


def case(name):
    """-> dict(name, text, offs, rows (bytes))"""
    rng = np.random.default_rng(9500 + 100 * NAMES.index(name))
    r = _Rows()
    if name == "short_rows":      # every row of 0 .. 3 bytes over {a, ' ', '\n'}; runs of empty rows; rows of spaces only
        r.rows += [b"", b"", b""]
        for n in range(4):
            for k in range(3 ** n):
                r.rows.append(bytes(b"a \n"[(k // 3 ** j) % 3] for j in range(n)))
        r.rows += [b"", b"", b" " * 5, b" \t\n\r\x0b\x0c" * 20, b"", "é".encode(), b"\x80", b"-", b"#", b".", b"", b""]
    elif name == "byte_classes":  # all 256 byte values in one row, one word per value, and the bytes around the classes' ends
        r.rows += [bytes(range(256)), bytes(range(255, -1, -1)), b" ".join(bytes([b]) for b in range(256)), b"@ [ ` { A Z a z \x7f \x80 \xbf \xc0 \xff 0 9",
                   b"\x1c\x1d\x1e\x1f \x08\x0e \x85 \xa0 \xc2\xa0 \xe2\x80\x83"]   # separators that are no space here; NEL and NBSP as bytes
    elif name == "word_at_chunk_edges":  # a word end on a chunk's last lane, a word start on the next chunk's first lane: each alone, then both
        e = r.next_edge()
        r.to(e - 4).put(b"end1").put(b" ").put(b"xy ")                 # an end on lane 63, a space on lane 0
        e = r.next_edge()
        r.to(e).put(b"start1 b ")                                     # a space on lane 63, a start on lane 0
        e = r.next_edge()
        r.to(e - 4).put(b"end2").end()                                # an end on lane 63 that is the row's last byte ...
        r.put(b"start2 tail").end()                                   # ... and a start on lane 0 that is the next row's first
        e = r.next_edge()
        r.to(e - 1, space_last=False).put(b"ab cd").end()              # one word astride the edge, for contrast
    elif name == "long_words":    # words of five tiles: the only letter, then the only byte >= 0x80, in the word's first chunk
        r.put(b"12 ").put(b"3" * 10 + b"a" + b"4" * (5 * TILE - 11)).put(b" 56\n").end()
        r.put(b"7 ").put(b"8" * 5 + b"\x80" + b"9" * (5 * TILE - 6)).end()
        r.put(b"0" * (5 * TILE)).put(b" a").end()                      # neither: digits only
    elif name == "limit_words":   # words of exactly each limit and one more, in bytes and in characters; a lead byte on a chunk's last lane
        e2 = "é".encode()
        r.put(b"a aaaaa aaaaaa " + e2 * 5 + b" " + e2 * 6 + b" " + e2 * 2 + b"a " + e2 * 3 + b"\n").end()
        for ch in ("é", "€", "😀"):
            e = r.next_edge()
            r.to(e - 5).put(b"kkkk").put(ch.encode() * 2).put(b" ")    # five characters and one more, the lead byte on lane 63
            e = r.next_edge()
            r.to(e - 4).put(b"kkk").put(ch.encode()).put(b"kk ")       # six characters
        r.end()
    elif name in EDGES:           # fillers, then a row that crosses one edge and ends at the next but one + d, words astride both
        edge = EDGES[name]
        for d in (-3, -2, -1, 0, 1, 2, 3):
            r.rows += [b"", b"a b\n", b" \n- c\n"]
            r.n = sum(len(x) for x in r.rows)
            crossed = (r.n // edge + 2) * edge
            start = r.n
            row = bytearray(_prose(rng, crossed + edge + d - start))
            _one_word(row, crossed - 5 - start, crossed + 5 - start)
            _one_word(row, crossed + edge - 5 - start, len(row))
            r.rows.append(bytes(row))
        r.rows.append(b"end")
    elif name == "rows_without_space":  # two rows with no space between them: the word is cut at the row's end; also at a chunk's edge
        r.put(b"abc").end().put(b"def ghi").end().put(b"the").end().put(b"me of").end().put(b"ba").end().put(b"the").end()
        e = r.next_edge()
        r.to(e - 3).put(b"abs").end().put(b"olute x").end()            # "absolute" cut in two by a row's end on a chunk's edge
        r.put(b"..").end().put(b". x").end().put(b"\xe2\x80").end().put(b"\xa6 \xe2").end().put(b"\x80\xa2").end()   # no ellipsis, no bullet across rows
    elif name == "stop_words":
        r.put(b"the bathe theme the. of off a aa ` `` I II\n").end()   # an entry as a word's suffix and as a word's prefix
        r.put(b"absolute xabsolute absolute absolutes\n").end()        # the ninth byte back: in front of the row, a non-space, a space
        e = r.next_edge()
        r.to(e).put(b"absolute ")                                     # ... a space in the chunk before
        e = r.next_edge()
        r.to(e, space_last=False).put(b"absolute ")                   # ... a non-space in the chunk before
        e = r.next_edge()
        r.to(e - 1).put(b"the ")                                      # a match whose bytes straddle a chunk: 1 | 2
        e = r.next_edge()
        r.to(e - 2).put(b"the ")                                      # 2 | 1
        e = r.next_edge()
        r.to(e - 5).put(b"absolute ")                                 # 5 | 3
        e = r.next_edge()
        r.to(e - 1).put(b" a ").end()                                 # a one-byte entry on lane 0 with its space on lane 63
        r.put(b"The THE tHe OF Of A I i ABSOLUTE Absolute\n").end()    # matched only where the text is folded
        r.put(b"@ ` @@ [ { a@ \n").end()                               # '@' is not folded into a backtick
        r.put(b"of " + b"x " * 100 + b"of the " + b"y " * 100 + b"of").end()   # the same stop word in several chunks of one row: one bit, three counted
        r.put(b"nothing here to see").end()
    elif name == "bullets":
        r.put(b"- a\n -b\n" + b" " * 70 + b"* c\n").put(b"a - b\n--\n-\n*\n \t * x\n").end()   # after 0, 1 and 70 spaces; "a -" is none, "--" is one
        e = r.next_edge()
        r.to(e - 1).put(b"\n").put(b" " * CHUNK).put(b"- d\n")         # the indentation fills a whole chunk, the bullet is first in the next
        b = "•".encode()
        e = r.next_edge()
        r.to(e - 2).put(b"\n").put(b[:1]).put(b[1:]).put(b" e\n")      # U+2022 cut 1 | 2 by a chunk's edge
        e = r.next_edge()
        r.to(e - 3).put(b"\n").put(b[:2]).put(b[2:]).put(b" f\n")      # 2 | 1
        r.put(b" " + b + b"\n" + b + b + b"\nx" + b + b"\n" + b[:2] + b"\n" + b"\xe2 \x80\xa2\n" + b"  " + b).end()
        r.put(b"no newline at the end").end().put(b"- a bullet as a row's first byte after a row without its terminator\n").end()
        r.put(b"x").end().put(b"*").end().put(b"\n\n-").end()
    elif name == "ellipses":
        for dots in (2, 3, 4, 6):                                      # runs of dots astride a chunk's edge, at every cut
            for left in range(1, dots):
                e = r.next_edge()
                r.to(e - left).put(b"." * dots).put(b" ")
        u = "…".encode()
        for left in (1, 2):
            e = r.next_edge()
            r.to(e - left).put(u).put(b" ")                            # U+2026 astride one
        e = r.next_edge()
        r.to(e - 3).put(b"...").put(b"\n")                             # "...\n" with the '\n' on the next chunk's first lane
        e = r.next_edge()
        r.to(e - 3).put(u).put(b"\n")
        r.put(b"... \n" + b"...\n\n" + b"....\n" + b"..\n" + b".\n...\n" + u + b"\n" + u + b" \n" + u + u + b"...\n").put(b"a... b.... c.. d").end()
        r.put(b"ends with three dots...").end().put(b"...").end().put(u).end().put(b"..").end().put(b"says \"hi\"\nwhy?\nyes!\nno.\nmaybe\n \nx\"").end()
    else:
        raise KeyError(name)
    if r.cur:
        r.end()
    text, offs = pack(r.rows)
    return dict(name=name, text=text, offs=offs, rows=r.rows)


# ---- past the cap of the kernels' grid -------------------------------------------------------------------------------------

RUN = 2 * TILE                            # the bytes of a block's run of per_block = 2 tiles
PAST_N = CAP * TILE + 2 * TILE + 70       # 2050 tiles and 70 bytes: the last tile's third and fourth chunk are empty


def past_cap_case():
    """-> a case dict with `where`: PAST_N bytes, so that n_tiles = 2051 is over the grid's 2048 blocks: per_block = 2 and
    block b takes tiles 2b and 2b + 1 (a run of 512 bytes).  The rows, a few thousand, are prose of 100 to 300 bytes and
    rows of 0 to 3 bytes.  where["word_row"] and where["indent_row"] are rows over bytes 150 .. 800 of a run each, so over
    both tiles of the run and into the next block's.  In the first, where["word_inside"] = (a, z) is a word over bytes
    200 .. 350 of the run (from the run's first tile into its second) and where["word_straddle"] one over 400 .. 700 (from
    one block's run into the next); in the second, where["indent_inside"] and where["indent_straddle"] are the same
    stretches as spaces after a '\\n', each with a bullet as the byte behind it."""
    rng = np.random.default_rng(9950)
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
    bases = {}
    for key, at in (("word", 300), ("indent", 600)):
        fill_to(at * RUN + 17)
        bases[key] = (cum // RUN + 2) * RUN
        fill_to(bases[key] + 150)
        where[key + "_row"] = add(650)
    fill_to(PAST_N - 10)
    for n in (4, 3, 2, 1, 0, 0):
        add(n)
    assert cum == PAST_N
    offs = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    buf = bytearray(_prose(rng, PAST_N))
    for a, z, key in ((200, 350, "inside"), (400, 700, "straddle")):
        base = bases["word"]
        _one_word(buf, base + a, base + z + 1)
        buf[base + a] = ord("Q")
        buf[base + a - 1] = buf[base + z + 1] = ord(" ")
        where["word_" + key] = (base + a, base + z)
        base = bases["indent"]
        buf[base + a - 1] = 10
        buf[base + a:base + z + 1] = b" " * (z + 1 - a)
        buf[base + z + 1:base + z + 3] = b"- "
        where["indent_" + key] = (base + a, base + z)
    text = np.frombuffer(bytes(buf), np.uint8).copy()
    return dict(name="past_cap", text=text, offs=offs, where=where)
