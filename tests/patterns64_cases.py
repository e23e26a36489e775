"""The one case table of the 64-state byte patterns (include/tgx_patterns64.h; csrc/dfa64.hip), shared by
tests/test_patterns64_cpu.py and tests/test_patterns64_gpu.py, with the header's definition restated as a per-row loop.
A chunk is 64 bytes and a segment 4 096; every automaton has a string that it matches, which the texts plant on the
edges of both."""
import functools

import numpy as np

import tokengeex_amd as tgx

PHONE_17 = r"\+\d{2} \d{3} \d{3} \d{4}"  # the shape that 16 states refuse
EMAIL = r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}"
# name -> (patterns, the states of the minimal search automaton, a string that the first pattern matches)
AUTOMATA = {
    "phone17": ([PHONE_17], 17, b"+12 345 678 9012"), "hex32": ([r"[0-9a-f]{32}"], 33, b"0123456789abcdef" * 2), "a{63}": (["a{63}"], 64, b"a" * 63),
    "email7": ([EMAIL], 7, b"a@b.cd"), "ab": (["ab"], 3, b"ab"), "two_tags": ([PHONE_17, r"\d{4}"], 21, b"+12 345 678 9012"),  # both end on one byte
}
N_EDGES = 4096 + 3 * 64 + 17                # a short last segment that ends in a short chunk
N_SEAMS = 2048 * 4096 + 2 * 4096 + 70       # a wave takes more than one segment, and the scan has more than one group
SEAMS = [64, 4096, 4 * 4096, 16 * 4096, 64 * 4096, 65 * 4096, 1024 * 4096, 2048 * 4096, 2049 * 4096, 2050 * 4096, N_SEAMS]


def _place(text, hit, ends):
    """`hit` written so that its last byte is at every position of `ends`"""
    for e in ends:
        text[e + 1 - len(hit):e + 1] = np.frombuffer(hit, np.uint8)
    return text


def _edges(hit):
    """matches that end on byte 63 of a chunk, on byte 0 of the next chunk, behind the segment's edge and on the last byte;
    rows that begin on bytes 0, 1 and 63 of a chunk, in chunks 0 and 63 of a segment"""
    text = _place(np.full(N_EDGES, ord(" "), np.uint8), hit, [63, 256, 4096 + len(hit) // 2, N_EDGES - 1]).tobytes()
    return [text[a:b] for a, b in zip([0, 1, 191, 4033], [1, 191, 4033, N_EDGES])]


def _seams(hit):
    """an empty row, rows of some 200 bytes around an empty and a long one, a match across every seam and on the last byte"""
    rng = np.random.default_rng(7)
    text = _place(np.frombuffer(b"x 1a\n+", np.uint8)[rng.integers(0, 6, N_SEAMS)], hit, [s + len(hit) // 2 - (s == N_SEAMS) * (len(hit) // 2 + 1) for s in SEAMS])
    cuts = np.unique(rng.integers(0, N_SEAMS, N_SEAMS // 200))
    cuts = cuts[(cuts <= 100_000) | (cuts > 170_000)]  # one row of 70 000 bytes or so
    cuts = np.sort(np.concatenate([cuts[np.all([(cuts <= s - len(hit)) | (cuts > s + len(hit)) for s in SEAMS], axis=0)], [0, 0, 5000, 5000, N_SEAMS]]))
    return text, cuts.astype(np.uint64)


# name -> the rows, given the automaton's string (empty rows first, in the middle, in a run and last; rows of one byte; a
# match cut by a row boundary: "a" then "b" under `ab`)
TEXTS = {
    "edges": _edges,
    "rows": lambda h: [b"", b"", h, b"", b"", b"", h[:1], h[1:], b"x", h[-1:], b"y" + h, b""],
    "no_rows": lambda h: [], "no_bytes": lambda h: [b"", b"", b""], "long_row": lambda h: [b"a" * 66_000],
    "all_bytes": lambda h: [bytes([0, 10, 255]) + bytes(range(256)) + bytes([0, 10, 255])],
}
CASES = [(a, t) for a in AUTOMATA for t in ("edges", "rows")] + [("email7", "no_rows"), ("phone17", "no_bytes"), ("a{63}", "long_row"), ("phone17", "all_bytes"),
                                                                ("email7", "all_bytes"), ("phone17", "seams")]
CASE_IDS = [f"{a}-{t}" for a, t in CASES]
SMALL = [c for c in CASES if c[1] in ("rows", "all_bytes")]  # rows the quadratic check of re can take


@functools.lru_cache(maxsize=None)
def pattern(name):
    pat = tgx.compile_pattern(AUTOMATA[name][0], max_states=64)
    assert pat.n_states == AUTOMATA[name][1], (name, pat.n_states)
    return pat


@functools.lru_cache(maxsize=None)
def text(case):
    flat, offs = _seams(AUTOMATA[case[0]][2]) if case[1] == "seams" else tgx.pack(TEXTS[case[1]](AUTOMATA[case[0]][2]))
    for a in (flat, offs):
        a.setflags(write=False)
    return flat, offs


def reference(pat, flat, offs):
    """the header's definition: per row q = start, then q = next[b][q] byte by byte"""
    nxt, tag, data = pat.next.tolist(), pat.tag.tolist(), flat.tolist()
    count, ends = np.zeros(len(offs) - 1, np.int64), bytearray(len(data))
    for i in range(len(offs) - 1):
        q = pat.start
        for p in range(int(offs[i]), int(offs[i + 1])):
            q = nxt[data[p]][q]
            ends[p] = tag[q]
        count[i] = int(offs[i + 1]) - int(offs[i]) - ends.count(0, int(offs[i]), int(offs[i + 1]))
    return count, np.frombuffer(bytes(ends), np.uint8)


@functools.lru_cache(maxsize=None)
def want(case):
    """a case's answers by the reference: computed once, never changed"""
    return reference(pattern(case[0]), *text(case))
