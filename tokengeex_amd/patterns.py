"""Byte patterns over character classes, compiled to the automaton that pattern_hits runs on the device
(include/tgx_patterns.h: tgx_dfa; csrc/dfa.hip).

    pat = compile_pattern(r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\\.[a-zA-Z]{2,}")     # 7 states
    pat = compile_pattern([r"\\d{3}-\\d{2}-\\d{4}", r"\\d{5,}"])                    # pattern k tags its matches with bit k

Pure Python over bytes: a parser, Thompson's NFA, the subset construction (with search=True the start is re-entered at
every byte, which is the automaton of .*R: it marks where a match of R ENDS) and Moore's minimisation.  The device
serves automata of at most 16 states; a pattern that needs more raises ValueError with the count.

    pat = compile_pattern(r"\\(?\\d{3}\\)?[ .-]?\\d{3}[ .-]?\\d{4}", max_states=64)   # a phone shape: 17 states

With max_states=64 the automaton may have up to 64 states; one of more than 16 is run by the kernels of csrc/dfa64.hip (a
lane per state, then a lane per chunk: include/tgx_patterns64.h: tgx_dfa64).

    pat = compile_pattern(r"\\d{3}-\\d{2}-\\d{4}", cover=True)                     # 12 forward and 11 backward states

With cover=True the pattern also carries a backward automaton and a table over the pairs of states, which together say
which bytes lie INSIDE a match (include/tgx_redact.h: tgx_dfa_cover; csrc/cover.hip).

    pat = compile_pattern(r"std::\\w+", find=True)                                # what re.finditer finds: 8 states

With find=True the automaton is the anchored, leftmost-first one that find_matches and mine_idioms walk from every
start byte (include/tgx_find.h; csrc/find.hip).

Syntax: literal bytes; the escapes \\\\ \\. (a backslash before any ASCII punctuation is that byte) \\n \\t \\r \\f \\v \\d \\w
\\s \\xHH; `.`, any byte but '\\n'; [...] with ranges and a leading ^; ( ) and (?: ), |, * + ?, {m}, {m,}, {m,n}.  A str pattern is
its UTF-8 bytes, a non-ASCII byte inside [...] is refused, \\d \\w \\s are ASCII ([0-9], [A-Za-z0-9_], space and 0x09 ..
0x0D).  Anchors, backreferences, look-around, lazy and possessive quantifiers and Unicode classes are refused by name."""
from __future__ import annotations

import numpy as np

MAX_STATES = 16      # TGX_DFA_MAX_STATES
MAX_STATES64 = 64    # TGX_DFA64_MAX_STATES
MAX_PATTERNS = 8     # one tag bit each
MAX_SUBSETS = 4096   # the subset construction gives up beyond this many states
MAX_REPEAT = 256     # of one {m,n}

_ALL = (1 << 256) - 1
_DIGIT = sum(1 << b for b in range(0x30, 0x3A))
_WORD = _DIGIT | sum(1 << b for b in range(0x41, 0x5B)) | sum(1 << b for b in range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = (1 << 0x20) | sum(1 << b for b in range(9, 14))
_CLASSES = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE}
_CONTROLS = {ord("n"): 10, ord("t"): 9, ord("r"): 13, ord("f"): 12, ord("v"): 11}
_PUNCT = frozenset(b"!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ ")


def _fold(mask: int) -> int:
    """the other ASCII case of every letter of the set"""
    for lo in range(0x61, 0x7B):
        if mask >> lo & 1 or mask >> (lo - 32) & 1:
            mask |= (1 << lo) | (1 << (lo - 32))
    return mask


class _Parser:
    """pattern bytes -> a tree of ("set", mask), ("cat", [..]), ("alt", [..]), ("rep", node, m, n | None)"""

    def __init__(self, src: bytes, fold_case: bool):
        self.s, self.i, self.fold = src, 0, fold_case

    def fail(self, what: str):
        raise ValueError(f"pattern {self.s!r}: {what} at byte {self.i}")

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else None

    def set(self, mask: int):
        return ("set", _fold(mask) if self.fold else mask)

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail("an unmatched )")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == ord("*"):
                m, n = 0, None
            elif c == ord("+"):
                m, n = 1, None
            elif c == ord("?"):
                m, n = 0, 1
            elif c == ord("{"):
                m, n = self.bounds()
            else:
                return node
            self.i += 1
            if self.peek() == ord("?"):
                self.fail("a lazy quantifier (not supported)")
            if self.peek() == ord("+"):
                self.fail("a possessive quantifier (not supported)")
            node = ("rep", node, m, n)

    def bounds(self):
        """at '{': -> (m, n), leaving the index on the '}'"""
        close = self.s.find(b"}", self.i)
        body = self.s[self.i + 1:close] if close > 0 else b""
        lo, comma, hi = body.partition(b",")
        if not lo.isdigit() or (hi and not hi.isdigit()):
            self.fail("a malformed {m,n}")
        m = int(lo)
        n = m if not comma else (int(hi) if hi else None)
        if (n is not None and n < m) or max(m, n or 0) > MAX_REPEAT:
            self.fail(f"a {{m,n}} with n < m or a bound above {MAX_REPEAT}")
        self.i = close
        return m, n

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == ord("("):
            if self.s[self.i:self.i + 2] == b"?:":  # a group that captures nothing: every group here is one
                self.i += 2
            elif self.peek() == ord("?"):
                nxt = self.s[self.i + 1:self.i + 3]
                self.fail("look-around (not supported)" if nxt[:1] in (b"=", b"!") or nxt[:2] in (b"<=", b"<!") else
                          "a backreference (not supported)" if nxt[:2] == b"P=" else "a (?...) group (not supported)")
            node = self.alt()
            if self.peek() != ord(")"):
                self.fail("a missing )")
            self.i += 1
            return node
        if c == ord("["):
            return self.char_class()
        if c == ord("."):
            return ("set", _ALL & ~(1 << 10))
        if c in b"^$":
            self.i -= 1
            self.fail("an anchor (not supported)")
        if c in b"*+?{":
            self.i -= 1
            self.fail("a quantifier with nothing to repeat")
        if c == ord("\\"):
            return self.set(self.escape(False))
        return self.set(1 << c)

    def escape(self, in_class: bool) -> int:
        """after a backslash: -> the set it stands for"""
        c = self.peek()
        if c is None:
            self.fail("a trailing backslash")
        self.i += 1
        if c in _CLASSES:
            return _CLASSES[c]
        if c in _CONTROLS:
            return 1 << _CONTROLS[c]
        if c == ord("x"):
            hexes = self.s[self.i:self.i + 2]
            try:
                b = int(hexes, 16) if len(hexes) == 2 else -1
            except ValueError:
                b = -1
            if b < 0:
                self.fail("a malformed \\xHH")
            self.i += 2
            return 1 << b
        if c in _PUNCT:
            return 1 << c
        self.i -= 1
        if c in b"0123456789":
            self.fail("a backreference (not supported)")
        if c in b"bBAZz":
            self.fail("an anchor (not supported)")
        if c in b"pPNX":
            self.fail("a Unicode class (not supported)")
        self.fail(f"the escape \\{chr(c)} (not supported)")

    def class_item(self):
        """one member of a [...]: -> (set, the single byte it is or None)"""
        c = self.peek()
        if c is None:
            self.fail("an unterminated [")
        self.i += 1
        if c == ord("\\"):
            mask = self.escape(True)
            return mask, (mask.bit_length() - 1 if mask & (mask - 1) == 0 else None)
        if c >= 0x80:
            self.i -= 1
            self.fail("a non-ASCII byte inside [...] (a class is a set of bytes; write \\xHH for a byte)")
        return 1 << c, c

    def char_class(self):
        negate = self.peek() == ord("^")
        self.i += negate
        mask, first = 0, True
        while first or self.peek() != ord("]"):
            first = False
            part, lo = self.class_item()
            if self.peek() == ord("-") and self.s[self.i + 1:self.i + 2] not in (b"]", b""):
                self.i += 1
                _, hi = self.class_item()
                if lo is None or hi is None or hi < lo:
                    self.fail("a bad range in [...]")
                part = sum(1 << b for b in range(lo, hi + 1))
            mask |= part
        self.i += 1
        if self.fold:
            mask = _fold(mask)
        return ("set", _ALL & ~mask if negate else mask)


class _Nfa:
    """Thompson's construction: eps[s] the states reached for free, edge[s] = (mask, target) or None"""

    def __init__(self):
        self.eps, self.edge = [], []

    def state(self):
        self.eps.append([])
        self.edge.append(None)
        return len(self.eps) - 1

    def build(self, node, a: int) -> int:
        """the fragment of `node` from state a -> its end state"""
        kind = node[0]
        if kind == "set":
            z = self.state()  # (every fragment begins at a fresh state, so `a` has no edge yet)
            self.edge[a] = (node[1], z)
            return z
        if kind == "cat":
            for item in node[1]:
                nxt = self.state()
                self.eps[a].append(nxt)
                a = self.build(item, nxt)
            return a
        if kind == "alt":
            z = self.state()
            for arm in node[1]:
                s = self.state()
                self.eps[a].append(s)
                self.eps[self.build(arm, s)].append(z)
            return z
        _, sub, m, n = node
        for _ in range(m):
            s = self.state()
            self.eps[a].append(s)
            a = self.build(sub, s)
        if n is None:  # a star
            s, z = self.state(), self.state()
            self.eps[a] += [s, z]
            self.eps[self.build(sub, s)] += [s, z]
            return z
        z = self.state()
        for _ in range(n - m):  # optional copies, each skipping to the end; the copy goes first: a repeat is greedy
            s = self.state()
            self.eps[a] += [s, z]
            a = self.build(sub, s)
        self.eps[a].append(z)
        return z

    def ordered_closure(self, states, accept):
        """the states reached for free from `states`, in priority order (eps edges in their order, depth first, a state
        at its first visit), of which only those with an edge or in `accept` are kept -> a tuple that ends at its first
        accepting state: what has a lower priority than a match can no longer win"""
        seen, out = set(), []
        todo = list(reversed(states))
        while todo:
            s = todo.pop()
            if s in seen:
                continue
            seen.add(s)
            if s in accept:
                return tuple(out + [s])
            if self.edge[s]:
                out.append(s)
            todo += reversed(self.eps[s])
        return tuple(out)

    def closure(self, states):
        seen, todo = set(states), list(states)
        while todo:
            for t in self.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)


def _byte_classes(masks):
    """the bytes grouped by the sets they belong to: -> (class of each byte, a representative byte per class)"""
    sig = {}
    cls = np.zeros(256, np.int64)
    reps = []
    for b in range(256):
        key = tuple(m >> b & 1 for m in masks)
        if key not in sig:
            sig[key] = len(reps)
            reps.append(b)
        cls[b] = sig[key]
    return cls, reps


class BytePattern:
    """A compiled automaton: .n_states, .start, .next (uint8 [256, 16]: next[b][s]), .tag (uint8 [16]: bit k set in an
    accepting state of pattern k) as numpy, the fields of tgx_dfa, and .patterns, the sources as bytes.  One of more
    than 16 states (compile_pattern(..., max_states=64)) has the fields of tgx_dfa64: .next [256, 64] and .tag [64]."""

    def __init__(self, n_states, start, nxt, tag, patterns=()):
        self.n_states, self.start, self.patterns = int(n_states), int(start), tuple(patterns)
        self.next = np.ascontiguousarray(nxt, dtype=np.uint8)
        self.tag = np.ascontiguousarray(tag, dtype=np.uint8)
        width = MAX_STATES if self.n_states <= MAX_STATES else MAX_STATES64
        assert self.next.shape == (256, width) and self.tag.shape == (width,)

    def __repr__(self):
        return f"BytePattern({list(self.patterns)!r}, n_states={self.n_states})"

    def fullmatch(self, data: bytes) -> bool:
        """The plain walk from .start over all of data: does it end in a tagged state?  For an anchored automaton
        (search=False) that is "the pattern matches exactly data", what the device's allow filter asks of a window."""
        q = self.start
        for b in data:
            q = int(self.next[b][q])
        return bool(self.tag[q])


class BackPattern:
    """The backward half of a cover pattern: .n_states, .start, .next (uint8 [256, 16]) and an all-zero .tag, the fields of
    tgx_dfa_cover's bwd, which is run from a row's last byte to its first."""

    def __init__(self, n_states, start, nxt):
        self.n_states, self.start = int(n_states), int(start)
        self.next = np.ascontiguousarray(nxt, dtype=np.uint8)
        self.tag = np.zeros(MAX_STATES, np.uint8)


def _explore(start, reps, move):
    """the subsets reachable from `start` under move(subset, representative byte): -> (subsets, trans[i][class])"""
    index, subsets, trans = {start: 0}, [start], []
    while len(trans) < len(subsets):
        row = []
        for b in reps:
            moved = move(subsets[len(trans)], b)
            if moved not in index:
                if len(subsets) >= MAX_SUBSETS:
                    raise ValueError(f"more than {MAX_SUBSETS} states before minimisation: the limit after it is {MAX_STATES}")
                index[moved] = len(subsets)
                subsets.append(moved)
            row.append(index[moved])
        trans.append(row)
    return subsets, trans


def _moore(block, trans):
    """Moore's refinement of the initial blocks (any hashable per state) -> (the class of each state, numbered by first
    member, so the start is class 0; the number of classes)"""
    while True:
        keys = {}
        refined = [keys.setdefault((block[i], tuple(block[t] for t in trans[i])), len(keys)) for i in range(len(trans))]
        if len(keys) == len(set(block)):
            break
        block = refined
    names = {}
    for b in block:
        names.setdefault(b, len(names))
    return [names[b] for b in block], len(names)


def _table(state_of, trans, cls):
    nxt = np.zeros((256, MAX_STATES), np.uint8)
    for i, s in enumerate(state_of):
        nxt[:, s] = np.array([state_of[t] for t in trans[i]], np.uint8)[cls]
    return nxt


def _compile_cover(nfa, first, accept, owner, cls, reps, sources) -> BytePattern:
    """The two-sided automaton of include/tgx_redact.h.  Forward: the NFA states reached after AT LEAST one byte of an
    attempt begun at or before the byte (the attempts' first states stay out of the set: a match that begins at j + 1
    must not cover j).  Backward: the NFA states from which the bytes to the right, or none, reach an accept.  A byte is
    inside a match of pattern k iff the two sets share a state of pattern k's fragment."""
    edge = nfa.edge
    into = [[] for _ in nfa.eps]  # the eps edges reversed
    for s, targets in enumerate(nfa.eps):
        for t in targets:
            into[t].append(s)

    def back_closure(states):
        seen, todo = set(states), list(states)
        while todo:
            for t in into[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    ends = back_closure(accept)
    fsub, ftrans = _explore(frozenset(), reps, lambda cur, b: nfa.closure([edge[s][1] for s in cur | first if edge[s] and edge[s][0] >> b & 1]))
    bsub, btrans = _explore(ends, reps, lambda cur, b: back_closure([s for s, e in enumerate(edge) if e and e[0] >> b & 1 and e[1] in cur]) | ends)
    ftag = [sum({accept[s] for s in sub if s in accept}) for sub in fsub]
    pair = [[0] * len(bsub) for _ in fsub]
    for i, x in enumerate(fsub):
        for j, y in enumerate(bsub):
            for s in x & y:
                pair[i][j] |= owner[s]
    fstate, nf = _moore([(ftag[i], tuple(pair[i])) for i in range(len(fsub))], ftrans)
    bstate, nb = _moore([tuple(pair[i][j] for i in range(len(fsub))) for j in range(len(bsub))], btrans)
    for side, n in (("forward", nf), ("backward", nb)):
        if n > MAX_STATES:
            raise ValueError(f"the {side} automaton of the cover has {n} states after minimisation: the limit is {MAX_STATES}")
    tag, cover = np.zeros(MAX_STATES, np.uint8), np.zeros((MAX_STATES, MAX_STATES), np.uint8)
    for i, f in enumerate(fstate):
        tag[f] = ftag[i]
        for j, g in enumerate(bstate):
            cover[f][g] = pair[i][j]
    pat = BytePattern(nf, 0, _table(fstate, ftrans, cls), tag, sources)
    pat.back, pat.cover = BackPattern(nb, 0, _table(bstate, btrans, cls)), cover
    return pat


def _compile_find(nfa, root, accept, cls, reps, sources) -> BytePattern:
    """The automaton of find_matches (include/tgx_find.h): the subset construction over ORDERED lists of NFA states, so
    that from a start byte the last tagged state before the dead state is the leftmost-first match."""
    final = set(accept)

    def move(cur, b):
        return nfa.ordered_closure([nfa.edge[s][1] for s in cur if s not in final and nfa.edge[s][0] >> b & 1], final)

    subsets, trans = _explore(nfa.ordered_closure([root], final), reps, move)
    state_of, n = _moore([int(bool(sub) and sub[-1] in final) for sub in subsets], trans)
    if n > MAX_STATES64:
        raise ValueError(f"the automaton has {n} states after minimisation: the limit is {MAX_STATES64}")
    width = MAX_STATES if n <= MAX_STATES else MAX_STATES64
    nxt, tag = np.zeros((256, width), np.uint8), np.zeros(width, np.uint8)
    for i, s in enumerate(state_of):
        tag[s] = int(bool(subsets[i]) and subsets[i][-1] in final)
        nxt[:, s] = np.array([state_of[t] for t in trans[i]], np.uint8)[cls]
    pat = BytePattern(n, 0, nxt, tag, sources)
    pat.find = True
    return pat


def compile_pattern(patterns, fold_case: bool = False, search: bool | None = None, cover: bool = False, max_states: int = MAX_STATES,
                    find: bool = False) -> BytePattern:
    """-> a BytePattern of one pattern (bytes or str) or of a list of up to 8, pattern k tagging its matches with bit k.
    search=True: the automaton of .*R, whose tag at a byte says that a match ends there (what pattern_hits counts);
    search=False: the automaton of R itself from a row's first byte, with a dead state.  fold_case adds the other ASCII
    case to every literal and class.  ValueError: a syntax error, an unsupported construct (named), a pattern that
    matches the empty string, or more than 16 states after minimisation (the message carries the count).
    cover=True (pattern_cover, redact_patterns): the pattern also carries .back, a BackPattern run from a row's last byte
    to its first, and .cover, uint8 [16, 16]: cover[f][g] has bit k set iff a byte after which the forward automaton is
    in f, and before which the backward one is in g, lies inside a match of pattern k.  The forward automaton still
    tags match ends, but is a larger one than without cover; more than 16 states on either side is a ValueError that
    names the side.
    max_states=64 (pattern_hits, pattern_rows): up to 64 states after minimisation, and a ValueError with the count above
    that; an automaton of more than 16 has .next [256, 64] and .tag [64].  Any value but 16 and 64 is a ValueError, and so
    is 64 with cover=True: cover and redaction keep their 16 states.
    find=True (find_matches, mine_idioms): the anchored automaton of the patterns' alternation in list order, with a dead
    state and the tag 1, of up to 64 states whatever max_states says, built over ordered state lists so that the last
    tagged state before the dead state is the match a regex engine's leftmost-first search finds at that start
    (alternatives in source order, greedy repeats); .find is True.  With cover=True or an explicit search= it is a
    ValueError."""
    if find and (cover or search is not None):
        raise ValueError("find=True is an automaton of its own: it takes neither cover=True nor search=")
    search = True if search is None else search
    if max_states not in (MAX_STATES, MAX_STATES64):
        raise ValueError(f"max_states={max_states!r}: an automaton has at most {MAX_STATES} states, or {MAX_STATES64} with max_states={MAX_STATES64}")
    if cover and max_states != MAX_STATES:
        raise ValueError(f"cover=True keeps the limit of {MAX_STATES} states on either side")
    if isinstance(patterns, (str, bytes, bytearray)):
        patterns = [patterns]
    sources = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
    if not 1 <= len(sources) <= MAX_PATTERNS:
        raise ValueError(f"{len(sources)} patterns: 1 to {MAX_PATTERNS} go into one automaton")
    nfa = _Nfa()
    root = nfa.state()
    accept, owner = {}, [0]
    for k, src in enumerate(sources):
        s = nfa.state()
        nfa.eps[root].append(s)
        accept[nfa.build(_Parser(src, fold_case).parse(), s)] = 1 << k
        owner += [1 << k] * (len(nfa.eps) - len(owner))  # every state of the fragment belongs to pattern k
    first = nfa.closure([root])
    if any(s in accept for s in first):
        raise ValueError("a pattern matches the empty string")
    cls, reps = _byte_classes(sorted({e[0] for e in nfa.edge if e}))
    if find:
        return _compile_find(nfa, root, accept, cls, reps, sources)
    if cover:
        if not search:
            raise ValueError("cover=True needs search=True: a cover is of the matches anywhere in a row")
        return _compile_cover(nfa, first, accept, owner, cls, reps, sources)
    # the subset construction over the byte classes
    index, subsets, trans = {first: 0}, [first], []
    while len(trans) < len(subsets):
        cur, row = subsets[len(trans)], []
        for b in reps:
            moved = nfa.closure([nfa.edge[s][1] for s in cur if nfa.edge[s] and nfa.edge[s][0] >> b & 1])
            if search:
                moved |= first
            if moved not in index:
                if len(subsets) >= MAX_SUBSETS:
                    raise ValueError(f"more than {MAX_SUBSETS} states before minimisation: the limit after it is {max_states}")
                index[moved] = len(subsets)
                subsets.append(moved)
            row.append(index[moved])
        trans.append(row)
    tags = [0] * len(subsets)
    for i, sub in enumerate(subsets):
        for s in sub:
            tags[i] |= accept.get(s, 0)
    # Moore: split by tag, then by the blocks of the successors, until nothing splits
    block = tags
    while True:
        keys = {}
        refined = [keys.setdefault((block[i], tuple(block[t] for t in trans[i])), len(keys)) for i in range(len(subsets))]
        if len(keys) == len(set(block)):
            break
        block = refined
    names = {}
    for i in range(len(subsets)):  # blocks numbered by their first member: the start is state 0
        names.setdefault(block[i], len(names))
    n = len(names)
    if n > max_states:
        raise ValueError(f"the automaton has {n} states after minimisation: the limit is {max_states}")
    width = MAX_STATES if n <= MAX_STATES else MAX_STATES64
    nxt, tag = np.zeros((256, width), np.uint8), np.zeros(width, np.uint8)
    for i in range(len(subsets)):
        s = names[block[i]]
        tag[s] = tags[i]
        nxt[:, s] = np.array([names[block[t]] for t in trans[i]], np.uint8)[cls]
    return BytePattern(n, 0, nxt, tag, sources)


# ---- shapes: fixed-length sequences of byte classes (include/tgx_shapes.h; csrc/shape.hip) ----------------
SHAPE_MAX_LEN = 64        # TGX_SHAPE_MAX_LEN
SHAPES_MAX_BITS = 128     # TGX_SHAPES_MAX_BITS
SHAPES_MAX_PATTERNS = 8   # TGX_SHAPES_MAX_PATTERNS


class ShapePattern:
    """Compiled shapes: .n_patterns, .len (uint32 [8]), .cls (uint8 [128, 32]: position q of the patterns laid end to
    end, byte b at bit b & 7 of cls[q][b >> 3]), .not_before and .not_after (uint8 [8, 32]) as numpy, the fields of
    tgx_shapes, and .patterns, the sources as bytes."""

    def __init__(self, lens, cls, not_before, not_after, patterns=()):
        self.n_patterns, self.patterns = len(lens), tuple(patterns)
        self.len = np.zeros(SHAPES_MAX_PATTERNS, np.uint32)
        self.len[:len(lens)] = lens
        self.cls = np.ascontiguousarray(cls, dtype=np.uint8)
        self.not_before = np.ascontiguousarray(not_before, dtype=np.uint8)
        self.not_after = np.ascontiguousarray(not_after, dtype=np.uint8)
        assert self.cls.shape == (SHAPES_MAX_BITS, 32) and self.not_before.shape == self.not_after.shape == (SHAPES_MAX_PATTERNS, 32)

    def __repr__(self):
        return f"ShapePattern({list(self.patterns)!r}, len={self.len[:self.n_patterns].tolist()})"


_NO_SHAPE = "a shape is a fixed-length sequence of byte classes"


def _shape_atoms(src: bytes, node, top: bool = True):
    """a pattern's tree -> the sets of its positions, or ValueError naming the construct that is no shape"""
    kind = node[0]
    if kind == "set":
        return [node[1]]
    if kind == "alt":
        raise ValueError(f"pattern {src!r}: an alternation (|): {_NO_SHAPE}")
    if kind == "cat":
        atoms = [a for item in node[1] for a in _shape_atoms(src, item, False)]
        if not top and len(node[1]) != 1:
            raise ValueError(f"pattern {src!r}: a group around {len(node[1])} atoms: {_NO_SHAPE}")
        return atoms
    _, sub, m, n = node
    if m != n:
        what = {(0, None): "*", (1, None): "+", (0, 1): "?"}.get((m, n), f"{{{m},{'' if n is None else n}}}")
        raise ValueError(f"pattern {src!r}: the quantifier {what}: {_NO_SHAPE} (an atom may have {{m}} and nothing else)")
    atoms = _shape_atoms(src, sub, False)
    if len(atoms) != 1 or sub[0] == "rep":
        raise ValueError(f"pattern {src!r}: a {{m}} of more than one atom: {_NO_SHAPE}")
    return atoms * m


def _set_bytes(mask: int) -> np.ndarray:
    return np.frombuffer(mask.to_bytes(32, "little"), np.uint8)


def compile_shapes(patterns, fold_case: bool = False) -> ShapePattern:
    """-> a ShapePattern of one pattern or of a list of up to 8, pattern k marking its matches with bit k (shape_hits,
    shape_cover, redact_patterns(shapes=True)).  A pattern is bytes or str, or a tuple (pattern, not_before,
    not_after) whose guards are a [...] class or "": the byte in front of a match must not be in not_before, the byte
    behind it not in not_after (a row's ends pass every guard).  The pattern is a sequence of single-byte atoms, literals,
    escapes, `.` and [...], each with an optional {m}: `AKIA[0-9A-Z]{16}`, `ghp_[0-9a-zA-Z]{36}`, ("[0-9a-f]{32}",
    "[0-9a-f]", "[0-9a-f]").  ValueError: a syntax error, any other construct (named: |, * + ?, {m,n}, a group around more
    than one atom), a length of 0 or over 64, a total over 128 positions, more than 8 patterns (the message carries the
    number).  fold_case adds the other ASCII case to every literal and class, the guards' too."""
    if isinstance(patterns, (str, bytes, bytearray)) or (isinstance(patterns, tuple) and len(patterns) == 3 and not isinstance(patterns[0], tuple)):
        patterns = [patterns]
    patterns = list(patterns)
    if not 1 <= len(patterns) <= SHAPES_MAX_PATTERNS:
        raise ValueError(f"{len(patterns)} patterns: 1 to {SHAPES_MAX_PATTERNS} go into one set of shapes")

    def source(p):
        return p.encode("utf-8") if isinstance(p, str) else bytes(p)

    lens, sets, sources = [], [], []
    guards = np.zeros((2, SHAPES_MAX_PATTERNS, 32), np.uint8)
    for k, p in enumerate(patterns):
        src, before, after = (source(x) for x in (p if isinstance(p, tuple) else (p, b"", b"")))
        atoms = _shape_atoms(src, _Parser(src, fold_case).parse())
        if not 1 <= len(atoms) <= SHAPE_MAX_LEN:
            raise ValueError(f"pattern {src!r}: a length of {len(atoms)}: a shape has 1 to {SHAPE_MAX_LEN} positions" +
                             (" (it matches the empty string)" if not atoms else ""))
        if any(a == 0 for a in atoms):
            raise ValueError(f"pattern {src!r}: an empty class matches nothing")
        for side, g in enumerate((before, after)):
            if g:
                one = _shape_atoms(g, _Parser(g, fold_case).parse())
                if len(one) != 1:
                    raise ValueError(f"guard {g!r}: a guard is one class of bytes, [...], or \"\"")
                guards[side, k] = _set_bytes(one[0])
        lens.append(len(atoms))
        sets += atoms
        sources.append(src)
    if len(sets) > SHAPES_MAX_BITS:
        raise ValueError(f"{len(sets)} positions in all: one set of shapes has at most {SHAPES_MAX_BITS}")
    cls = np.zeros((SHAPES_MAX_BITS, 32), np.uint8)
    for q, mask in enumerate(sets):
        cls[q] = _set_bytes(mask)
    return ShapePattern(lens, cls, guards[0], guards[1], sources)
