"""A second registry of device calls, of the shape of tests/dirty_runs.py, for the functions that the side headers declare
(include/tgx_words.h, tgx_word_ids.h, tgx_phrases.h, tgx_patterns.h, tgx_patterns64.h, tgx_redact.h, tgx_shapes.h,
tgx_hashed.h, tgx_find.h, tgx_allow.h, tgx_dupspans.h) and include/tgx.h does not.  dirty_runs.ENTRIES is held to
include/tgx.h alone (tests/test_dirty_runs_cpu.py), so these calls cannot be registered there; tests/test_side_runs_cpu.py
holds this registry to the side headers in the same way, tests/test_pool_fill_side_gpu.py runs every entry on filled
memory and tests/test_pass_sequences_side_gpu.py the same calls in mixed order on handles that stay alive.

An entry is a dirty_runs.Entry (covers, run(ctx), check(out); env empty, deterministic always: every output is integer
work) with one part more:
    twin()         the same output dictionary through the host twins, without a device: tests/test_side_runs_cpu.py
                   passes it to check, and then changes one element of every output and wants check to fail.
The rules are dirty_runs.py's: every handle is made inside run; caller outputs are torch tensors over a sentinel (-7 for
int64, 7 for uint8); an output that is not asked for must still hold it; check compares with the reference the subsystem
already has and asserts that the reference holds something (an all-zero output never passes).  Inputs are the smallest
cases of each subsystem's case module at which its kernels cross their seams; a past-the-cap case only where the kernel
carries state between a block's tiles or between scan groups and the reference is a matter of a second or two."""
from __future__ import annotations

import functools

import numpy as np

import tokengeex_amd as tgx
from tokengeex_amd import _lib

from dirty_runs import Ctx, Entry, _eq, _np  # noqa: F401  (Ctx: for the tests that run the entries)

ENTRIES: dict = {}

_TWIN = "host twin: pure host code"
_TIMES = "*_last_times: reads the thread's recorded stage times"
_HOST = "pure host code"
_GETTER = "getter of a handle's or the library's host-side state"
_FREE = "frees a handle (buffers go back to the pool, nothing is queued)"
EXCLUDED = {
    "tgx_word_stats_host": _TWIN, "tgx_wordstat_last_times": _TIMES,
    "tgx_word_key": _HOST, "tgx_words_host": _TWIN, "tgx_words_last_times": _TIMES,
    "tgx_phraseset_info": _GETTER, "tgx_phraseset_free": _FREE, "tgx_phrase_hits_host": _TWIN, "tgx_phrase_last_times": _TIMES,
    "tgx_dfa_hits_host": _TWIN, "tgx_dfa_last_times": _TIMES,
    "tgx_dfa64_hits_host": _TWIN, "tgx_dfa64_last_times": _TIMES,
    "tgx_dfa_cover_host": _TWIN, "tgx_redact_host": _TWIN, "tgx_redact_last_times": _TIMES,
    "tgx_shape_hits_host": _TWIN, "tgx_shape_cover_host": _TWIN, "tgx_shapes_last_times": _TIMES,
    "tgx_hashed_bucket": _HOST, "tgx_hashed_info": _GETTER, "tgx_hashed_counts_host": _TWIN, "tgx_hashed_scores_host": _TWIN,
    "tgx_hashed_last_times": _TIMES,
    "tgx_find_host": _TWIN, "tgx_mine_host": _TWIN, "tgx_find_last_times": _TIMES,
    "tgx_allow_masks_host": _TWIN, "tgx_allow_last_times": _TIMES,
    "tgx_dup_spans_host": _TWIN, "tgx_dupspan_last_times": _TIMES,
}

ROW, BYTE = -7, 7   # the sentinels of an int64 and of a uint8 output


def _add(name, covers, run, check, twin):
    assert name not in ENTRIES, name
    e = Entry(name, covers, run, check, {}, True)
    e.twin = twin
    ENTRIES[name] = e


def _held(got, sentinel, what):
    assert got.size and (got == sentinel).all(), (what, "an output that was not asked for was written")


# ======================================================================================================================
# calls of one shape: (corpus, a struct) -> a number per row (int64[S]) and a byte per byte (uint8[N]), either optional
# ======================================================================================================================
def _pair_entry(name, covers, method, host, cases, keys, both):
    """cases() -> [(label, struct, (flat, offs), want() -> (per row, per byte))]; both: ask for the bytes too"""

    def run(ctx):
        out = {}
        for label, pat, (flat, offs), _ in cases():
            corpus = tgx.NativeCorpus(flat, offs)
            row, byte = ctx.full((offs.size - 1,), "int64", ROW), ctx.full((flat.size,), "uint8", BYTE)
            getattr(corpus, method)(pat, row.data_ptr(), byte.data_ptr() if both else 0, stream=ctx.stream)
            out[f"{label}/{keys[0]}"], out[f"{label}/{keys[1]}"] = _np(row), _np(byte)
            corpus.free()
        return out

    def twin():
        out = {}
        for label, pat, (flat, offs), _ in cases():
            row, byte = host(flat, offs, pat)
            out[f"{label}/{keys[0]}"], out[f"{label}/{keys[1]}"] = row, byte if both else np.full(flat.size, BYTE, np.uint8)
        return out

    def check(out):
        for label, _, _, want in cases():
            w_row, w_byte = want()
            assert w_row.sum() > 0 and w_byte.any(), (label, "the reference holds nothing")
            _eq(out[f"{label}/{keys[0]}"], w_row, (label, keys[0]))
            if both:
                _eq(out[f"{label}/{keys[1]}"], w_byte, (label, keys[1]))
            else:
                _held(out[f"{label}/{keys[1]}"], BYTE, (label, keys[1]))

    _add(name, covers, run, check, twin)


# ---- byte patterns of up to 16 states (csrc/dfa.hip): a tile is 256 bytes; past 2048 tiles a block carries the state over two --
def _dfa_cases():
    import test_patterns_cpu as pc
    picked = (("ab", "edges"), ("ab", "empties"), ("ab|b", "both_tags"), ("email", "mixed"), ("a{15}", "long_row"), ("email", "two_tiles"))
    return [(f"{p}-{t}", pc.pattern(p), pc.text(t), functools.partial(pc.want, (p, t))) for p, t in picked]


for _both in (True, False):
    _pair_entry("dfa_hits" + ("" if _both else "_count_alone"), ("tgx_corpus_dfa_hits_device",), "dfa_hits", _lib.dfa_hits_host, _dfa_cases,
                ("count", "ends"), _both)


# ---- byte patterns of up to 64 states (csrc/dfa64.hip): chunks of 64 bytes, segments of 64 chunks, a wave's run of four
# segments at least, scan groups of 64 segments --------------------------------------------------------------------------
N_TWO_GROUPS = 65 * 4096 + 3 * 64 + 17   # the smallest text of two scan groups: 64 segments, then a short one that ends in a short chunk
TWO_GROUP_SEAMS = (64, 4096, 4 * 4096, 16 * 4096, 63 * 4096, 64 * 4096, 65 * 4096)


@functools.lru_cache(maxsize=None)
def two_groups(automaton="phone17"):
    """patterns64_cases' seams in small: a match across a chunk's, a segment's, a wave's run's, a block's and the scan
    group's edge (64 segments) and on the last byte; an empty row first, rows of some 300 bytes, one of 70 000 or so that
    crosses the block's edge, and a row that begins on the group's first byte -> (flat, offs)"""
    import patterns64_cases as p64
    hit = p64.AUTOMATA[automaton][2]
    rng = np.random.default_rng(11)
    N = N_TWO_GROUPS
    ends = [s + len(hit) // 2 for s in TWO_GROUP_SEAMS] + [N - 1]
    text = p64._place(np.frombuffer(b"x 1a\n+", np.uint8)[rng.integers(0, 6, N)], hit, ends)
    cuts = np.unique(rng.integers(0, N, N // 300))
    cuts = cuts[(cuts <= 30_000) | (cuts > 100_000)]
    cuts = cuts[np.all([(cuts <= e - len(hit)) | (cuts > e) for e in ends], axis=0)]
    offs = np.sort(np.concatenate([cuts, [0, 0, 64 * 4096 + len(hit), N]])).astype(np.uint64)
    assert (np.diff(offs.astype(np.int64)) >= 0).all() and int(np.diff(offs.astype(np.int64)).max()) > 65_536
    for a in (text, offs):
        a.setflags(write=False)
    return text, offs


@functools.lru_cache(maxsize=None)
def two_groups_want(automaton="phone17"):
    import patterns64_cases as p64
    return p64.reference(p64.pattern(automaton), *two_groups(automaton))


def _dfa64_cases():
    import patterns64_cases as p64
    picked = (("phone17", "edges"), ("hex32", "edges"), ("a{63}", "edges"), ("two_tags", "rows"), ("email7", "rows"), ("a{63}", "long_row"))
    return [(f"{a}-{t}", p64.pattern(a), p64.text((a, t)), functools.partial(p64.want, (a, t))) for a, t in picked] + \
        [("phone17-two_groups", p64.pattern("phone17"), two_groups(), two_groups_want)]


for _both in (True, False):
    _pair_entry("dfa64_hits" + ("" if _both else "_count_alone"), ("tgx_corpus_dfa64_hits_device",), "dfa64_hits", _lib.dfa64_hits_host, _dfa64_cases,
                ("count", "ends"), _both)


# ---- the cover by a two-sided DFA (csrc/cover.hip): dfa.hip's tiles in both directions, the carries mirrored ----------------------
def _cover_cases():
    import test_cover_cpu as cc
    picked = (("ab", "edges"), ("ab", "row_ends"), ("ab+c|c", "xbbc"), ("ssn+digits", "overlap"), ("ab", "empties"), ("email", "mixed"),
              ("a+b", "long_row"), ("email", "two_tiles"))
    return [(f"{p}-{t}", cc.pattern(p), cc.text(t), functools.partial(cc.want, (p, t))) for p, t in picked]


for _both in (True, False):
    _pair_entry("dfa_cover" + ("" if _both else "_covered_alone"), ("tgx_corpus_dfa_cover_device",), "dfa_cover", _lib.dfa_cover_host, _cover_cases,
                ("covered", "mask"), _both)


# ---- shapes (csrc/shape.hip): chunks with a halo, tiles of 256 bytes; past the cap a block takes two tiles ----------------------
def _shape_cases(cover):
    import shape_cases as sc
    picked = (("l64", "edges"), ("l64", "edges_one_row"), ("l40x2", "edges"), ("three", "edges"), ("guarded", "guards"), ("adjacent", "empties"),
              ("eight", "mixed"), ("keys", "two_tiles"))
    k = 2 if cover else 0
    return [(f"{s}-{t}", sc.shapes(s), sc.text(t), functools.partial(lambda c, k: sc.want(c)[k:k + 2], (s, t), k)) for s, t in picked]


for _both in (True, False):
    _pair_entry("shape_hits" + ("" if _both else "_count_alone"), ("tgx_corpus_shape_hits_device",), "shape_hits", _lib.shape_hits_host,
                functools.partial(_shape_cases, False), ("count", "ends"), _both)
    _pair_entry("shape_cover" + ("" if _both else "_covered_alone"), ("tgx_corpus_shape_cover_device",), "shape_cover", _lib.shape_cover_host,
                functools.partial(_shape_cases, True), ("covered", "mask"), _both)


# ---- redaction (csrc/redact.hip): run heads at chunk and tile edges, lengths summed into the new offsets ---------------------------
REDACT_CASES = ("small", "edges", "all_covered")


def _run_redact(ctx):
    import test_cover_cpu as cc
    out = {}
    for name in REDACT_CASES:
        flat, offs, mask, repl, _, _ = cc.redact_case(name)
        corpus = tgx.NativeCorpus(flat, offs)
        d_mask = ctx.dev(mask)
        new = corpus.redact(d_mask.data_ptr(), repl, stream=ctx.stream)
        out[f"{name}/bytes"], out[f"{name}/offs"] = new.bytes(), new.offsets()
        new.free()
        corpus.free()
    return out


def _twin_redact():
    import test_cover_cpu as cc
    out = {}
    for name in REDACT_CASES:
        flat, offs, mask, repl, _, _ = cc.redact_case(name)
        out[f"{name}/bytes"], out[f"{name}/offs"] = _lib.redact_host(flat, offs, mask, repl)
    return out


def _check_redact(out):
    import test_cover_cpu as cc
    for name in REDACT_CASES:
        _, _, mask, _, want_text, want_offs = cc.redact_case(name)
        assert mask.any() and want_text.size, (name, "the reference holds nothing")
        _eq(out[f"{name}/offs"], want_offs, (name, "offsets"))
        _eq(out[f"{name}/bytes"], want_text, (name, "bytes"))


_add("redact", ("tgx_corpus_redact",), _run_redact, _check_redact, _twin_redact)


# ---- leftmost-first matches and idiom mining (csrc/find.hip over dfa64.hip's scan): find_cases' mixed batch of 280 000 bytes
# is 69 segments, two scan groups; its last row ends mid-chunk ---------------------------------------------------------------------
FIND_PATTERNS = (r"\s+", r"std::\w+", r"a|ab|abc+")   # matches cut at max_len; idioms; leftmost-first is not leftmost-longest
MINE_TOP = 5


def _run_find(ctx, outs):
    import find_cases as fc
    out = {}
    corpus = tgx.NativeCorpus(fc.FLAT, fc.OFFS)
    S, N = fc.OFFS.size - 1, fc.FLAT.size
    for src in FIND_PATTERNS:
        bufs = [ctx.full((S,), "int64", ROW), ctx.full((N,), "uint8", BYTE), ctx.full((S,), "int64", ROW)]
        corpus.find(fc.pattern(src), *(b.data_ptr() if outs >> k & 1 else 0 for k, b in enumerate(bufs)), stream=ctx.stream)
        for key, b in zip(("count", "lens", "truncated"), bufs):
            out[f"{src}/{key}"] = _np(b)
    corpus.free()
    return out


def _twin_find(outs):
    import find_cases as fc
    out = {}
    for src in FIND_PATTERNS:
        got = _lib.find_host(fc.FLAT, fc.OFFS, fc.pattern(src))
        for k, (key, sentinel) in enumerate((("count", ROW), ("lens", BYTE), ("truncated", ROW))):
            out[f"{src}/{key}"] = got[k] if outs >> k & 1 else np.full_like(got[k], sentinel)
    return out


def _check_find(out, outs):
    import find_cases as fc
    for src in FIND_PATTERNS:
        want = fc.want(src)
        assert want[0].sum() > 0 and want[1].any(), (src, "the reference holds nothing")
        for k, (key, sentinel) in enumerate((("count", ROW), ("lens", BYTE), ("truncated", ROW))):
            if outs >> k & 1:
                _eq(out[f"{src}/{key}"], want[k], (src, key))
            else:
                _held(out[f"{src}/{key}"], sentinel, (src, key))
    assert fc.want(r"\s+")[2].sum() > 0, "no walk ran into max_len"


for _name, _outs in (("find", 7), ("find_count_alone", 1)):   # (count alone: the call allocates its own walk buffer)
    _add(_name, ("tgx_corpus_find_device",), functools.partial(_run_find, outs=_outs), functools.partial(_check_find, outs=_outs),
         functools.partial(_twin_find, _outs))


def _mine_out(res):
    pos, length, count, n_distinct, n_matches = res
    return {"pos": pos.copy(), "len": length.copy(), "count": count.copy(), "totals": np.array([n_distinct, n_matches], np.uint64)}


def _run_mine(ctx):
    import find_cases as fc
    out = {}
    corpus = tgx.NativeCorpus(fc.FLAT, fc.OFFS)
    for src in FIND_PATTERNS:
        out.update({f"{src}/{k}": v for k, v in _mine_out(corpus.mine(fc.pattern(src), MINE_TOP, stream=ctx.stream)).items()})
    corpus.free()
    return out


def _twin_mine():
    import find_cases as fc
    out = {}
    for src in FIND_PATTERNS:
        out.update({f"{src}/{k}": v for k, v in _mine_out(_lib.mine_host(fc.FLAT, fc.OFFS, fc.pattern(src), MINE_TOP)).items()})
    return out


@functools.lru_cache(maxsize=None)
def _first_positions(src):
    """the reference's matches -> {matched bytes: the offset of its first occurrence in the batch's text}"""
    import find_cases as fc
    first = {}
    for i, (row, spans) in enumerate(zip(fc.ROWS, fc.spans_of(src, fc.ROWS, fc.SPACES))):
        for a, b in spans:
            first.setdefault(row[a:b], int(fc.OFFS[i]) + a)
    return first


def _check_mine(out):
    import find_cases as fc
    for src in FIND_PATTERNS:
        want_count, _, _, want_top = fc.want(src)
        assert len(want_top) >= 1 and want_top[0][1] > 0, (src, "the reference holds no idiom")
        res = tuple(out[f"{src}/{k}"] for k in ("pos", "len", "count")) + tuple(int(x) for x in out[f"{src}/totals"])
        got, n_distinct, n_matches = fc.mined(fc.FLAT, res)
        assert got == want_top[:MINE_TOP] and n_distinct == len(want_top) and n_matches == int(want_count.sum()), src
        assert out[f"{src}/pos"].tolist() == [_first_positions(src)[m] for m, _ in got], (src, "pos is the first occurrence")


_add("mine", ("tgx_corpus_mine_device",), _run_mine, _check_mine, _twin_mine)


# ---- word ids (csrc/words.hip): a summary per chunk, a scan, the emit; a result comes back --------------------------------------
WORDS_CASES = ("edges", "rows", "at63", "at64", "fold", "long")   # (long: one word of 66 000 bytes, a scan of more than one block)
WORDS_FOLD = True


def _run_words(ctx):
    import test_words_cpu as wc
    out = {}
    for name in WORDS_CASES:
        text, offs, _, _ = wc.case(name, WORDS_FOLD)
        corpus = tgx.NativeCorpus(text, offs)
        res = corpus.words(_lib.words_flags(WORDS_FOLD), wc.SEED, stream=ctx.stream)
        out[f"{name}/ids"], out[f"{name}/offs"] = res.ids(), res.offsets()
        res.free()
        corpus.free()
    return out


def _twin_words():
    import test_words_cpu as wc
    out = {}
    for name in WORDS_CASES:
        text, offs, _, _ = wc.case(name, WORDS_FOLD)
        out[f"{name}/ids"], out[f"{name}/offs"] = _lib.words_host(text, offs, WORDS_FOLD, wc.SEED)
    return out


def _check_words(out):
    import test_words_cpu as wc
    for name in WORDS_CASES:
        _, _, want_ids, want_offs = wc.case(name, WORDS_FOLD)
        assert want_ids.size > 0, (name, "the reference holds no word")
        _eq(out[f"{name}/offs"], want_offs, (name, "offsets"))
        _eq(out[f"{name}/ids"], want_ids, (name, "ids"))


_add("words", ("tgx_corpus_words",), _run_words, _check_words, _twin_words)


# ---- per-row word statistics (csrc/wordstat.hip) --------------------------------------------------------------------------------
WORDSTAT_CASES = ("short_rows", "edges_chunk", "edges_tile", "edges_two_tiles", "stop_words", "bullets", "ellipses", "past_cap")
WORDSTAT_COMBO = (5, "char", True, True)   # limit, unit, fold, with the stop table


@functools.lru_cache(maxsize=None)
def wordstat_case(name):
    """a case of wordstat_cases, read-only: computed once and shared with tests/test_wordstat_gpu.py"""
    import wordstat_cases
    c = wordstat_cases.past_cap_case() if name == "past_cap" else wordstat_cases.case(name)
    for a in (c["text"], c["offs"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def wordstat_want(name, combo):
    """the checker's (table, marks) of a case under a combination: computed once, never changed"""
    import wordstat_checker as ck
    from wordstat_cases import table_for
    c = wordstat_case(name)
    out = ck.stats_of(c["text"], c["offs"], combo[0], table_for(combo[2], combo[3]), combo[1], combo[2])
    for a in out:
        a.setflags(write=False)
    return out


def _wordstat_entry(with_marks):
    from wordstat_cases import table_for
    limit, unit, fold, with_table = WORDSTAT_COMBO

    def run(ctx):
        out = {}
        for name in WORDSTAT_CASES:
            c = wordstat_case(name)
            corpus = tgx.NativeCorpus(c["text"], c["offs"])
            S, N = len(c["offs"]) - 1, c["text"].size
            table, marks = ctx.full((_lib.WORDSTAT_N, S), "int64", ROW), ctx.full((max(N, 1),), "uint8", BYTE)
            corpus.word_stats(table.data_ptr(), marks.data_ptr() if with_marks and N else 0, limit, table_for(fold, with_table), unit, fold, stream=ctx.stream)
            out[f"{name}/table"], out[f"{name}/marks"] = _np(table), _np(marks)[:N]
            corpus.free()
        return out

    def twin():
        out = {}
        for name in WORDSTAT_CASES:
            c = wordstat_case(name)
            table, marks = _lib.word_stats_host(c["text"], c["offs"], limit, table_for(fold, with_table), unit, fold)
            out[f"{name}/table"], out[f"{name}/marks"] = table, marks if with_marks else np.full_like(marks, BYTE)
        return out

    def check(out):
        for name in WORDSTAT_CASES:
            want, want_marks = wordstat_want(name, WORDSTAT_COMBO)
            assert want.any() and want_marks.any(), (name, "the reference holds nothing")
            assert np.array_equal(out[f"{name}/table"], want), (name, "table")
            assert np.array_equal(out[f"{name}/marks"], want_marks) if with_marks else (out[f"{name}/marks"] == BYTE).all(), (name, "marks")

    _add(f"word_stats_{'with' if with_marks else 'without'}_marks", ("tgx_corpus_word_stats_device",), run, check, twin)


_wordstat_entry(True)
_wordstat_entry(False)


# ---- literal phrases (csrc/phrase.hip): the set is built on the device, the hits read it ------------------------------------------
PHRASE_CASES = (("lens123", "bytes"), ("max_len", "bytes"), ("max_len", "ids"), ("edges", "bytes"), ("edges", "ids"), ("all_bytes", "bytes"),
                ("past_cap", "bytes"), ("past_cap", "ids"), ("large_set", "bytes"))
PHRASE_COMBO = (False, False)   # fold_case, whole_word


@functools.lru_cache(maxsize=None)
def phrase_case(name, kind):
    """a case of phrase_cases, read-only: computed once and shared with tests/test_phrase_gpu.py"""
    import phrase_cases
    c = phrase_cases.case(name, kind)
    for a in (c["data"], c["offs"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def phrase_want(name, kind, combo):
    """the checker's (count, longest, per_phrase) of a case under a combination: computed once, never changed"""
    import phrase_checker as ck
    c = phrase_case(name, kind)
    out = ck.hits_of(c["data"], c["offs"], c["phrases"], *combo)
    for a in out:
        a.setflags(write=False)
    return out


def phrase_source(c):
    return _lib.NativeResult.from_ids(c["data"], c["offs"], c["vocab_size"]) if c["kind"] == "ids" else _lib.NativeCorpus(c["data"], c["offs"])


_PHRASE_OUTS = (("count", ROW), ("longest", BYTE), ("per", ROW))


def _phrase_entry(outs):
    """outs: bit 0 the counts, 1 longest, 2 per_phrase"""

    def run(ctx):
        out = {}
        for name, kind in PHRASE_CASES:
            c = phrase_case(name, kind)
            src = phrase_source(c)
            ps = tgx.phrase_set(c["phrases"], kind=kind)
            S, N, P = len(c["offs"]) - 1, c["data"].size, len(c["phrases"])
            count, longest, per = ctx.full((S,), "int64", ROW), ctx.full((N,), "uint8", BYTE), ctx.full((P,), "int64", ROW)
            src.phrase_hits(ps, count.data_ptr() if outs & 1 else 0, longest.data_ptr() if outs & 2 else 0, per.data_ptr() if outs & 4 else 0,
                            stream=ctx.stream)
            out[f"{name}/{kind}/count"], out[f"{name}/{kind}/longest"], out[f"{name}/{kind}/per"] = _np(count), _np(longest), _np(per)
            ps.free()
            src.free()
        return out

    def twin():
        out = {}
        for name, kind in PHRASE_CASES:
            c = phrase_case(name, kind)
            got = _lib.phrase_hits_host(c["data"], c["offs"], c["phrases"], *PHRASE_COMBO)
            for k, (stat, sentinel) in enumerate(_PHRASE_OUTS):
                out[f"{name}/{kind}/{stat}"] = got[k] if outs >> k & 1 else np.full_like(got[k], sentinel)
        return out

    def check(out):
        for name, kind in PHRASE_CASES:
            want = phrase_want(name, kind, PHRASE_COMBO)
            assert want[0].sum() > 0 and want[1].any() and want[2].any(), (name, kind, "the reference holds nothing")
            for k, (stat, sentinel) in enumerate(_PHRASE_OUTS):
                got = out[f"{name}/{kind}/{stat}"]
                assert np.array_equal(got, want[k]) if outs >> k & 1 else (got == sentinel).all(), (name, kind, stat)

    _add(f"phrase_hits_outs_{outs}", ("tgx_phraseset_create", "tgx_corpus_phrase_hits_device", "tgx_result_phrase_hits_device"), run, check, twin)


_phrase_entry(7)
_phrase_entry(1)


# ---- hashed n-gram features (csrc/hashed.hip): the bucket counts are atomic adds; on either side of the LDS threshold ------------
HASHED_WIDTHS = {"ids": (2, 3), "bytes": (3, 50)}   # (50: most rows are shorter than the width)
HASHED_K = 3


@functools.lru_cache(maxsize=None)
def _hashed_combos():
    """(kind, widths, B): 1 000 buckets fit the LDS tables; one more than the counts' threshold does not, for counts or scores"""
    over = _lib.hashed_info(1)["lds_max_buckets"] + 1
    assert over > _lib.hashed_info(HASHED_K)["lds_max_buckets"] >= 1000
    return tuple((kind, HASHED_WIDTHS[kind], B) for kind in ("ids", "bytes") for B in (1000, over))


def _hashed_source(kind, data, offs):
    return _lib.NativeResult.from_ids(data, offs, 2**31) if kind == "ids" else _lib.NativeCorpus(data, offs)


def _run_hashed(ctx):
    import hashed_cases as hc
    out = {}
    for kind, widths, B in _hashed_combos():
        data, offs = hc.batch(kind)
        src = _hashed_source(kind, data, offs)
        counts, scores = ctx.full((B,), "int64", ROW), ctx.full((offs.size - 1, HASHED_K), "int64", ROW)
        d_q = ctx.dev(hc.weights(B, HASHED_K))
        _lib.hashed_counts_device(src, widths, B, hc.SEED, counts.data_ptr(), stream=ctx.stream)
        _lib.hashed_scores_device(src, widths, B, HASHED_K, hc.SEED, d_q.data_ptr(), scores.data_ptr(), stream=ctx.stream)
        out[f"{kind}/{B}/counts"], out[f"{kind}/{B}/scores"] = _np(counts), _np(scores)
        src.free()
    return out


def _twin_hashed():
    import hashed_cases as hc
    out = {}
    for kind, widths, B in _hashed_combos():
        data, offs = hc.batch(kind)
        out[f"{kind}/{B}/counts"] = _lib.hashed_counts_host(data, offs, widths, B, hc.SEED)
        out[f"{kind}/{B}/scores"] = _lib.hashed_scores_host(data, offs, widths, hc.weights(B, HASHED_K), hc.SEED)
    return out


@functools.lru_cache(maxsize=None)
def _hashed_want(kind, widths, B):
    import hashed_cases as hc
    return hc.reference(*hc.batch(kind), widths, B, hc.SEED, hc.weights(B, HASHED_K))


def _check_hashed(out):
    for kind, widths, B in _hashed_combos():
        counts, scores = _hashed_want(kind, widths, B)
        assert counts.sum() > 0 and scores.any(), (kind, B, "the reference holds nothing")
        _eq(out[f"{kind}/{B}/counts"], counts, (kind, B, "counts"))
        _eq(out[f"{kind}/{B}/scores"], scores, (kind, B, "scores"))


_add("hashed_counts_and_scores", ("tgx_corpus_hashed_counts_device", "tgx_result_hashed_counts_device", "tgx_corpus_hashed_scores_device",
                                  "tgx_result_hashed_scores_device"), _run_hashed, _check_hashed, _twin_hashed)


# ---- duplicate spans across rows (csrc/dupspan.hip): keys, a sort on the masked key, the walk back, the cover's window -----------
def _dupspan_cases():
    """(name, kind, width, key_bits): 4 bits force the walk back through a run of other grams; 64 and 20 are the ordinary sorts"""
    out = []
    for kind in ("bytes", "ids"):
        out += [("paste", kind, 5, 64), ("paste", kind, 5, 4), ("twins", kind, 13, 20), ("twins", kind, 2, 1), ("edges_tile", kind, 5, 20),
                ("row_end", kind, 13, 64)]
    return out


def _dupspan_source(c):
    return _lib.NativeResult.from_ids(c["data"], c["offs"], 2**31) if c["kind"] == "ids" else _lib.NativeCorpus(c["data"], c["offs"])


def _dupspan_entry(name, with_mask):
    import dupspan_cases as dsc

    def run(ctx):
        out = {}
        for case, kind, w, bits in _dupspan_cases():
            c = dsc.checked_case(case, kind, w)
            src = _dupspan_source(c)
            table, mask = ctx.full((3, len(c["offs"]) - 1), "int64", ROW), ctx.full((c["data"].size,), "uint8", BYTE)
            src.dup_spans(w, bits, bits, table.data_ptr(), mask.data_ptr() if with_mask else 0, stream=ctx.stream)
            out[f"{case}/{kind}/{w}/{bits}/table"], out[f"{case}/{kind}/{w}/{bits}/mask"] = _np(table), _np(mask)
            src.free()
        return out

    def twin():
        out = {}
        for case, kind, w, bits in _dupspan_cases():
            c = dsc.checked_case(case, kind, w)
            table, mask = _lib.dup_spans_host(c["data"], c["offs"], w, bits, seed=bits)
            out[f"{case}/{kind}/{w}/{bits}/table"], out[f"{case}/{kind}/{w}/{bits}/mask"] = table, mask if with_mask else np.full_like(mask, BYTE)
        return out

    def check(out):
        for case, kind, w, bits in _dupspan_cases():
            want_table, want_mask = dsc.checked_case(case, kind, w)["want"]
            assert want_table[1].sum() > 0 and want_mask.any(), (case, kind, w, "the reference holds no duplicate span")
            _eq(out[f"{case}/{kind}/{w}/{bits}/table"], want_table, (case, kind, w, bits, "table"))
            if with_mask:
                _eq(out[f"{case}/{kind}/{w}/{bits}/mask"], want_mask, (case, kind, w, bits, "mask"))
            else:
                _held(out[f"{case}/{kind}/{w}/{bits}/mask"], BYTE, (case, kind, w, bits, "mask"))

    _add(name, ("tgx_corpus_dup_spans_device", "tgx_result_dup_spans_device"), run, check, twin)


_dupspan_entry("dup_spans", True)
_dupspan_entry("dup_spans_table_alone", False)


# ---- the allow pattern inside the document-frequency pass (csrc/allow.hip; csrc/generate.hip's allocator) ----------------------
ALLOW_MTL = 32


def _allow_out(c, which, table, n_windows, n_distinct, cutoff):
    keys = sorted(table)
    assert all(b"\x00" not in k for k in keys)
    return {f"{c['name']}/{which}/strings": np.frombuffer(b"\x00".join(keys), np.uint8).copy(),
            f"{c['name']}/{which}/df": np.array([table[k] for k in keys] + [n_windows, n_distinct, cutoff], np.int64)}


def _run_allow(ctx):
    import allow_cases as ac
    import generate_cases as gc
    out = {}
    for which in ("A", "B"):
        for c in ac.chunk_cases():
            flat, pb, pe, ps, po = gc.arrays(c)
            pos, ln, df, n_windows, n_distinct, cutoff = _lib.substring_df_allow(flat, pb, pe, ps, ALLOW_MTL, 0, ac.automaton(which), part_origin=po)
            table = {c["text"][int(p):int(p) + int(l)]: int(d) for p, l, d in zip(pos, ln, df)}
            assert len(table) == pos.size, "a substring came back twice"
            out.update(_allow_out(c, which, table, n_windows, n_distinct, cutoff))
    return out


def _twin_allow():
    """the host twin of the pass's first kernel gives the kept windows; the table is their substrings, each with the number of
    samples that hold it"""
    import allow_cases as ac
    import generate_cases as gc
    out = {}
    for which in ("A", "B"):
        for c in ac.chunk_cases():
            flat, pb, pe, ps, po = gc.arrays(c)
            mask, n_windows = _lib.allow_masks_host(flat, pb, pe, ps, ALLOW_MTL, ac.automaton(which), part_origin=po)
            sets: dict = {}
            for b, e, s in c["parts"]:
                for p in range(b, e):
                    for ln in range(1, ALLOW_MTL + 1):
                        if int(mask[p]) >> (ln - 1) & 1:
                            sets.setdefault(c["text"][p:p + ln], set()).add(s)
            out.update(_allow_out(c, which, {k: len(v) for k, v in sets.items()}, n_windows, len(sets), 0))
    return out


def _check_allow(out):
    import allow_cases as ac
    for which in ("A", "B"):
        for c in ac.chunk_cases():
            _, want, want_windows = ac.reference(c, which, ALLOW_MTL)
            assert len(want) > 0 and want_windows > 0, (c["name"], which, "the reference holds nothing")
            strings, df = out[f"{c['name']}/{which}/strings"], out[f"{c['name']}/{which}/df"]
            keys = bytes(strings).split(b"\x00")
            assert len(keys) == df.size - 3 and dict(zip(keys, df[:-3].tolist())) == want, (c["name"], which, "table")
            assert df[-3:].tolist() == [want_windows, len(want), 0], (c["name"], which, "windows, distinct, cutoff")


_add("substring_df_allow", ("tgx_substring_df_allow",), _run_allow, _check_allow, _twin_allow)
