"""Per-row word statistics on the GPU (tgx_corpus_word_stats_device; csrc/wordstat.hip) against the independent checker
(tests/wordstat_checker.py) and the host twin, on the batches of tests/wordstat_cases.py under both units, both limits,
with and without the fold and with and without a stop table (one batch past the cap of the kernels' grid), on filled pool
memory, and on real text: test_dedup_gpu.py's corpus with planted rows that each fail one Gopher rule alone.  Everything
is compared exactly: this is integer work."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import dedup_checker as dc
import dirty_runs
import wordstat_cases
import wordstat_checker as ck
from wordstat_cases import COMBOS, table_for

STAGES = ["wordstat_summary_kernel", "wordstat_scan", "wordstat_kernel"]
ALL = wordstat_cases.NAMES + ("past_cap",)


@functools.lru_cache(maxsize=None)
def _case(name):
    """a case with the checker's answers: computed once, never changed"""
    c = wordstat_cases.past_cap_case() if name == "past_cap" else wordstat_cases.case(name)
    c["want"] = {combo: ck.stats_of(c["text"], c["offs"], combo[0], table_for(combo[2], combo[3]), combo[1], combo[2]) for combo in COMBOS}
    for a in (c["text"], c["offs"]) + tuple(x for pair in c["want"].values() for x in pair):
        a.setflags(write=False)
    return c


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", ALL)
def test_device_matches_twin_and_checker(name):
    import torch
    c = _case(name)
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    S, N = len(c["offs"]) - 1, c["text"].size
    try:
        for (limit, unit, fold, with_table), (want, want_marks) in c["want"].items():
            what = (name, limit, unit, fold, with_table)
            stops = table_for(fold, with_table)
            s = tgx.word_stats(corpus, word_limit=limit, stop_words=stops, unit=unit, fold_case=fold, return_mask=True)
            assert s.table.dtype == torch.int64 and s.table.shape == (ck.N, S) and s.table.device.type == "cuda" and s.unit == unit
            assert s.mask.dtype == torch.uint8 and s.mask.shape == (N,)
            times = _lib.wordstat_last_times()
            assert list(times) == STAGES and all(t > 0 for t in times.values()), times
            twin, twin_marks = _lib.word_stats_host(c["text"], c["offs"], limit, stops, unit, fold)
            got = _np(s.table)
            for k, stat in enumerate(ck.NAMES):
                assert np.array_equal(got[k], want[k]) and np.array_equal(_np(getattr(s, stat)), twin[k]), (stat, what)
            assert np.array_equal(_np(s.mask), want_marks) and np.array_equal(twin_marks, want_marks), what
            # every byte of both outputs is written: over a sentinel, each alone
            table = torch.full((ck.N, S), -7, dtype=torch.int64, device="cuda")
            marks = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
            corpus.word_stats(table.data_ptr(), 0, limit, stops, unit, fold)
            assert np.array_equal(_np(table), want) and (_np(marks) == 7).all(), what
            corpus.word_stats(0, marks.data_ptr(), limit, stops, unit, fold)
            assert np.array_equal(_np(marks), want_marks), what
        d = dict(zip(ck.NAMES, want))
        assert np.array_equal(_np(s.mean_word), d["word_units"].astype(np.float64) / np.maximum(d["words"], 1))
        assert np.array_equal(_np(s.alpha_frac), d["alpha_words"].astype(np.float64) / np.maximum(d["words"], 1))
        assert np.array_equal(_np(s.alpha_wide_frac), d["alpha_wide_words"].astype(np.float64) / np.maximum(d["words"], 1))
        assert np.array_equal(_np(s.hash_ratio), d["hash"].astype(np.float64) / np.maximum(d["words"], 1))
        assert np.array_equal(_np(s.ellipsis_ratio), d["ellipsis"].astype(np.float64) / np.maximum(d["words"], 1))
        for share, count in (("bullet_frac", "bullet_lines"), ("ellipsis_line_frac", "ellipsis_lines"), ("punct_line_frac", "punct_lines")):
            assert np.array_equal(_np(getattr(s, share)), d[count].astype(np.float64) / np.maximum(d["lines"], 1)), share
        assert np.array_equal(corpus.bytes(), c["text"]) and np.array_equal(corpus.offsets(), c["offs"]), "the inputs are only read"
    finally:
        corpus.free()


def test_stop_mask_and_lines_agree_with_their_neighbours():
    c = _case("stop_words")
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    try:
        s = tgx.word_stats(corpus, word_limit=5, stop_words=table_for(True, True))
        want = c["want"][(5, "char", True, True)][0]
        assert np.array_equal(_np(s.stop_distinct), [bin(int(m)).count("1") for m in want[ck.NAMES.index("stop_mask")]])
        assert np.array_equal(_np(s.lines), _np(tgx.text_stats(corpus).lines)), "`lines` is the text statistics' own"
    finally:
        corpus.free()


def test_no_rows_and_no_bytes():
    import torch
    none = np.zeros(0, np.uint8)
    nothing, empties = _lib.NativeCorpus(none, np.zeros(1, np.uint64)), _lib.NativeCorpus(none, np.zeros(6, np.uint64))
    try:
        s = tgx.word_stats(nothing, return_mask=True)
        assert s.table.shape == (ck.N, 0) and s.mask.shape == (0,) and tgx.gopher_quality_rows(nothing).shape == (0,)
        table = torch.full((ck.N, 5), -7, dtype=torch.int64, device="cuda")
        empties.word_stats(table.data_ptr(), 0)
        assert not _np(table).any(), "rows without bytes are never visited and keep the pre-set 0"
        assert tgx.gopher_quality_rows(empties).shape == (0,), "an empty row fails min_words"
    finally:
        nothing.free()
        empties.free()


def test_bad_arguments_are_refused_before_anything_is_queued():
    import torch
    lib = _lib.lib
    c = _case("edges_chunk")
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    S, N = corpus.num_samples, c["text"].size
    table = torch.full((ck.N, S), -7, dtype=torch.int64, device="cuda")
    marks = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    h_table, h_marks = np.full((ck.N, S), 9, np.int64), np.full(N, 9, np.uint8)
    stats, p = lib.tgx_corpus_word_stats_device, lambda t: t.data_ptr()
    flat, offs = _lib.pack([b"the", b"of"])
    try:
        assert stats(corpus._h, 5, _lib.ptr(flat), _lib.ptr(offs), 2, 3, None, _lib.ptr(h_table), p(marks)) == _lib.ERR_INVALID   # host memory
        assert "not device memory" in lib.tgx_last_error().decode()
        assert stats(corpus._h, 5, _lib.ptr(flat), _lib.ptr(offs), 2, 3, None, p(table), _lib.ptr(h_marks)) == _lib.ERR_INVALID
        assert stats(corpus._h, 5, _lib.ptr(flat), _lib.ptr(offs), 2, 4, None, p(table), p(marks)) == _lib.ERR_INVALID            # an unknown flag
        assert stats(corpus._h, 5, _lib.ptr(flat), _lib.ptr(offs), 2, 3, None, None, None) == _lib.ERR_INVALID                    # no output
        assert stats(None, 5, _lib.ptr(flat), _lib.ptr(offs), 2, 3, None, p(table), p(marks)) == _lib.ERR_INVALID
        for bad in ([b""], [b"ninebytes"], [b"a b"], [b"the", b"the"], [b"The"], [bytes([97 + k % 26, 97 + k // 26]) for k in range(64)]):
            with pytest.raises(tgx.TokenGeeXError) as e:
                corpus.word_stats(p(table), p(marks), 5, bad)
            assert e.value.status == _lib.ERR_INVALID, bad
        corpus.word_stats(p(table), 0, 5, [b"The"], fold_case=False)   # A-Z is refused only where the text is folded
        table.fill_(-7)
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            tgx.word_stats(corpus, unit="word")
        torch.cuda.synchronize()
        assert (_np(table) == -7).all() and (_np(marks) == 7).all() and (h_table == 9).all() and (h_marks == 9).all()   # nothing was written
    finally:
        corpus.free()


# ---- filled pool memory ---------------------------------------------------------------------------------------------------

FILL_CASES = ("short_rows", "edges_chunk", "edges_tile", "edges_two_tiles", "stop_words", "bullets", "ellipses", "past_cap")
FILL_COMBO = (5, "char", True, True)


def _fill_entry(with_marks):
    """a dirty_runs.Entry of the word statistics, built here and not registered: the registry holds include/tgx.h's
    functions, and this call is declared in include/tgx_words.h"""

    def run(ctx):
        out = {}
        for name in FILL_CASES:
            c = _case(name)
            corpus = tgx.NativeCorpus(c["text"], c["offs"])
            S, N = len(c["offs"]) - 1, c["text"].size
            table, marks = ctx.full((ck.N, S), "int64", -7), ctx.full((max(N, 1),), "uint8", 7)
            corpus.word_stats(table.data_ptr(), marks.data_ptr() if with_marks and N else 0, FILL_COMBO[0], table_for(True, True), FILL_COMBO[1], FILL_COMBO[2],
                              stream=ctx.stream)
            out[f"{name}/table"], out[f"{name}/marks"] = _np(table), _np(marks)[:N]
            corpus.free()
        return out

    def check(out):
        for name in FILL_CASES:
            want, want_marks = _case(name)["want"][FILL_COMBO]
            assert np.array_equal(out[f"{name}/table"], want), (name, "table")
            assert np.array_equal(out[f"{name}/marks"], want_marks) if with_marks else (out[f"{name}/marks"] == 7).all(), (name, "marks")

    return dirty_runs.Entry(f"word_stats_{'with' if with_marks else 'without'}_marks", ("tgx_corpus_word_stats_device",), run, check, {}, True)


@pytest.mark.parametrize("with_marks", [True, False])
def test_on_filled_pool_memory(monkeypatch, with_marks):
    """test_pool_fill_gpu.py's three fills: every pooled buffer of the call (the summaries, the carries, the scan's room,
    the stop table) holds 0, 255 or 1 before its owner sees it, and the outputs are the same bits under all three"""
    import test_pool_fill_gpu as pf
    e = _fill_entry(with_marks)
    ctx = dirty_runs.Ctx()
    tgx.pool_trim()
    runs = {}
    for fill in pf.FILLS:
        monkeypatch.setenv(pf.KNOB, fill)
        before = _lib.pool_filled_bytes()
        out = e.run(ctx)
        assert _lib.pool_filled_bytes() > before, (fill, "nothing was filled")
        e.check(out)
        runs[fill] = out
    for fill in pf.FILLS[1:]:
        pf.same_outputs(e, runs[fill], runs["0"], fill)


# ---- real text --------------------------------------------------------------------------------------------------------

PLANTED = {
    "few_words": (b"the cat and the dog sat with that of mine", dict(min_words=1)),
    "long_words": (b"the and " + b"incomprehensib " * 60, dict(mean_word=(3, 100))),
    "hashes": (b"the and " + b"#tagged " * 60, dict(max_symbol_ratio=10.0)),
    "bullets": (b"- the item and more\n" * 60, dict(max_bullet_lines=1.0)),
    "ellipsis_lines": (b"the story of that night went on and on and then some...\n" * 60, dict(max_ellipsis_lines=1.0)),
    "digits": (b"the and " + b"12345 " * 100, dict(min_alpha_words=0.0)),
    "no_stop_word": (b"quick brown fox jumps over lazy dog " * 9, dict(min_stop_words=0)),
}
# rows that pass every rule (the synthetic text holds no English stop words, so nothing else is kept)
GOOD = (b"The quick brown fox jumps over the lazy dog, and that is all we have to say of it.\n" * 6,
        "Mit dem Wörterbuch and with the café of the town, they have to be here \u2026 or so it seems!\n".encode() * 5)


@functools.lru_cache(maxsize=None)
def _texts():
    """test_dedup_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end.  Planted into it: the rows of PLANTED and of GOOD."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    texts = [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]
    step = len(texts) // (len(PLANTED) + 1)
    for k, (row, _) in reversed(list(enumerate(PLANTED.values()))):
        texts.insert(3 + k * step, row)
    texts.insert(10, GOOD[0])
    texts.insert(len(texts) - 5, GOOD[1])
    where = {key: texts.index(row) for key, (row, _) in PLANTED.items()}
    return texts, where


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], [])


def test_gopher_quality_rows_on_real_text():
    texts, where = _texts()
    assert max(len(t) for t in texts) == 70_000, "the 70 000-byte row is present"
    flat, offs = tgx.pack(texts)
    want, _ = ck.stats_of(flat, offs, 20, ck.GOPHER, "char", True)
    want_keep = ck.keep_of(want)
    assert {texts.index(row) for row in GOOD} <= set(want_keep.tolist()) and not set(where.values()) & set(want_keep.tolist())
    nat = _tokenizer().native_model()
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    try:
        assert np.array_equal(_np(tgx.word_stats(corpus).table), want)
        keep = tgx.gopher_quality_rows(corpus)
        assert np.array_equal(_np(keep), want_keep)
        # each planted row fails one rule alone: without that rule it is kept
        for key, (_, rule) in PLANTED.items():
            relaxed = _np(tgx.gopher_quality_rows(corpus, **rule))
            assert np.array_equal(relaxed, ck.keep_of(want, **rule)) and where[key] in relaxed.tolist(), key
            assert not (set(where.values()) - {where[key]}) & set(relaxed.tolist()), key
        # select by it keeps corpus and result aligned
        k_corpus, k_res = tgx.select(corpus, keep), tgx.select(res, keep)
        assert dc.row_bytes(k_corpus.bytes(), k_corpus.offsets()) == [texts[int(k)] for k in want_keep]
        enc = nat.encode_corpus(k_corpus)
        assert np.array_equal(k_res.ids(), enc.ids()) and np.array_equal(k_res.offsets(), enc.offsets())
        for o in (enc, k_res, k_corpus):
            o.free()
    finally:
        res.free()
        corpus.free()
