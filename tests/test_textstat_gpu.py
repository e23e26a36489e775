"""Per-row text statistics and the line view on the GPU (tgx_corpus_text_stats_device, tgx_corpus_lines;
csrc/textstat.hip) against the independent checker (tests/textstat_checker.py), the host twins and Python's own strings,
on the batches of tests/textstat_cases.py under both units and both limits (one batch past the cap of the kernels'
grid), and on real text: test_dedup_gpu.py's corpus with three planted rows that the quality filters must drop.
Everything is compared exactly: this is integer work."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import dedup_checker as dc
import textstat_cases
import textstat_checker as tc
from textstat_cases import LIMITS

STAGES = ["textstat_summary_kernel", "textstat_scan", "textstat_kernel", "textstat_lines"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """a case with the checker's answers: computed once, never changed"""
    c = textstat_cases.past_cap_case() if name == "past_cap" else textstat_cases.case(name)
    c["want"] = {(limit, unit): tc.stats_of(c["text"], c["offs"], limit, unit) for limit in LIMITS for unit in tc.UNITS}
    c["lines"] = tc.lines_of(c["text"], c["offs"])
    c["truth"] = [tc.second_truth(raw) for raw in tc.rows_of(c["text"], c["offs"])]
    for a in (c["text"], c["offs"]) + c["lines"] + tuple(x for pair in c["want"].values() for x in pair):
        a.setflags(write=False)
    return c


def _np(t):
    return t.cpu().numpy()


def _check_case(c):
    import torch
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    S, N = len(c["offs"]) - 1, c["text"].size
    try:
        for (limit, unit), (want, want_marks) in c["want"].items():
            s = tgx.text_stats(corpus, unit=unit, line_limit=limit, return_line_start=True)
            assert s.table.dtype == torch.int64 and s.table.shape == (tc.N, S) and s.table.device.type == "cuda" and s.unit == unit
            assert s.line_start.dtype == torch.uint8 and s.line_start.shape == (N,)
            times = _lib.textstat_last_times()
            assert list(times) == STAGES and all(t > 0 for t in list(times.values())[:3]) and times["textstat_lines"] == 0
            twin, twin_marks = _lib.text_stats_host(c["text"], c["offs"], limit, unit)
            for k, name in enumerate(tc.NAMES):
                assert np.array_equal(_np(s.table[k]), want[k]) and np.array_equal(_np(getattr(s, name)), twin[k]), (name, limit, unit)
            assert np.array_equal(_np(s.line_start), want_marks) and np.array_equal(twin_marks, want_marks)
            if unit == "char":
                got = _np(s.table)
                for i, truth in enumerate(c["truth"]):
                    if truth is not None:
                        lens = truth[1]
                        assert (got[1, i], got[3, i], got[4, i], got[5, i]) == (truth[0], len(lens), max(lens, default=0), sum(n > limit for n in lens)), i
            # every byte of both outputs is written: over a sentinel, each alone
            table = torch.full((tc.N, S), -7, dtype=torch.int64, device="cuda")
            marks = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
            corpus.text_stats(table.data_ptr(), 0, limit, unit)
            assert np.array_equal(_np(table), want) and (_np(marks) == 7).all()
            corpus.text_stats(0, marks.data_ptr(), limit, unit)
            assert np.array_equal(_np(marks), want_marks)
            assert np.array_equal(_np(tgx.text_stats(corpus, unit=unit, line_limit=limit).table), want), "the table alone"
            units = want[1] if unit == "char" else want[0]
            assert np.array_equal(_np(s.mean_line), (units - want[2]).astype(np.float64) / np.maximum(want[3], 1))
            assert np.array_equal(_np(s.alnum_frac), (want[6] + want[7]).astype(np.float64) / np.maximum(want[1], 1))
        assert np.array_equal(corpus.bytes(), c["text"]) and np.array_equal(corpus.offsets(), c["offs"]), "the inputs are only read"
    finally:
        corpus.free()


@pytest.mark.parametrize("name", textstat_cases.NAMES)
def test_device_matches_checker_twin_and_truth(name):
    _check_case(_case(name))


def test_past_the_cap():
    """2048·256 + 2·256 + 70 bytes: a block takes two tiles, and in the second a wave gallops from the `hi` of its chunk
    of the first; one line goes from a run's first tile into its second, one from one block's run into the next, inside
    one row over both; the last working block takes one short tile (tests/test_textstat_cpu.py holds the batch to this)"""
    _check_case(_case("past_cap"))


@pytest.mark.parametrize("name", textstat_cases.NAMES + ("past_cap",))
def test_line_rows(name):
    import torch
    c = _case(name)
    want_offs, want_row = c["lines"]
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    try:
        lines, line_row = tgx.line_rows(corpus)
        times = _lib.textstat_last_times()   # (of line_rows' own statistics call, which came last)
        assert list(times) == STAGES
        assert lines.num_samples == want_row.size and lines.num_bytes == c["text"].size
        assert np.array_equal(lines.offsets(), want_offs) and np.array_equal(lines.bytes(), c["text"])
        assert line_row.dtype == torch.int64 and np.array_equal(_np(line_row), want_row)
        assert np.array_equal(_lib.lines_host(c["text"], c["offs"]), want_offs)
        again = corpus.lines()
        times = _lib.textstat_last_times()
        assert all(t > 0 for t in times.values()), times
        assert np.array_equal(again.offsets(), want_offs)
        again.free()
        lines.free()
        assert np.array_equal(corpus.bytes(), c["text"]) and np.array_equal(corpus.offsets(), c["offs"]), "the inputs are only read"
    finally:
        corpus.free()


def test_no_rows_no_bytes_no_lines():
    import torch
    none = np.zeros(0, np.uint8)
    nothing, empties = _lib.NativeCorpus(none, np.zeros(1, np.uint64)), _lib.NativeCorpus(none, np.zeros(6, np.uint64))
    try:
        s = tgx.text_stats(nothing, return_line_start=True)
        assert s.table.shape == (tc.N, 0) and s.line_start.shape == (0,) and tgx.quality_rows(nothing).shape == (0,)
        table = torch.full((tc.N, 5), -7, dtype=torch.int64, device="cuda")
        empties.text_stats(table.data_ptr(), 0)
        assert not _np(table).any(), "rows without bytes are never visited and keep the pre-set 0"
        assert _np(tgx.quality_rows(empties)).tolist() == [0, 1, 2, 3, 4], "an empty row is kept"
        for corpus in (nothing, empties):
            lines, line_row = tgx.line_rows(corpus)
            assert lines.num_samples == 0 and lines.num_bytes == 0 and lines.offsets().tolist() == [0] and line_row.shape == (0,)
            lines.free()
    finally:
        nothing.free()
        empties.free()


def test_duplicate_lines_through_first_equal():
    """a planted line repeated within one row and across two rows: first_equal of the line view finds exactly those"""
    plant = b"import numpy as np\n"
    rows = [b"a = 1\n" + plant + b"b = 2\n" + plant + b"c", b"", b"x\ny\n", b"z = 0\n" + plant + b"last line without its terminator"]
    text, offs = textstat_cases.pack(rows)
    corpus = _lib.NativeCorpus(text, offs)
    try:
        lines, line_row = tgx.line_rows(corpus)
        first = _np(tgx.first_equal(lines))
        got = dc.row_bytes(lines.bytes(), lines.offsets())
        assert got == [b"a = 1\n", plant, b"b = 2\n", plant, b"c", b"x\n", b"y\n", b"z = 0\n", plant, b"last line without its terminator"]
        assert _np(line_row).tolist() == [0, 0, 0, 0, 0, 2, 2, 3, 3, 3]
        assert first.tolist() == [0, 1, 2, 1, 4, 5, 6, 7, 1, 9]
        lines.free()
    finally:
        corpus.free()


def test_bad_arguments_are_refused_before_anything_is_queued():
    import torch
    lib = _lib.lib
    c = _case("edges_chunk")
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    S, N = corpus.num_samples, c["text"].size
    table = torch.full((tc.N, S), -7, dtype=torch.int64, device="cuda")
    marks = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    h_table, h_marks = np.full((tc.N, S), 9, np.int64), np.full(N, 9, np.uint8)
    stats, p = lib.tgx_corpus_text_stats_device, lambda t: t.data_ptr()
    try:
        assert stats(corpus._h, 5, 0, None, _lib.ptr(h_table), p(marks)) == _lib.ERR_INVALID               # host memory
        assert "not device memory" in lib.tgx_last_error().decode()
        assert stats(corpus._h, 5, 0, None, p(table), _lib.ptr(h_marks)) == _lib.ERR_INVALID
        assert stats(corpus._h, 5, 2, None, p(table), p(marks)) == _lib.ERR_INVALID                        # an unknown flag
        assert stats(corpus._h, 5, 0, None, None, None) == _lib.ERR_INVALID                                # no output
        assert stats(None, 5, 0, None, p(table), p(marks)) == _lib.ERR_INVALID
        out = C.c_void_p(7)
        assert lib.tgx_corpus_lines(corpus._h, 1, None, C.byref(out)) == _lib.ERR_INVALID and not out.value  # flags
        assert lib.tgx_corpus_lines(None, 0, None, C.byref(out)) == _lib.ERR_INVALID and lib.tgx_corpus_lines(corpus._h, 0, None, None) == _lib.ERR_INVALID
        if torch.cuda.device_count() >= 2:
            there = torch.full((tc.N, S), -7, dtype=torch.int64, device="cuda:1")
            assert stats(corpus._h, 5, 0, None, p(there), p(marks)) == _lib.ERR_INVALID                    # an output on another device
        torch.cuda.synchronize()
        assert (_np(table) == -7).all() and (_np(marks) == 7).all() and (h_table == 9).all() and (h_marks == 9).all()   # nothing was written
        with pytest.raises(ValueError):
            tgx.text_stats(corpus, unit="word")
    finally:
        corpus.free()


def test_on_torchs_current_stream_and_from_another_device():
    import torch
    c = _case("edges_tile")
    want, want_marks = c["want"][(5, "char")]
    corpus = _lib.NativeCorpus(c["text"], c["offs"])
    stream = torch.cuda.Stream(device=0)
    try:
        with torch.cuda.stream(stream):        # tensors.* pick up torch's current stream
            s = tgx.text_stats(corpus, line_limit=5, return_line_start=True)
            lines, line_row = tgx.line_rows(corpus)
        assert np.array_equal(_np(s.table), want) and np.array_equal(_np(s.line_start), want_marks)
        assert np.array_equal(lines.offsets(), c["lines"][0]) and np.array_equal(_np(line_row), c["lines"][1])
        lines.free()
        if torch.cuda.device_count() >= 2:
            with torch.cuda.device(1):         # the corpus lives on device 0
                table = torch.full((tc.N, len(c["offs"]) - 1), -7, dtype=torch.int64, device="cuda:0")
                corpus.text_stats(table.data_ptr(), 0, 5, "char", stream=stream.cuda_stream)
                assert torch.cuda.current_device() == 1
            assert np.array_equal(_np(table), want)
    finally:
        corpus.free()


# ---- real text --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _texts():
    """test_dedup_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end.  Planted into it: a row with one line of 1 500
    characters among short ones, a row of 150-character lines, a row of punctuation and hex with few letters and digits."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    texts = [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]
    long_line = b"".join(b"value_%d = compute(%d)\n" % (k, k) for k in range(60)) + ("x = '" + "aé b" * 373 + "';#\n").encode() + b"done = True\n" * 60
    wide = b"".join(b"%0150d\n" % (k * 7919) for k in range(20))
    noise = b"".join(b"{{[[((--++==::;;..,,//\\\\||!!@@##$$%%^^&&**~~``<<>>??__  0x1f}})]\n" for _ in range(30))
    planted = {7: long_line, len(texts) // 2: wide, len(texts) - 4: noise}
    for at, row in sorted(planted.items(), reverse=True):
        texts.insert(at, row)
    where = [texts.index(row) for row in (long_line, wide, noise)]
    return texts, where


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], [])


def test_quality_rows_on_real_text():
    texts, (r_long, r_wide, r_noise) = _texts()
    assert max(len(t) for t in texts) == 70_000, "the 70 000-byte row is present"
    flat, offs = tgx.pack(texts)
    want, _ = tc.stats_of(flat, offs, 1000, "char")
    d = dict(zip(tc.NAMES, want))
    assert d["max_line"][r_long] == 5 + 4 * 373 + 3 == 1500 and d["long_lines"][r_long] == 1 and d["max_line"][r_wide] == 150 and d["max_line"][r_noise] < 100
    assert (d["alpha"][r_noise] + d["digit"][r_noise]) / d["chars"][r_noise] < 0.25
    tk = _tokenizer()
    nat = tk.native_model()
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    try:
        s = tgx.text_stats(corpus)
        assert np.array_equal(_np(s.table), want)
        for unit in tc.UNITS:
            keep = _np(tgx.quality_rows(corpus, unit=unit))
            assert np.array_equal(keep, tc.keep_list(flat, offs, unit=unit)) and not {r_long, r_wide, r_noise} & set(keep.tolist()), unit
        # each planted row fails one rule alone: without that rule it is kept
        for row, rule in ((r_long, dict(max_line=10 ** 9)), (r_wide, dict(mean_line=1e9)), (r_noise, dict(min_alnum=0.0))):
            relaxed = _np(tgx.quality_rows(corpus, **rule))
            assert np.array_equal(relaxed, tc.keep_list(flat, offs, **rule)) and row in relaxed.tolist(), rule
        keep = tgx.quality_rows(corpus)
        want_keep = tc.keep_list(flat, offs)
        assert 0 < want_keep.size < len(texts)
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
