"""Exact row deduplication on the GPU (tgx_corpus_first_equal_device, tgx_result_first_equal_device,
tgx_*_row_hashes_device; csrc/dedup.hip) against the independent checker (tests/dedup_checker.py) and the host twin, at
the default 64 key bits and, through the test knob TGX_DEDUP_HASH_BITS, at 4 and 0 bits, where rows collide and the
rounds go on; the unique rows of a corpus and of its encoded result stay aligned on real text.  Everything is compared
exactly: this is integer work.

The shapes are tests/dedup_cases.py's, among them one batch per kind that takes every capped grid past its cap (over
8 MiB of padded bytes, over 2048 tiles of candidates, over 2^19 rows); the real text is test_assemble_gpu.py's corpus,
96 KiB of mixed text with a 70 000-byte sample and empty samples, a third of its rows repeated through select, under the
spec 32 000 vocabulary."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import dedup_cases
import dedup_checker as dc

KNOB = "TGX_DEDUP_HASH_BITS"


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """a case with the checker's and the twin's answers: computed once, never changed"""
    c = dedup_cases.case(name, kind)
    c["want"] = dc.first_equal(c["data"], c["offs"])
    c["twin"] = {bits: _lib.first_equal_host(c["data"], c["offs"], hash_bits=bits) for bits in (64, 4, 0)}
    for a in (c["data"], c["offs"], c["want"][0]):
        a.setflags(write=False)
    return c


def _source(c):
    if c["kind"] == "ids":
        return _lib.NativeResult.from_ids(c["data"], c["offs"], c["vocab_size"])
    return _lib.NativeCorpus(c["data"], c["offs"])


def _read(obj, kind):
    return (obj.ids(), obj.offsets()) if kind == "ids" else (obj.bytes(), obj.offsets())


class _bits:
    """TGX_DEDUP_HASH_BITS set around a call and put back (None: not set)"""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        self.before = os.environ.pop(KNOB, None)
        if self.bits is not None:
            os.environ[KNOB] = str(self.bits)

    def __exit__(self, *exc):
        os.environ.pop(KNOB, None)
        if self.before is not None:
            os.environ[KNOB] = self.before


def _first_equal(obj, stream=0):
    import torch
    out = torch.full((obj.num_samples,), -5, dtype=torch.int64, device=torch.device("cuda", obj.device))
    n_unique = obj.first_equal(out.data_ptr() if out.numel() else 0, stream=stream)
    return out.cpu().numpy(), n_unique


@pytest.mark.parametrize("name,kind", dedup_cases.all_cases())
def test_device_matches_checker_and_twin(name, kind):
    c = _case(name, kind)
    want_first, want_unique = c["want"]
    src = _source(c)
    try:
        for bits in (None, 4, 0):
            with _bits(bits):
                first, n_unique = _first_equal(src)
            twin_first, twin_unique, twin_rounds = c["twin"][64 if bits is None else bits]
            assert np.array_equal(first, want_first), bits
            assert np.array_equal(first, twin_first), bits
            assert n_unique == want_unique == twin_unique, bits
            assert _lib.dedup_last_rounds() == twin_rounds, bits
            if bits is None:
                assert twin_rounds == 1
            if bits == 0:
                assert twin_rounds == c["n_distinct"]
        got = _read(src, kind)
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
        times = _lib.dedup_last_times()
        assert list(times) == ["dedup_hash_kernel", "dedup_sort", "dedup_compare_kernel", "dedup_resolve"]
        assert all(t >= 0 for t in times.values()) and times["dedup_hash_kernel"] > 0
    finally:
        src.free()


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_row_hashes_are_tgx_row_hash_of_every_row(kind):
    for name in ("lengths", "tile_edges", "alignments", "trailing_zero", "word_swap", "long"):
        c = _case(name, kind)
        rows = dc.row_bytes(c["data"], c["offs"])
        src = _source(c)
        try:
            for seed in (0, 0x9E3779B97F4A7C15):
                got = tensors.row_hashes(src, seed).cpu().numpy().view(np.uint64)
                want = np.asarray([dc.row_hash(r, seed) for r in rows], np.uint64)
                assert np.array_equal(got, want), (name, seed)
                lib_hash = [_lib.row_hash(r, seed) for r in rows[:8]]
                assert lib_hash == [int(x) for x in want[:8]]
        finally:
            src.free()


# ---- past the caps of the grids: the second tile of a block's run, the second trip of the compare and of the row kernels --

@functools.lru_cache(maxsize=None)
def _past_cap(kind):
    """dedup_cases.past_cap_case with the checker's and the twin's answers: computed once, never changed"""
    c = dedup_cases.past_cap_case(kind)
    c["want"] = dc.first_equal(c["data"], c["offs"])
    c["twin"] = {bits: _lib.first_equal_host(c["data"], c["offs"], hash_bits=bits) for bits in (64, c["low_bits"])}
    for a in (c["data"], c["offs"], c["want"][0]):
        a.setflags(write=False)
    return c


@pytest.mark.parametrize("bits", [None, dedup_cases.PAST_CAP_BITS])
@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_past_the_caps_first_equal(kind, bits):
    """Over 2048·4096 + 4096 padded bytes (a block of dedup_hash_kernel takes two tiles, the last working block one, the
    blocks behind it none), over 2048 tiles of candidates' elements (dedup_compare_kernel goes round twice) and over
    256·2048 rows (so do dedup_finish / runs / resolve_kernel); tests/test_dedup_cpu.py holds the batch to these.  Under
    the knob the later rounds hash over 8 MiB of padded bytes through a compacted list, and the copies of the
    70 000-element row with one element changed are compared, in the compare's second trip, with the row they were made
    from.  The rounds are the twin's, and at most MAX_DISTINCT."""
    c = _past_cap(kind)
    want_first, want_unique = c["want"]
    twin_first, twin_unique, twin_rounds = c["twin"][64 if bits is None else bits]
    assert (twin_rounds == 1) if bits is None else (2 <= twin_rounds <= dedup_cases.MAX_DISTINCT)
    src = _source(c)
    try:
        with _bits(bits):
            first, n_unique = _first_equal(src)
        assert np.array_equal(first, want_first) and np.array_equal(first, twin_first)
        assert n_unique == want_unique == twin_unique
        assert _lib.dedup_last_rounds() == twin_rounds
        got = _read(src, kind)
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
    finally:
        src.free()


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_past_the_caps_row_hashes(kind):
    """every row's hash against the vectorised restatement, and against the scalar one on every long row, on the rows on
    either side of every tile edge, and on a seeded sample of 2 000 short rows"""
    c = _past_cap(kind)
    where = c["where"]
    rows = dc.row_bytes(c["data"], c["offs"])
    S = len(rows)
    rng = np.random.default_rng(8)
    look = np.unique(np.concatenate([where["rows"], where["edge_rows"], rng.choice(S, 2000, replace=False), [0, S - 1]]))
    scalar = functools.lru_cache(maxsize=None)(dc.row_hash)   # (most of these rows are copies of a few)
    src = _source(c)
    try:
        for seed in (0, 0x9E3779B97F4A7C15):
            got = tensors.row_hashes(src, seed).cpu().numpy().view(np.uint64)
            assert np.array_equal(got, dc.row_hashes(c["data"], c["offs"], seed)), seed
            assert [int(x) for x in got[look]] == [scalar(rows[k], seed) for k in look], seed
    finally:
        src.free()


# ---- real text: the unique rows of a corpus and of its encoded result stay aligned --------------------------------

@functools.lru_cache(maxsize=None)
def _texts():
    """test_assemble_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
    samples: two at the start, a run in the middle, one at the end."""
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    return [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]


@functools.lru_cache(maxsize=None)
def _tokenizer():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], [])


def test_unique_rows_keep_corpus_and_result_aligned_on_real_text():
    import torch
    texts = _texts()
    S = len(texts)
    lens = np.asarray([len(t) for t in texts])
    rng = np.random.default_rng(21)
    again = rng.choice(S, S // 3, replace=False)
    again[:2] = (int(np.argmax(lens)), S - 1)          # the 70 000-byte sample and an empty one are among the repeated
    index = np.concatenate([np.arange(S), again])[rng.permutation(S + S // 3)].astype(np.int64)
    flat, offs = tgx.pack(texts)
    tk = _tokenizer()
    nat = tk.native_model()
    base = _lib.NativeCorpus(flat, offs)
    corpus = tgx.select(base, torch.from_numpy(index).cuda())
    base.free()
    d_flat, d_offs = corpus.bytes(), corpus.offsets()
    want_first, want_unique = dc.first_equal(d_flat, d_offs)
    assert want_unique < S and (want_first != np.arange(index.size)).sum() >= S // 3
    res = nat.encode_corpus(corpus)
    try:
        first = tgx.first_equal(corpus)
        assert first.dtype == torch.int64 and first.device.type == "cuda"
        assert np.array_equal(first.cpu().numpy(), want_first)
        assert _lib.dedup_last_rounds() == 1
        keep = tgx.unique_rows(corpus)
        want_keep = np.flatnonzero(want_first == np.arange(index.size))
        assert np.array_equal(keep.cpu().numpy(), want_keep) and keep.numel() == want_unique
        assert np.array_equal(torch.bincount(first, minlength=index.size).cpu().numpy(), np.bincount(want_first, minlength=index.size))
        # the encoded rows are equal exactly where the texts are (the encode is a function of the text, and decodes back to it)
        assert np.array_equal(tgx.first_equal(res).cpu().numpy(), want_first)
        u_corpus, u_res = tgx.select(corpus, keep), tgx.select(res, keep)
        rows = dc.row_bytes(d_flat, d_offs)
        got = dc.row_bytes(u_corpus.bytes(), u_corpus.offsets())
        assert got == [rows[int(k)] for k in want_keep] and len(set(got)) == len(got) and set(got) == set(rows)
        enc = nat.encode_corpus(u_corpus)
        assert np.array_equal(u_res.ids(), enc.ids()) and np.array_equal(u_res.offsets(), enc.offsets())
        dec, dec_offs = tk.decode_result_flat(u_res, False)
        want_dec, want_dec_offs = tk.decode_result_flat(enc, False)
        assert np.array_equal(dec_offs, want_dec_offs) and np.array_equal(dec, want_dec)
        try:
            [t.decode("utf-8") for t in got]
            valid = True
        except UnicodeDecodeError:
            valid = False
        if valid:   # then the decode is the text itself
            assert dc.row_bytes(np.asarray(dec, np.uint8), dec_offs) == got
        for o in (enc, u_res, u_corpus):
            o.free()
    finally:
        res.free()
        corpus.free()


def test_a_stream_of_the_caller_the_null_stream_and_the_current_device():
    import torch
    c = _case("group40", "bytes")
    r = _case("pairs", "ids")
    corpus, res = _source(c), _source(r)
    stream = torch.cuda.Stream(device=corpus.device)
    other = 1 if torch.cuda.device_count() >= 2 else 0
    try:
        for st in (0, stream.cuda_stream):
            torch.cuda.synchronize()
            with torch.cuda.device(other):     # the objects live on device 0
                before = torch.cuda.current_device()
                first, n_unique = _first_equal(corpus, stream=st)
                first_r, n_unique_r = _first_equal(res, stream=st)
                assert torch.cuda.current_device() == before == other
            assert np.array_equal(first, c["want"][0]) and n_unique == c["want"][1]
            assert np.array_equal(first_r, r["want"][0]) and n_unique_r == r["want"][1]
        with torch.cuda.stream(stream):        # tensors.* pick up torch's current stream
            first = tgx.first_equal(corpus)
            hashes = tgx.row_hashes(res, 3)
        assert np.array_equal(first.cpu().numpy(), c["want"][0])
        assert [int(x) for x in hashes.cpu().numpy().view(np.uint64)] == [dc.row_hash(b, 3) for b in dc.row_bytes(r["data"], r["offs"])]
    finally:
        corpus.free()
        res.free()


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_bad_arguments_are_refused_before_anything_is_queued(kind):
    import torch
    lib = _lib.lib
    c = _case("pairs", kind)
    src = _source(c)
    S = src.num_samples
    fn = lib.tgx_result_first_equal_device if kind == "ids" else lib.tgx_corpus_first_equal_device
    hn = lib.tgx_result_row_hashes_device if kind == "ids" else lib.tgx_corpus_row_hashes_device
    host = np.full(S, -9, np.int64)
    dev = torch.full((S,), -5, dtype=torch.int64, device="cuda")
    nu = C.c_uint64(77)
    try:
        assert fn(src._h, 0, None, _lib.ptr(host), C.byref(nu)) == _lib.ERR_INVALID      # host memory
        assert "not device memory" in lib.tgx_last_error().decode() and (host == -9).all()
        assert fn(src._h, 0, None, None, C.byref(nu)) == _lib.ERR_INVALID                # NULL with S > 0
        assert fn(src._h, 1, None, dev.data_ptr(), C.byref(nu)) == _lib.ERR_INVALID      # flags
        assert fn(None, 0, None, dev.data_ptr(), C.byref(nu)) == _lib.ERR_INVALID
        assert hn(src._h, 0, None, _lib.ptr(host.view(np.uint64))) == _lib.ERR_INVALID
        assert hn(src._h, 0, None, None) == _lib.ERR_INVALID
        assert hn(None, 0, None, dev.data_ptr()) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == -5).all()                                           # nothing was written
        assert fn(src._h, 0, None, dev.data_ptr(), None) == 0                            # n_unique may be NULL
        assert np.array_equal(dev.cpu().numpy(), c["want"][0])
    finally:
        src.free()


@pytest.mark.parametrize("kind", dedup_cases.KINDS)
def test_no_rows(kind):
    dt = np.uint32 if kind == "ids" else np.uint8
    src = _source(dict(kind=kind, data=np.zeros(0, dt), offs=np.zeros(1, np.uint64), vocab_size=10))
    try:
        assert src.first_equal(0) == 0 and _lib.dedup_last_rounds() == 0
        src.row_hashes(0)
        assert tgx.first_equal(src).shape == (0,) and tgx.unique_rows(src).shape == (0,) and tgx.row_hashes(src).shape == (0,)
    finally:
        src.free()
    # rows, but none with an element: one content
    src = _source(dict(kind=kind, data=np.zeros(0, dt), offs=np.zeros(6, np.uint64), vocab_size=10))
    try:
        first, n_unique = _first_equal(src)
        assert first.tolist() == [0] * 5 and n_unique == 1 and _lib.dedup_last_rounds() == 1
        assert [int(x) for x in tgx.row_hashes(src).cpu().numpy().view(np.uint64)] == [dc.row_hash(b"")] * 5
    finally:
        src.free()
