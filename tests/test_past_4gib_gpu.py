"""Device calls on sources of more than 2^32 bytes and of more than 2^32 elements (tests/big_cases.py).

Tier A is the base corpus selected 4160 times on the device (4 362 080 320 bytes), Tier B the base result selected 4160
times (1 090 523 200 ids, 4 362 092 800 bytes of them), Tier C the base result selected 16 448 times (4 311 760 960
ids).  In each, the long row of one copy straddles the boundary and 64 whole copies lie behind it.  The content of each
source is first shown by a path that is not under test: Tier A's text is copied to the host once and compared with the
base copy by copy, Tier B's and C's ids are read with hipMemcpy in the first copy, the last, and the copies around the
boundary; their offsets are compared on the host.  Then, per call, the device's output on the big source is the base's
output tiled (big_cases.Tiled compares on the device, 64 copies at a time), and the base's output is the host twin's,
which tests/test_big_cases_cpu.py holds to the Python checkers, or the oracle's.  Everything but the E-step is integer
work or deterministic and is compared exactly.

The E-step sums the copies' counts with atomics: expected / R and log Z / R are held to the oracle on the base at the
tolerance of tests/test_estep_pairs_gpu.py::test_estep_realistic_corpus (_check_estep there: util.rtol_for of the
longest snippet with ATOL for the counts, 1e-12 relative + 1e-9 for log Z).  Lattice statistics and n-best are
`deterministic` entries of tests/dirty_runs.py, and per row: bit-equal to the base's.

Tier C is built and freed by each of its tests, not held beside A and B; it skips only where the device has less free
memory than big_cases.tier_c_needs (the source and its largest output).

Left out:
  - dropout encode, sampling and fill-in-the-middle: their random draws are keyed by the row index, so the output of
    the big source is not the base's tiled;
  - generate: it takes host arrays and feeds at most 4 GiB per call;
  - the forced kernel paths (TGX_PATH and its kin): the default decision is what a large corpus meets;
  - any host array of a tier's size other than Tier A's text, once, for the content check.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import _lib, synth, tensors

import big_cases as bc
import stats_cases as sx
from test_estep_pairs_gpu import ATOL
from util import rtol_for

POISON = -77
PAD = 7
NO_SPECIALS = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
_HELD = []     # every handle the module builds, for the fixture that frees them


def _torch():
    import torch
    return torch


def _keep(handle):
    _HELD.append(handle)
    return handle


@pytest.fixture(scope="module", autouse=True)
def _free_everything_at_the_end():
    yield
    for cached in (_tier_a, _tier_b, _short, _base, _native, _bytes_native):
        cached.cache_clear()
    while _HELD:
        _HELD.pop().free()
    _torch().cuda.empty_cache()
    _lib.pool_trim()


@functools.lru_cache(maxsize=None)
def _vocab():
    toks, scores, _ = synth.load_spec_vocab(bc.VOCAB)
    return list(toks), np.asarray(scores, np.float64)


@functools.lru_cache(maxsize=None)
def _native():
    return _keep(tgx.NativeModel(*_vocab()))


@functools.lru_cache(maxsize=None)
def _bytes_native():
    """a model of the 256 single bytes: a corpus has one token per byte"""
    return _keep(tgx.NativeModel([bytes([b]) for b in range(256)], np.full(256, -5.0)))


@functools.lru_cache(maxsize=None)
def _oracle():
    return orc.OracleModel(*_vocab())


class _Base:
    pass


@functools.lru_cache(maxsize=None)
def _base():
    """the base on the device, and its ids shown equal to the oracle's"""
    b = _Base()
    b.text, b.offs = bc.base_corpus()
    b.s0 = b.offs.size - 1
    b.corpus = _keep(tgx.NativeCorpus(b.text, b.offs))
    b.result = _keep(_native().encode_corpus(b.corpus))
    b.ids, b.id_offs = _oracle().encode_batch_flat(b.text, b.offs, 0.0, 0, threads=8)
    assert np.array_equal(b.result.ids(), b.ids) and np.array_equal(b.result.offsets(), b.id_offs) and b.ids.size == bc.T0
    for a in (b.ids, b.id_offs):
        a.setflags(write=False)
    return b


def _rows_dev(n0, s0, limit):
    return _torch().from_numpy(bc.big_rows(n0, s0, limit)).cuda()


@functools.lru_cache(maxsize=None)
def _tier_a():
    b = _base()
    return _keep(b.corpus.select(_rows_dev(bc.N0, b.s0, bc.LIMIT_A))), bc.copies(bc.N0, bc.LIMIT_A)


@functools.lru_cache(maxsize=None)
def _tier_b():
    b = _base()
    return _keep(b.result.select(_rows_dev(bc.T0, b.s0, bc.LIMIT_B))), bc.copies(bc.T0, bc.LIMIT_B)


@contextlib.contextmanager
def _tier_c():
    torch = _torch()
    b = _base()
    torch.cuda.empty_cache()
    _lib.pool_trim()
    free = torch.cuda.mem_get_info()[0]
    need = bc.tier_c_needs(b.s0, bc.N_PERM)
    if free < need:
        pytest.skip(f"Tier C needs {need} bytes of device memory, {free} are free")
    res = b.result.select(_rows_dev(bc.T0, b.s0, bc.LIMIT_C))
    try:
        yield res, bc.copies(bc.T0, bc.LIMIT_C)
    finally:
        res.free()
        torch.cuda.empty_cache()
        _lib.pool_trim()


@functools.lru_cache(maxsize=None)
def _short():
    """Tier B without the long rows, R' copies of it: -> (result, keep, ids and offsets of one copy, R')"""
    torch = _torch()
    b = _base()
    big, rb = _tier_b()
    keep, t, r = bc.short_selection(b.id_offs)
    index = ((torch.arange(r, device="cuda") % rb) * b.s0)[:, None] + torch.from_numpy(keep).cuda()[None, :]
    res = _keep(big.select(index.reshape(-1)))
    ids, offs = _lib.select_host(b.ids, b.id_offs, keep)
    assert ids.size == t and r > rb
    return res, keep, ids, offs, r


def _np(t):
    return t.cpu().numpy()


def _ids_slice(res, first, count):
    """ids first .. first + count of a result, read with hipMemcpy"""
    hip_memcpy = _lib.lib.hipMemcpy   # (the runtime libtgx.so is linked against)
    hip_memcpy.restype, hip_memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.full(count, 0xABABABAB, np.uint32)
    assert hip_memcpy(_lib.ptr(host), res.ids_device_ptr() + 4 * first, 4 * count, 2) == 0   # hipMemcpyDeviceToHost
    return host


def _row_hashes_of(data, offs, seed):
    raw = data.tobytes()
    w = data.dtype.itemsize
    return np.array([_lib.row_hash(raw[int(offs[k]) * w:int(offs[k + 1]) * w], seed) for k in range(offs.size - 1)], np.uint64)


def _check_ids_source(res, R, limit):
    b = _base()
    assert res.num_samples == R * b.s0 and res.num_tokens == R * bc.T0 and res.vocab_size == bc.VOCAB
    copy, row, begin, end = bc.straddling_row(b.id_offs, limit)
    assert begin < limit < end and copy + bc.SPARE < R
    for c in (0, copy - 1, copy, copy + 1, R - 1):
        assert np.array_equal(_ids_slice(res, c * bc.T0, bc.T0), b.ids), c
    m = limit % bc.T0
    assert np.array_equal(_ids_slice(res, limit - 3, 6), b.ids[m - 3:m + 3]), "the ids on either side of the boundary"
    offs = res.offsets()
    assert np.array_equal(offs, bc.big_offsets(b.id_offs, R))
    assert int(offs[copy * b.s0 + row]) == begin and int(offs[copy * b.s0 + row + 1]) == end


def _refused(call):
    with pytest.raises(_lib.TokenGeeXError) as e:
        call()
    assert e.value.status == _lib.ERR_UNSUPPORTED, e.value
    return e.value


# ---- Tier A: a resident corpus of more than 2^32 bytes ---------------------------------------------------------------------

def test_tier_a_is_the_base_copy_by_copy():
    b = _base()
    big, R = _tier_a()
    assert big.num_samples == R * b.s0 and big.num_bytes == R * bc.N0 > 2**32
    host = _lib.pinned_empty(R * bc.N0, np.uint8)       # (page-locked: the copy is one DMA transfer)
    _lib.check(_lib.lib.tgx_corpus_copy_text(big._h, _lib.ptr(host), host.size))
    host = host.reshape(R, bc.N0)
    for c in range(0, R, bc.SLAB):
        assert (host[c:c + bc.SLAB] == b.text[None, :]).all(), c
    del host
    offs = big.offsets()
    assert np.array_equal(offs, bc.big_offsets(b.offs, R))
    copy, row, begin, end = bc.straddling_row(b.offs, bc.LIMIT_A)
    assert int(offs[copy * b.s0 + row]) == begin < bc.LIMIT_A < end == int(offs[copy * b.s0 + row + 1]) and end - begin >= 70_000


def test_tier_a_first_equal_and_row_hashes():
    torch = _torch()
    b = _base()
    big, R = _tier_a()
    first, n_unique, _ = _lib.first_equal_host(b.text, b.offs)
    assert np.array_equal(_np(tensors.first_equal(b.corpus)), first)
    got = torch.full((R * b.s0,), POISON, dtype=torch.int64, device="cuda")
    assert big.first_equal(got.data_ptr()) == n_unique
    bc.expect_rows(first, R).check(got, "first_equal")      # first[k] == first_base[k % S0]: the first copy holds every first
    hashes = _row_hashes_of(b.text, b.offs, 5)
    assert np.array_equal(_np(tensors.row_hashes(b.corpus, 5)).view(np.uint64), hashes)
    bc.expect_rows(hashes, R).check(tensors.row_hashes(big, 5), "row_hashes")


def test_tier_a_minhash():
    b = _base()
    big, R = _tier_a()
    sig = _lib.minhash_host(b.text, b.offs, bc.MINHASH_WIDTH, bc.N_PERM, 0)
    assert np.array_equal(_np(tensors.minhash(b.corpus, bc.MINHASH_WIDTH, bc.N_PERM)).view(np.uint32), sig)
    bc.expect_rows(sig, R, axis=0).check(tensors.minhash(big, bc.MINHASH_WIDTH, bc.N_PERM), "minhash")


def _gram_set_of(source, data, offs, kind):
    """the gram set of every 7th row of the base, made on the device; -> (set, the twin's count and mask for the base)"""
    w = bc.GRAM_WIDTH[kind]
    held = source.select(bc.held_out_rows(offs.size - 1))
    try:
        grams = tensors.gram_set(held, w)
    finally:
        held.free()
    keys = _lib.gram_keys_host(*bc.held_out(data, offs), w, 0)
    assert np.array_equal(grams.keys(), keys)
    return grams, _lib.gram_hits_host(data, offs, w, 0, keys)


def test_tier_a_gram_hits_with_the_mask():
    b = _base()
    big, R = _tier_a()
    grams, (count, mask) = _gram_set_of(b.corpus, b.text, b.offs, "bytes")
    try:
        got = tensors.gram_hits(b.corpus, grams, return_mask=True)
        assert np.array_equal(_np(got[0]), count) and np.array_equal(_np(got[1]), mask) and 0 < mask.sum() < mask.size
        got = tensors.gram_hits(big, grams, return_mask=True)
        bc.expect_rows(count, R).check(got[0], "gram count")
        bc.expect_elems(mask, R).check(got[1], "gram mask")
    finally:
        grams.free()


def test_tier_a_text_stats():
    b = _base()
    big, R = _tier_a()
    stats, starts = _lib.text_stats_host(b.text, b.offs, 1000, "char")
    got = tensors.text_stats(b.corpus, "char", 1000, return_line_start=True)
    assert np.array_equal(_np(got.table), stats) and np.array_equal(_np(got.line_start), starts)
    got = tensors.text_stats(big, "char", 1000, return_line_start=True)
    bc.expect_rows(stats, R, axis=1).check(got.table, "text_stats")
    bc.expect_elems(starts, R).check(got.line_start, "line_start")


def test_tier_a_lines():
    """(most of its time is the new corpus's host side: tgx_corpus_lines takes the lines' offsets through the host and
    orders the rows by length there, as every new corpus is, and these are 110 million rows)"""
    torch = _torch()
    b = _base()
    big, R = _tier_a()
    stats, starts = _lib.text_stats_host(b.text, b.offs, 1000, "byte")
    line_offs = _lib.lines_host(b.text, b.offs)
    n_lines = line_offs.size - 1
    assert n_lines == int(starts.sum()) == int(stats[_lib.TEXTSTAT_NAMES.index("lines")].sum())
    small = b.corpus.lines()
    try:
        assert np.array_equal(small.offsets(), line_offs) and np.array_equal(small.bytes(), b.text)
    finally:
        small.free()
    lines = big.lines()
    try:
        assert lines.num_samples == R * n_lines and lines.num_bytes == R * bc.N0
        offs = lines.offsets()
    finally:
        lines.free()
    assert int(offs[-1]) == R * bc.N0
    bc.expect_rows(line_offs[:-1], R, step=bc.N0).check(torch.from_numpy(offs[:-1].view(np.int64)).cuda(), "the lines' offsets")


def test_tier_a_word_stats_with_marks_and_the_stop_table():
    b = _base()
    big, R = _tier_a()
    stats, marks = _lib.word_stats_host(b.text, b.offs, 20, _lib.GOPHER_STOP_WORDS, "char", True)
    got = tensors.word_stats(b.corpus, 20, _lib.GOPHER_STOP_WORDS, "char", True, return_mask=True)
    assert np.array_equal(_np(got.table), stats) and np.array_equal(_np(got.mask), marks)
    assert int(stats[_lib.WORDSTAT_NAMES.index("stop_words")].sum()) > 20 and (marks & _lib.WORD_MARK_STOP).any()
    got = tensors.word_stats(big, 20, _lib.GOPHER_STOP_WORDS, "char", True, return_mask=True)
    bc.expect_rows(stats, R, axis=1).check(got.table, "word_stats")
    bc.expect_elems(marks, R).check(got.mask, "word marks")


def test_tier_a_phrase_hits_with_every_output():
    b = _base()
    big, R = _tier_a()
    phrases = tgx.phrase_set(bc.PHRASES, fold_case=True)
    try:
        count, longest, per = _lib.phrase_hits_host(b.text, b.offs, bc.PHRASES, True, False)
        got = tgx.phrase_hits(b.corpus, phrases, True, True)
        assert all(np.array_equal(_np(g), w) for g, w in zip(got, (count, longest, per))) and (per > 0).all()
        got = tgx.phrase_hits(big, phrases, True, True)
        bc.expect_rows(count, R).check(got[0], "phrase count")
        bc.expect_elems(longest, R).check(got[1], "phrase longest")
        assert np.array_equal(_np(got[2]), R * per)
    finally:
        phrases.free()


@pytest.mark.parametrize("form", ["nfc", "nfkc"])
def test_tier_a_normalize(form):
    b = _base()
    big, R = _tier_a()
    flat, offs, pieces = _lib.normalize_host_twin(form, b.text, b.offs)
    assert pieces > 0 and flat.size != bc.N0
    hashes = _row_hashes_of(flat, offs, 0)
    small = b.corpus.normalize(form)
    try:
        assert np.array_equal(small.bytes(), flat) and np.array_equal(small.offsets(), offs) and small.n_pieces == pieces
    finally:
        small.free()
    out = big.normalize(form)
    try:
        assert out.num_samples == R * b.s0 and out.num_bytes == R * flat.size > 2**32 and out.n_pieces == R * pieces
        bc.expect_rows(hashes, R).check(tensors.row_hashes(out), "row_hashes of the normalised corpus")
        assert np.array_equal(out.offsets(), bc.big_offsets(offs, R))
    finally:
        out.free()


def test_tier_a_split_specials_with_crlf():
    b = _base()
    big, R = _tier_a()
    specials = list(bc.SPECIALS)
    seg_offs, seg_special, flat, offs = _lib.front_host(b.text, b.offs, specials, True)
    n_segments, n_encoded = seg_special.size, offs.size - 1
    assert (seg_special >= 0).sum() > 100 and flat.size < bc.N0 and n_encoded > b.s0, "special tokens were found"
    hashes = _row_hashes_of(flat, offs, 0)
    small, plan = b.corpus.split_specials(specials, True)
    try:
        assert np.array_equal(small.bytes(), flat) and np.array_equal(small.offsets(), offs)
        assert np.array_equal(plan.seg_offs(), seg_offs) and np.array_equal(plan.seg_special(), seg_special)
    finally:
        small.free()
        plan.free()
    out, plan = big.split_specials(specials, True)
    try:
        assert out.num_samples == R * n_encoded and out.num_bytes == R * flat.size
        assert (plan.num_samples, plan.num_segments, plan.num_encoded) == (R * b.s0, R * n_segments, R * n_encoded)
        bc.expect_rows(hashes, R).check(tensors.row_hashes(out), "row_hashes of the segments")
        assert np.array_equal(out.offsets(), bc.big_offsets(offs, R))
        got_offs, got_special = plan._copy()
        assert np.array_equal(got_offs, bc.big_offsets(seg_offs, R))
        bc.expect_rows(seg_special, R).check(_torch().from_numpy(got_special), "seg_special")
    finally:
        out.free()
        plan.free()


def _strided(torch, s0, R):
    mask0 = bc.strided_mask(s0)
    return mask0, torch.from_numpy(mask0).cuda().repeat(R)


def test_tier_a_select_with_a_strided_mask():
    torch = _torch()
    b = _base()
    big, R = _tier_a()
    mask0, mask = _strided(torch, b.s0, R)
    flat, offs = _lib.select_text_host(b.text, b.offs, mask0)
    small = b.corpus.select(mask0)
    try:
        assert np.array_equal(small.bytes(), flat) and np.array_equal(small.offsets(), offs)
    finally:
        small.free()
    out = big.select(mask)
    try:
        assert out.num_samples == R * int(mask0.sum()) and out.num_bytes == R * flat.size
        bc.expect_rows(_row_hashes_of(flat, offs, 0), R).check(tensors.row_hashes(out), "row_hashes of the selection")
        assert np.array_equal(out.offsets(), bc.big_offsets(offs, R))
    finally:
        out.free()


def test_tier_a_encode_corpus():
    torch = _torch()
    b = _base()
    big, R = _tier_a()
    nat = _native()
    hashes = _row_hashes_of(b.ids, b.id_offs, 0)
    assert np.array_equal(_np(tensors.row_hashes(b.result)).view(np.uint64), hashes)
    res = nat.encode_corpus(big)
    try:
        assert res.num_samples == R * b.s0 and res.num_tokens == R * bc.T0 and 4 * res.num_tokens > 2**32
        got = tensors.row_hashes(res)
        bc.expect_rows(hashes, R).check(got, "row_hashes of the encoded corpus")
        assert np.array_equal(res.offsets(), bc.big_offsets(b.id_offs, R))
        tier_b, rb = _tier_b()
        assert rb == R and torch.equal(got, tensors.row_hashes(tier_b)), "the encode of Tier A is Tier B"
    finally:
        res.free()


def _pairs_of(ids, offs, max_pairs):
    """the pair table's head by numpy: the pairs of neighbours within a row, by descending count, then ascending key"""
    inner = np.ones(ids.size, bool)
    inner[offs[1:-1][offs[1:-1] < ids.size].astype(np.int64)] = False   # no pair across a row's beginning
    inner[0] = False
    at = np.flatnonzero(inner)
    keys, counts = np.unique((ids[at - 1].astype(np.uint64) << np.uint64(32)) | ids[at].astype(np.uint64), return_counts=True)
    order = np.lexsort((keys, -counts.astype(np.int64)))[:max_pairs]
    return keys[order], counts[order].astype(np.uint64), keys.size


def test_tier_a_count_tokens_and_the_top_pairs():
    b = _base()
    big, R = _tier_a()
    nat = _native()
    freq = np.bincount(b.ids, minlength=bc.VOCAB).astype(np.uint64)
    assert np.array_equal(nat.count_tokens(b.corpus), freq)
    assert np.array_equal(nat.count_tokens(big), np.uint64(R) * freq)
    keys, counts, total = _pairs_of(b.ids, b.id_offs, 1000)
    got = nat.count_pairs_top(b.corpus, 1000)
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts) and got[2] == total
    got = nat.count_pairs_top(big, 1000)
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], np.uint64(R) * counts) and got[2] == total


def test_tier_a_estep():
    """expected / R and log Z / R against the oracle on the base, at test_estep_realistic_corpus's tolerance"""
    b = _base()
    big, R = _tier_a()
    nat = _native()
    st, want, wz, _ = _oracle().estep_flat(b.text, b.offs, 81920, 0.0, 0, threads=8)
    assert st == orc.OK
    rtol = rtol_for(min(81920, int(np.diff(b.offs.astype(np.int64)).max())))
    got, gz = nat.estep(b.corpus)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=ATOL)
    assert abs(gz - wz) <= 1e-12 * abs(wz) + 1e-9
    got, gz = nat.estep(big)
    got, gz = got / R, gz / R
    print(f"estep on Tier A: max relative distance {float(np.max(np.abs(got - want)[want > 1e-9] / want[want > 1e-9])):.3e} (rtol {rtol:.3e}), "
          f"log Z / R {gz!r} against {wz!r}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=ATOL)
    assert np.array_equal(got != 0, want != 0)
    assert abs(gz - wz) <= 1e-12 * abs(wz) + 1e-9


def test_tier_a_lattice_stats_per_row():
    b = _base()
    big, R = _tier_a()
    nat = _native()
    toks, scores = _vocab()
    twin = _lib.lattice_stats_host(toks, scores, b.text, b.offs, 1.0)
    base = nat.lattice_stats_corpus(b.corpus, 1.0)
    base_kernels = set(nat.last_kernel_times())
    assert base.n_no_path == twin.n_no_path == 0
    # the base against the twin, as tests/test_stats_gpu.py holds a kernel to it: each within its own bound of the truth
    n, rows = np.diff(b.offs.astype(np.int64)).astype(np.float64), "stats_rows_kernel" in base_kernels
    assert np.all(np.abs(base.logz - twin.logz) <= sx.logz_bound(rows, n, twin.logz) + sx.logz_bound(False, n, twin.logz))
    for got, want in ((base.expected_score, twin.expected_score), (base.expected_tokens, twin.expected_tokens)):
        own = sx.ROWS_RTOL * np.maximum(1.0, np.abs(want)) if rows else sx.twin_bound(n, twin.logz, want)
        assert np.all(np.abs(got - want) <= own + sx.twin_bound(n, twin.logz, want))
    st = nat.lattice_stats_corpus(big, 1.0)
    assert set(nat.last_kernel_times()) == base_kernels, "the same kernels ran: a `deterministic` entry of dirty_runs.py, so the same bits"
    assert st.n_no_path == 0 and np.array_equal(st.n_bytes, np.tile(base.n_bytes, R))
    for name in ("logz", "expected_score", "expected_tokens"):
        got = getattr(st, name).view(np.uint64).reshape(R, b.s0)
        assert (got == getattr(base, name).view(np.uint64)[None, :]).all(), name


def test_tier_a_nbest_of_two_per_row():
    torch = _torch()
    b = _base()
    big, R = _tier_a()
    nat = _native()
    toks, _ = _vocab()
    res, scores, found = nat.encode_corpus_nbest(b.corpus, 2)
    try:
        ids, offs = res.ids(), res.offsets()
        base_kernels = set(nat.last_kernel_times())
    finally:
        res.free()
    # the base's rows: the best is the oracle's encode, the second another segmentation of the same bytes with no higher score
    best = np.arange(0, 2 * b.s0, 2)
    assert np.array_equal(_lib.select_host(ids, offs, best)[0], b.ids) and np.array_equal((offs[best + 1] - offs[best]), np.diff(b.id_offs))
    assert (found >= 1).all() and (found == 2).sum() > b.s0 // 2
    lens = np.array([len(t) for t in toks], np.int64)
    n_bytes = np.add.reduceat(np.concatenate([lens[ids], [0]]), np.minimum(offs[:-1].astype(np.int64), ids.size))
    n_bytes[offs[1:] == offs[:-1]] = 0
    second = found == 2
    assert np.array_equal(n_bytes[1::2][second], np.diff(b.offs.astype(np.int64))[second]) and (scores[1::2][second] <= scores[0::2][second]).all()
    assert np.isneginf(scores[1::2][~second]).all() and (n_bytes[1::2][~second] == 0).all()
    hashes = _row_hashes_of(ids, offs, 0)
    res, big_scores, big_found = nat.encode_corpus_nbest(big, 2)
    try:
        assert set(nat.last_kernel_times()) == base_kernels
        assert res.num_samples == 2 * R * b.s0 and res.num_tokens == R * ids.size
        bc.expect_rows(hashes, R).check(tensors.row_hashes(res), "row_hashes of the two best")
        assert np.array_equal(res.offsets(), bc.big_offsets(offs, R))
    finally:
        res.free()
    assert (big_scores.view(np.uint64).reshape(R, -1) == scores.view(np.uint64)[None, :]).all()
    assert (big_found.reshape(R, -1) == found[None, :]).all()


# ---- Tier B: a result whose ids pass byte 2^32 ----------------------------------------------------------------------------

def test_tier_b_is_the_base_result_around_the_boundary():
    res, R = _tier_b()
    assert 4 * res.num_tokens > 2**32 > res.num_tokens
    _check_ids_source(res, R, bc.LIMIT_B)


def _ids_calls(res, R, masks=True):
    """row_lengths, first_equal, row_hashes, minhash, gram_hits and phrase_hits of a result of R copies of the base's"""
    torch = _torch()
    b = _base()
    bc.expect_rows(np.diff(b.id_offs.astype(np.int64)), R).check(tensors.row_lengths(res), "row_lengths")
    first, n_unique, _ = _lib.first_equal_host(b.ids, b.id_offs)
    assert np.array_equal(_np(tensors.first_equal(b.result)), first)
    got = torch.full((R * b.s0,), POISON, dtype=torch.int64, device="cuda")
    assert res.first_equal(got.data_ptr()) == n_unique
    bc.expect_rows(first, R).check(got, "first_equal")
    del got
    hashes = _row_hashes_of(b.ids, b.id_offs, 5)
    assert np.array_equal(_np(tensors.row_hashes(b.result, 5)).view(np.uint64), hashes)
    bc.expect_rows(hashes, R).check(tensors.row_hashes(res, 5), "row_hashes")
    for width in bc.MINHASH_WIDTHS:     # (at width 1 Tier C's shingles pass 2^32)
        sig = _lib.minhash_host(b.ids, b.id_offs, width, bc.N_PERM, 0)
        assert np.array_equal(_np(tensors.minhash(b.result, width, bc.N_PERM)).view(np.uint32), sig)
        bc.expect_rows(sig, R, axis=0).check(tensors.minhash(res, width, bc.N_PERM), f"minhash of width {width}")
    grams, (count, mask) = _gram_set_of(b.result, b.ids, b.id_offs, "ids")
    try:
        got = tensors.gram_hits(b.result, grams, return_mask=True)
        assert np.array_equal(_np(got[0]), count) and np.array_equal(_np(got[1]), mask) and 0 < mask.sum() < mask.size
        got = tensors.gram_hits(res, grams, return_mask=masks)
        bc.expect_rows(count, R).check(got[0] if masks else got, "gram count")
        if masks:
            bc.expect_elems(mask, R).check(got[1], "gram mask")
        del got
    finally:
        grams.free()
    id_phrases = bc.id_phrases(b.ids, b.id_offs)
    phrases = tgx.phrase_set(id_phrases, kind="ids")
    try:
        count, longest, per = _lib.phrase_hits_host(b.ids, b.id_offs, id_phrases)
        got = tgx.phrase_hits(b.result, phrases, True, True)
        assert all(np.array_equal(_np(g), w) for g, w in zip(got, (count, longest, per))) and (per > 0).all()
        if masks:
            got = tgx.phrase_hits(res, phrases, True, True)
            bc.expect_elems(longest, R).check(got[1], "phrase longest")
            assert np.array_equal(_np(got[2]), R * per)
            bc.expect_rows(count, R).check(got[0], "phrase count")
        else:
            bc.expect_rows(count, R).check(tgx.phrase_hits(res, phrases), "phrase count")
    finally:
        phrases.free()


def test_tier_b_rows_hashes_minhash_grams_and_phrases():
    _ids_calls(*_tier_b())


def _check_packed(res, R, with_doc):
    """pack_into without bos and eos as int32: the flat stream is the ids, so the base's stream tiled, and the tail padded"""
    torch = _torch()
    b = _base()
    L = 4096
    T = R * bc.T0
    n_blocks = -(-T // L)
    assert T % L, "the last block has a tail"
    out = torch.full((n_blocks * L,), POISON, dtype=torch.int32, device="cuda")
    doc = torch.full((n_blocks * L,), POISON, dtype=torch.int32, device="cuda") if with_doc else None
    pos = torch.full((n_blocks * L,), POISON, dtype=torch.int32, device="cuda") if with_doc else None
    assert tensors.pack_into(res, out, doc, pos, block_len=L, pad_id=PAD) == n_blocks
    bc.expect_elems(b.ids, R).check(out[:T], "the packed stream")
    assert bool((out[T:] == PAD).all())
    if with_doc:
        want = _lib.layout_pack_host(b.ids, b.id_offs, bc.T0, PAD)     # one block of T0: the base's stream with its rows and positions
        bc.expect_rows(want["doc_ids"].reshape(-1), R, step=b.s0).check(doc[:T], "doc_ids")
        bc.expect_elems(want["positions"].reshape(-1), R).check(pos[:T], "positions")
        assert bool((doc[T:] == -1).all()) and bool((pos[T:] == 0).all())


def test_tier_b_pack_into():
    b = _base()
    want = _lib.layout_pack_host(b.ids, b.id_offs, 4096, PAD)
    got = tensors.to_packed(b.result, 4096, pad_id=PAD, dtype=_torch().int32, return_doc=True)
    assert all(np.array_equal(_np(got[k]), want[k]) for k in want)
    _check_packed(*_tier_b(), with_doc=True)


def test_tier_b_pad_into_and_window_into_without_the_long_row():
    torch = _torch()
    b = _base()
    res, keep, ids, offs, R = _short()
    S = keep.size
    copy, row, begin, end = bc.straddling_row(offs, bc.LIMIT_B)
    assert begin < bc.LIMIT_B < end, "a row of the selection straddles byte 2^32 of its ids"
    assert res.num_samples == R * S and res.num_tokens == R * ids.size > 2**30
    L = bc.PAD_LEN
    assert R * S * L > 2**32, "and the padded ids are more than 2^32 elements"
    want = _lib.layout_pad_host(ids, offs, L, PAD)
    assert 0 < want["n_truncated"] < S
    small = b.result.select(keep)
    try:
        got = tensors.to_padded(small, max_length=L, pad_id=PAD, dtype=torch.int32, return_lengths=True)
        assert all(np.array_equal(_np(got[k]), want[k]) for k in got)
        windows = _lib.layout_windows_host(ids, offs, L, bc.WINDOW_STRIDE, PAD)
        got = tensors.to_windows(small, max_length=L, stride=bc.WINDOW_STRIDE, pad_id=PAD, dtype=torch.int32, return_lengths=True)
        assert all(np.array_equal(_np(got[k]), windows[k]) for k in ("input_ids", "attention_mask", "lengths", "overflow_to_sample_mapping"))
    finally:
        small.free()
    out = torch.full((R * S, L), POISON, dtype=torch.int32, device="cuda")
    mask = torch.full((R * S, L), 9, dtype=torch.uint8, device="cuda")
    lengths = torch.full((R * S,), POISON, dtype=torch.int32, device="cuda")
    assert tensors.pad_into(res, out, mask, lengths, row_len=L, pad_id=PAD) == R * want["n_truncated"]
    bc.expect_rows(want["input_ids"], R, axis=0).check(out, "padded ids")
    bc.expect_rows(want["attention_mask"], R, axis=0).check(mask, "padded mask")
    bc.expect_rows(want["lengths"], R).check(lengths, "padded lengths")
    del out, mask, lengths
    W0 = windows["lengths"].size
    assert res.window_info(L, bc.WINDOW_STRIDE) == R * W0
    out = torch.full((R * W0, L), POISON, dtype=torch.int32, device="cuda")
    mask = torch.full((R * W0, L), 9, dtype=torch.uint8, device="cuda")
    lengths, window_row, window_first = (torch.full((R * W0,), POISON, dtype=torch.int32, device="cuda") for _ in range(3))
    assert tensors.window_into(res, out, mask, lengths, window_row, window_first, row_len=L, stride=bc.WINDOW_STRIDE, pad_id=PAD) == R * W0
    bc.expect_rows(windows["input_ids"], R, axis=0).check(out, "window ids")
    bc.expect_rows(windows["attention_mask"], R, axis=0).check(mask, "window mask")
    bc.expect_rows(windows["lengths"], R).check(lengths, "window lengths")
    bc.expect_rows(windows["overflow_to_sample_mapping"], R, step=S).check(window_row, "window_row")
    bc.expect_rows(windows["window_first"], R).check(window_first, "window_first")


def test_tier_b_spans_into_in_bytes():
    torch = _torch()
    b = _base()
    res, R = _tier_b()
    nat = _native()
    toks, _ = _vocab()
    lens = np.array([len(t) for t in toks], np.int64)[b.ids]
    ends = np.cumsum(lens)
    row = np.repeat(np.arange(b.s0), np.diff(b.id_offs.astype(np.int64)))
    ends -= b.offs.astype(np.int64)[row]                  # a token ends where its row's text has got to
    want = np.stack([ends - lens, ends], axis=1).astype(np.int32)
    got = torch.full((bc.T0, 2), POISON, dtype=torch.int32, device="cuda")
    tensors.spans_into(b.result, nat, got, unit="byte")
    assert np.array_equal(_np(got), want)
    got = torch.full((R * bc.T0, 2), POISON, dtype=torch.int32, device="cuda")
    tensors.spans_into(res, nat, got, unit="byte")
    bc.expect_rows(want, R, axis=0).check(got, "spans")


def test_tier_b_decode_result_is_tier_a():
    torch = _torch()
    b = _base()
    res, R = _tier_b()
    big, ra = _tier_a()
    assert ra == R
    text = _native().decode_result(res, *NO_SPECIALS, True)
    try:
        assert text.num_rows == R * b.s0 and text.num_bytes == R * bc.N0 and text.num_replaced == 0
        corpus = text.to_corpus()
    finally:
        text.free()
    try:
        got = tensors.row_hashes(corpus)
        bc.expect_rows(_row_hashes_of(b.text, b.offs, 0), R).check(got, "row_hashes of the decoded text")
        assert torch.equal(got, tensors.row_hashes(big)) and np.array_equal(corpus.offsets(), bc.big_offsets(b.offs, R))
    finally:
        corpus.free()


def test_tier_b_select_with_a_strided_mask():
    torch = _torch()
    b = _base()
    res, R = _tier_b()
    mask0, mask = _strided(torch, b.s0, R)
    ids, offs = _lib.select_host(b.ids, b.id_offs, mask0)
    small = b.result.select(mask0)
    try:
        assert np.array_equal(small.ids(), ids) and np.array_equal(small.offsets(), offs)
    finally:
        small.free()
    out = res.select(mask)
    try:
        assert out.num_samples == R * int(mask0.sum()) and out.num_tokens == R * ids.size
        bc.expect_rows(_row_hashes_of(ids, offs, 0), R).check(tensors.row_hashes(out), "row_hashes of the selection")
        assert np.array_equal(out.offsets(), bc.big_offsets(offs, R))
        for c in (0, R - 1):
            assert np.array_equal(_ids_slice(out, c * ids.size, ids.size), ids)
    finally:
        out.free()


# ---- Tier C: a result of more than 2^32 ids ---------------------------------------------------------------------------------

def test_tier_c_is_the_base_result_around_the_boundary():
    with _tier_c() as (res, R):
        assert res.num_tokens > 2**32
        _check_ids_source(res, R, bc.LIMIT_C)


def test_tier_c_rows_hashes_minhash_grams_and_phrases():
    with _tier_c() as (res, R):
        _ids_calls(res, R, masks=False)


def test_tier_c_pack_into():
    with _tier_c() as (res, R):
        _check_packed(res, R, with_doc=False)


# ---- what is refused, and that a refusal leaves the outputs and the handles alone ---------------------------------------------

def _check_repeat_stats_refused(source, n_rows, n_elems):
    torch = _torch()
    assert n_elems > bc.REPEAT_MAX_ELEMS
    stats = torch.full((_lib.REPEAT_N, n_rows), POISON, dtype=torch.int64, device="cuda")
    mask = torch.full((n_elems,), 9, dtype=torch.uint8, device="cuda")
    _refused(lambda: source.repeat_stats(3, 0, stats.data_ptr(), mask.data_ptr()))
    assert bool((stats == POISON).all()) and bool((mask == 9).all())


def test_repeat_stats_on_tier_a_is_refused():
    b = _base()
    big, R = _tier_a()
    _check_repeat_stats_refused(big, R * b.s0, R * bc.N0)
    bc.expect_rows(_row_hashes_of(b.text, b.offs, 1), R).check(tensors.row_hashes(big, 1), "the same handle serves the next call")
    small = tensors.repeat_stats(b.corpus, 3, return_mask=True)
    want = _lib.repeat_stats_host(b.text, b.offs, 3)
    assert np.array_equal(_np(small.table), want[0]) and np.array_equal(_np(small.mask), want[1])


def test_repeat_stats_on_tier_c_is_refused():
    b = _base()
    with _tier_c() as (res, R):
        _check_repeat_stats_refused(res, R * b.s0, R * bc.T0)
        bc.expect_rows(_row_hashes_of(b.ids, b.id_offs, 1), R).check(tensors.row_hashes(res, 1), "the same handle serves the next call")


def test_the_frequency_pass_and_the_pair_scan_past_their_token_limits_are_refused():
    """a model of single bytes gives Tier A one token per byte: more than either pass takes"""
    b = _base()
    big, R = _tier_a()
    nat = _bytes_native()
    assert big.num_bytes >= bc.FREQ_REFUSED_TOKENS and big.num_bytes >= bc.PAIRS_REFUSED_TOKENS
    freq = np.full(256, 7, np.uint64)
    _refused(lambda: nat.count_tokens(big, freq))
    assert (freq == 7).all()
    keys, counts, n, total = C.c_void_p(77), C.c_void_p(77), C.c_uint64(77), C.c_uint64(77)
    assert _lib.lib.tgx_count_pairs_top(nat._h, big._h, 10, C.byref(keys), C.byref(counts), C.byref(n), C.byref(total)) == _lib.ERR_UNSUPPORTED
    assert (keys.value, counts.value, n.value, total.value) == (None, None, 0, 0), "no table is handed out"
    assert _lib.lib.tgx_count_pairs(nat._h, big._h, C.byref(keys), C.byref(counts), C.byref(n)) == _lib.ERR_UNSUPPORTED
    assert (keys.value, counts.value, n.value) == (None, None, 0)
    # the same handles serve the next calls
    assert np.array_equal(nat.count_tokens(b.corpus), np.bincount(b.text, minlength=256).astype(np.uint64))
    got = nat.count_pairs_top(b.corpus, 10)
    want = _pairs_of(b.text.astype(np.uint32), b.offs, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    bc.expect_rows(_row_hashes_of(b.text, b.offs, 2), R).check(tensors.row_hashes(big, 2), "Tier A after the refusals")


def test_shuffled_rows_of_2_pow_31_are_refused():
    torch = _torch()
    n = bc.SHUFFLE_REFUSED_ROWS
    assert n == 2**31
    rows = torch.full((n,), POISON, dtype=torch.int64, device="cuda")
    _refused(lambda: _lib.shuffled_rows_device(0, n, 3, rows.data_ptr(), stream=torch.cuda.current_stream().cuda_stream))
    assert bool((rows == POISON).all())
    del rows
    _refused(lambda: tensors.shuffled_rows(n, 3))
    assert np.array_equal(_np(tensors.shuffled_rows(1000, 3)), _lib.shuffled_rows_host(1000, 3))
