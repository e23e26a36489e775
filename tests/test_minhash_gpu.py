"""Near-duplicate rows on the GPU (tgx_corpus_minhash_device, tgx_result_minhash_device, tgx_minhash_bands_device,
tgx_minhash_near_first_device; csrc/minhash.hip) against the independent checker (tests/minhash_checker.py) and the
host twins, on the shapes of tests/minhash_cases.py for both kinds (K up to 1024, and one batch past the cap of the
signature kernel's grid), on signatures, chains and heads made with numpy for the calls that take any, and on real text: test_dedup_gpu.py's corpus under
the spec 32 000 vocabulary, a third of its rows repeated exactly and a further set repeated with one token replaced.
Everything is compared exactly: this is integer work."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors

import dedup_checker as dc
import minhash_cases
import minhash_checker as mc

STAGES = ["minhash_sig_kernel", "minhash_band_keys", "minhash_sort", "minhash_heads", "minhash_verify", "minhash_roots"]
SEED = 0xC0FFEE1234567890


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """a case with the checker's answers: computed once, never changed"""
    c = minhash_cases.case(name, kind)
    c["sig"] = {seed: mc.signatures(c["data"], c["offs"], c["width"], c["n_perm"], seed) for seed in (0, SEED)}
    for a in (c["data"], c["offs"], c["sig"][0], c["sig"][SEED]):
        a.setflags(write=False)
    return c


def _source(c):
    if c["kind"] == "ids":
        return _lib.NativeResult.from_ids(c["data"], c["offs"], c["vocab_size"])
    return _lib.NativeCorpus(c["data"], c["offs"])


def _read(obj, kind):
    return (obj.ids(), obj.offsets()) if kind == "ids" else (obj.bytes(), obj.offsets())


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name,kind", minhash_cases.all_cases() + minhash_cases.wide_cases())
def test_device_matches_checker_and_twin(name, kind):
    import torch
    c = _case(name, kind)
    K = c["n_perm"]
    src = _source(c)
    try:
        for seed in (0, SEED):
            sig = tgx.minhash(src, c["width"], K, seed)
            assert sig.dtype == torch.int32 and sig.shape == (len(c["rows"]), K) and sig.device.type == "cuda"
            assert np.array_equal(_u32(sig), c["sig"][seed]), seed
            assert np.array_equal(_u32(sig), _lib.minhash_host(c["data"], c["offs"], c["width"], K, seed)), seed
        times = _lib.minhash_last_times()
        assert list(times) == STAGES and times["minhash_sig_kernel"] > 0 and all(t >= 0 for t in times.values())
        got = _read(src, kind)
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
        sig = tgx.minhash(src, c["width"], K)
        for bands in c["bands"]:
            for seed in (0, SEED):
                keys, heads = tgx.minhash_bands(sig, bands, seed)
                want_keys = mc.band_keys(c["sig"][0], bands, seed)
                want_heads = mc.heads_of(want_keys)
                twin_keys, twin_heads = _lib.minhash_bands_host(c["sig"][0], bands, seed)
                assert keys.dtype == heads.dtype == torch.int64
                assert np.array_equal(_u64(keys), want_keys) and np.array_equal(_u64(keys), twin_keys), (bands, seed)
                assert np.array_equal(heads.cpu().numpy(), want_heads) and np.array_equal(want_heads, twin_heads), (bands, seed)
            for min_agree in sorted({1, (K + 1) // 2, K}):
                first = torch.full((sig.shape[0],), -5, dtype=torch.int64, device=sig.device)
                n_clusters = _lib.minhash_near_first(0, sig.data_ptr(), sig.shape[0], K, heads.data_ptr(), bands, min_agree, first.data_ptr())
                want_first, want_clusters, _ = mc.near_first(c["sig"][0], want_heads, min_agree)
                twin_first, twin_clusters = _lib.minhash_near_first_host(c["sig"][0], want_heads, min_agree)
                assert np.array_equal(first.cpu().numpy(), want_first) and np.array_equal(want_first, twin_first), (bands, min_agree)
                assert n_clusters == want_clusters == twin_clusters, (bands, min_agree)
            assert np.array_equal(_u32(sig), c["sig"][0]), "the signatures are only read"
        times = _lib.minhash_last_times()
        assert list(times) == STAGES and all(t >= 0 for t in times.values())
    finally:
        src.free()


# ---- past the caps of the grids, deep chains, heads from elsewhere ---------------------------------------------------------

def _dev(a):
    """a numpy array (uint32 as its int32 bits) on the device"""
    import torch
    a = np.array(a, order="C")   # (a copy: the cases' arrays are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _near_first(sig, heads, min_agree):
    """tgx_minhash_near_first_device over numpy sig and heads -> (first, n_clusters)"""
    import torch
    d_sig, d_heads = _dev(sig), _dev(heads)
    S, K = sig.shape
    first = torch.full((S,), -5, dtype=torch.int64, device="cuda")
    n_clusters = _lib.minhash_near_first(0, d_sig.data_ptr(), S, K, d_heads.data_ptr(), heads.shape[1], min_agree, first.data_ptr())
    assert np.array_equal(_u32(d_sig), sig) and np.array_equal(d_heads.cpu().numpy(), heads), "the inputs are only read"
    return first.cpu().numpy(), n_clusters


@pytest.mark.parametrize("kind", minhash_cases.KINDS)
def test_past_the_caps_signatures(kind):
    """2048·256 + 2·256 + 70 shingle positions: a block of minhash_sig_kernel takes two tiles, and in the second a wave
    gallops from the `hi` of its chunk of the first; the last working block takes one tile, of which two waves have
    nothing (tests/test_minhash_cpu.py holds the batch to this).  K = 65: two permutations per lane, the second a tail."""
    c = minhash_cases.past_cap_case(kind)
    src = _source(c)
    try:
        for seed in (0, SEED):
            sig = tgx.minhash(src, c["width"], c["n_perm"], seed)
            assert np.array_equal(_u32(sig), mc.signatures(c["data"], c["offs"], c["width"], c["n_perm"], seed)), seed
            assert np.array_equal(_u32(sig), _lib.minhash_host(c["data"], c["offs"], c["width"], c["n_perm"], seed)), seed
        got = _read(src, kind)
        assert np.array_equal(got[0], c["data"]) and np.array_equal(got[1], c["offs"]), "the input is only read"
    finally:
        src.free()


@pytest.mark.parametrize("bands", [1, 2])
def test_past_the_row_caps_bands(bands):
    """256·2048 + 300 rows: minhash_iota_kernel and minhash_heads_kernel go round twice, and with two bands so does
    minhash_band_keys_kernel (a thread per key)"""
    import torch
    sig, _ = minhash_cases.band_rows_sig()
    S, K = sig.shape
    d_sig = _dev(sig)
    want_keys = mc.band_keys_np(sig, bands, 3)
    want_heads = mc.heads_of_np(want_keys)
    twin_keys, twin_heads = _lib.minhash_bands_host(sig, bands, 3)
    keys = torch.full((S, bands), -5, dtype=torch.int64, device="cuda")
    heads = torch.full((S, bands), -5, dtype=torch.int64, device="cuda")
    _lib.minhash_bands(0, d_sig.data_ptr(), S, K, bands, 3, keys.data_ptr(), heads.data_ptr())
    assert np.array_equal(_u64(keys), want_keys) and np.array_equal(_u64(keys), twin_keys)
    assert np.array_equal(heads.cpu().numpy(), want_heads) and np.array_equal(want_heads, twin_heads)
    assert np.array_equal(_u32(d_sig), sig), "the signatures are only read"
    t_keys, t_heads = tgx.minhash_bands(d_sig, bands, 3)
    assert np.array_equal(_u64(t_keys), want_keys) and np.array_equal(t_heads.cpu().numpy(), want_heads)


def test_past_the_verify_cap_near_first():
    """4·16384 + 300 rows of K = 65: minhash_verify_kernel (a wave per row, four to a block, 16384 blocks) goes round twice;
    13 bands, min_agree 40"""
    sig = minhash_cases.verify_rows_sig()
    heads = mc.heads_of_np(mc.band_keys_np(sig, 13))
    want_first, want_clusters, _ = mc.near_first_memo(sig, heads, 40)
    twin_first, twin_clusters = _lib.minhash_near_first_host(sig, heads, 40)
    first, n_clusters = _near_first(sig, heads, 40)
    assert np.array_equal(first, want_first) and np.array_equal(first, twin_first)
    assert n_clusters == want_clusters == twin_clusters
    keys, d_heads = tgx.minhash_bands(_dev(sig), 13)
    assert np.array_equal(d_heads.cpu().numpy(), heads)


@pytest.mark.parametrize("S", minhash_cases.CHAIN_SIZES)
def test_one_chain_of_every_row(S):
    """first0[i] = i - 1: a chain as deep as there are rows, so every round of the pointer doubling does work; the
    expected answer is the construction's"""
    sig, heads, want_first, want_clusters, min_agree = minhash_cases.chain_case(S)
    first, n_clusters = _near_first(sig, heads, min_agree)
    twin_first, twin_clusters = _lib.minhash_near_first_host(sig, heads, min_agree)
    assert np.array_equal(first, want_first) and np.array_equal(twin_first, want_first)
    assert n_clusters == want_clusters == twin_clusters == 1


def test_a_forest_of_chains():
    sig, heads, want_first, want_clusters, min_agree = minhash_cases.forest_case()
    first, n_clusters = _near_first(sig, heads, min_agree)
    twin_first, twin_clusters = _lib.minhash_near_first_host(sig, heads, min_agree)
    assert np.array_equal(first, want_first) and np.array_equal(twin_first, want_first)
    assert n_clusters == want_clusters == twin_clusters


def test_heads_from_elsewhere_are_never_followed():
    """entries of heads overwritten with i, i + 1, S, 2^40, -1 and INT64_MIN give what the same entries set to i give"""
    c = _case("contents", "ids")
    sig = np.asarray(c["sig"][0])
    wild, tame = minhash_cases.heads_from_elsewhere(mc.heads_of(mc.band_keys(sig, 32)))
    for min_agree in (1, 64, 128):
        want_first, want_clusters, _ = mc.near_first_memo(sig, tame, min_agree)
        for heads in (tame, wild):
            first, n_clusters = _near_first(sig, heads, min_agree)
            assert np.array_equal(first, want_first) and n_clusters == want_clusters, min_agree


# ---- real text --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _texts():
    """test_dedup_gpu.py's corpus: ~96 KiB of mixed text in samples of up to 4 KiB, one sample of 70 000 bytes, and empty
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


def test_near_unique_rows_keep_corpus_and_result_aligned_on_real_text():
    import torch
    texts = _texts()
    S = len(texts)
    rng = np.random.default_rng(33)
    again = rng.choice(S, S // 3, replace=False)
    again[:2] = (int(np.argmax([len(t) for t in texts])), S - 1)      # the 70 000-byte sample and an empty one are among the repeated
    flat, offs = tgx.pack(texts)
    tk = _tokenizer()
    nat = tk.native_model()
    base = _lib.NativeCorpus(flat, offs)
    res0 = nat.encode_corpus(base)
    ids0, offs0 = res0.ids(), res0.offsets()
    res0.free()
    n_tok = np.diff(offs0.astype(np.int64))
    long_rows = np.flatnonzero(n_tok >= 200)
    assert long_rows.size >= 4
    perturbed = rng.choice(long_rows, min(12, long_rows.size), replace=False)
    index = np.concatenate([np.arange(S), again, perturbed])
    order = rng.permutation(index.size)
    index = index[order].astype(np.int64)
    is_perturbed = (order >= S + again.size)
    corpus0 = tgx.select(base, torch.from_numpy(index).cuda())
    base.free()
    # one token replaced in the middle of every perturbed copy: decode the row's ids with one id swapped, so that the text
    # changes with it and the re-encode is checked on the real thing
    rows = dc.row_bytes(corpus0.bytes(), corpus0.offsets())
    corpus0.free()
    for k in np.flatnonzero(is_perturbed):
        r = int(index[k])
        ids = ids0[int(offs0[r]):int(offs0[r + 1])].copy()
        at = ids.size // 2
        ids[at] = ids[at - 1] if ids[at] != ids[at - 1] else ids[at + 1]
        one = _lib.NativeResult.from_ids(ids, np.asarray([0, ids.size], np.uint64), 32000)
        dec, _ = tk.decode_result_flat(one, False)
        one.free()
        rows[k] = bytes(np.asarray(dec, np.uint8))
    flat, offs = tgx.pack(rows)
    corpus = _lib.NativeCorpus(flat, offs)
    res = nat.encode_corpus(corpus)
    try:
        d_ids, d_offs = res.ids(), res.offsets()
        sig = tgx.minhash(res, 5, 128)
        want_sig = mc.signatures(d_ids, d_offs, 5, 128)
        assert np.array_equal(_u32(sig), want_sig)
        want_heads = mc.heads_of(mc.band_keys(want_sig, 32))
        want_first, want_clusters, _ = mc.near_first(want_sig, want_heads, 90)      # ceil(0.7 · 128)
        first = tgx.near_first(sig, 32, 0.7)
        assert first.dtype == torch.int64 and np.array_equal(first.cpu().numpy(), want_first)
        first_eq, _ = dc.first_equal(d_ids, d_offs)
        assert (first_eq != np.arange(index.size)).sum() >= S // 3
        assert np.array_equal(want_first[first_eq], want_first), "the exact copies share a cluster with their originals"
        # agree / K of the perturbed rows against their originals, beside the true Jaccard similarity (printed: a report)
        id_rows = mc.rows_of(d_ids, d_offs)
        for k in np.flatnonzero(is_perturbed):
            o = int(np.flatnonzero((index == index[k]) & ~is_perturbed)[0])     # a copy of the row it was made from
            assert want_first[k] == want_first[o], "a row with one token replaced joins the cluster of the row it was made from"
            print(f"row {k}: agree/K = {int((want_sig[k] == want_sig[o]).sum()) / 128:.3f}, J = {mc.jaccard(id_rows[k], id_rows[o], 5):.3f}")
        keep = tgx.near_unique_rows(sig, 32, 0.7)
        want_keep = np.flatnonzero(want_first == np.arange(index.size))
        assert np.array_equal(keep.cpu().numpy(), want_keep) and keep.numel() == want_clusters < index.size - S // 3 + 1
        u_corpus, u_res = tgx.select(corpus, keep), tgx.select(res, keep)
        assert dc.row_bytes(u_corpus.bytes(), u_corpus.offsets()) == [rows[int(k)] for k in want_keep]
        enc = nat.encode_corpus(u_corpus)
        assert np.array_equal(u_res.ids(), enc.ids()) and np.array_equal(u_res.offsets(), enc.offsets())
        for o in (enc, u_res, u_corpus):
            o.free()
        # the same on the text: shingles of 32 bytes
        sig_b = tgx.minhash(corpus, 32, 64)
        assert np.array_equal(_u32(sig_b), _lib.minhash_host(flat, offs, 32, 64))
    finally:
        res.free()
        corpus.free()


def test_a_stream_of_the_caller_the_null_stream_and_the_current_device():
    import torch
    c = _case("contents", "bytes")
    r = _case("edges_chunk", "ids")
    corpus, res = _source(c), _source(r)
    stream = torch.cuda.Stream(device=corpus.device)
    other = 1 if torch.cuda.device_count() >= 2 else 0
    want = {}
    for cc in (c, r):
        heads = mc.heads_of(mc.band_keys(cc["sig"][0], 32))
        want[cc["kind"]] = (heads, mc.near_first(cc["sig"][0], heads, 64))
    try:
        for st in (0, stream.cuda_stream):
            torch.cuda.synchronize()
            with torch.cuda.device(other):     # the objects live on device 0
                before = torch.cuda.current_device()
                for src, cc in ((corpus, c), (res, r)):
                    S, K = len(cc["rows"]), cc["n_perm"]
                    sig = torch.full((S, K), -5, dtype=torch.int32, device="cuda:0")
                    heads = torch.full((S, 32), -5, dtype=torch.int64, device="cuda:0")
                    first = torch.full((S,), -5, dtype=torch.int64, device="cuda:0")
                    src.minhash(sig.data_ptr(), cc["width"], K, 0, stream=st)
                    _lib.minhash_bands(0, sig.data_ptr(), S, K, 32, 0, 0, heads.data_ptr(), stream=st)
                    n_clusters = _lib.minhash_near_first(0, sig.data_ptr(), S, K, heads.data_ptr(), 32, 64, first.data_ptr(), stream=st)
                    assert torch.cuda.current_device() == before == other
                    w_heads, (w_first, w_clusters, _) = want[cc["kind"]]
                    assert np.array_equal(_u32(sig), cc["sig"][0]) and np.array_equal(heads.cpu().numpy(), w_heads)
                    assert np.array_equal(first.cpu().numpy(), w_first) and n_clusters == w_clusters
        with torch.cuda.stream(stream):        # tensors.* pick up torch's current stream
            sig = tgx.minhash(corpus, c["width"], c["n_perm"])
            first = tgx.near_first(sig, 32, 0.5)
        assert np.array_equal(_u32(sig), c["sig"][0]) and np.array_equal(first.cpu().numpy(), want["bytes"][1][0])
    finally:
        corpus.free()
        res.free()


@pytest.mark.parametrize("kind", minhash_cases.KINDS)
def test_bad_arguments_are_refused_before_anything_is_queued(kind):
    import torch
    lib = _lib.lib
    c = _case("contents", kind)
    src = _source(c)
    S, K = src.num_samples, c["n_perm"]
    fn = lib.tgx_result_minhash_device if kind == "ids" else lib.tgx_corpus_minhash_device
    w_max = minhash_cases.W_MAX[kind]
    host = np.full((S, K), 9, np.uint32)
    dev = torch.full((S, K), -5, dtype=torch.int32, device="cuda")
    try:
        assert fn(src._h, 5, K, 0, 0, None, _lib.ptr(host)) == _lib.ERR_INVALID                 # host memory
        assert "not device memory" in lib.tgx_last_error().decode() and (host == 9).all()
        assert fn(src._h, 5, K, 0, 0, None, None) == _lib.ERR_INVALID                            # NULL with S > 0
        assert fn(src._h, 5, K, 0, 1, None, dev.data_ptr()) == _lib.ERR_INVALID                  # flags
        assert fn(None, 5, K, 0, 0, None, dev.data_ptr()) == _lib.ERR_INVALID
        for w, k in ((0, K), (w_max + 1, K), (5, 0), (5, 1025)):
            assert fn(src._h, w, k, 0, 0, None, dev.data_ptr()) == _lib.ERR_INVALID, (w, k)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == -5).all()                                                   # nothing was written
        assert fn(src._h, w_max, K, 0, 0, None, dev.data_ptr()) == 0                             # the widest is accepted
        assert np.array_equal(_u32(dev), mc.signatures(c["data"], c["offs"], w_max, K))
        # the calls on signatures
        sig = tgx.minhash(src, c["width"], K)
        B = 32
        keys = torch.full((S, B), -5, dtype=torch.int64, device="cuda")
        heads = torch.full((S, B), -5, dtype=torch.int64, device="cuda")
        first = torch.full((S,), -5, dtype=torch.int64, device="cuda")
        h_keys, h_heads, h_first, h_sig = np.full((S, B), 9, np.uint64), np.full((S, B), 9, np.int64), np.full(S, 9, np.int64), _u32(sig).copy()
        bands, near = lib.tgx_minhash_bands_device, lib.tgx_minhash_near_first_device
        nc = C.c_uint64(77)
        p = lambda t: t.data_ptr()
        assert bands(0, p(sig), S, K, B, 0, None, _lib.ptr(h_keys), p(heads)) == _lib.ERR_INVALID
        assert bands(0, p(sig), S, K, B, 0, None, p(keys), _lib.ptr(h_heads)) == _lib.ERR_INVALID
        assert bands(0, _lib.ptr(h_sig), S, K, B, 0, None, p(keys), p(heads)) == _lib.ERR_INVALID
        assert bands(0, None, S, K, B, 0, None, p(keys), p(heads)) == _lib.ERR_INVALID
        assert bands(0, p(sig), S, K, B, 0, None, None, None) == _lib.ERR_INVALID
        for bad in (0, 3, K + 1):
            assert bands(0, p(sig), S, K, bad, 0, None, p(keys), p(heads)) == _lib.ERR_INVALID, bad
        assert bands(0, p(sig), S, 0, B, 0, None, p(keys), p(heads)) == _lib.ERR_INVALID
        assert bands(99, p(sig), S, K, B, 0, None, p(keys), p(heads)) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert (keys.cpu().numpy() == -5).all() and (heads.cpu().numpy() == -5).all() and (h_keys == 9).all() and (h_heads == 9).all()
        assert bands(0, p(sig), S, K, B, 0, None, p(keys), None) == 0 and (heads.cpu().numpy() == -5).all()      # either may be NULL
        assert bands(0, p(sig), S, K, B, 0, None, None, p(heads)) == 0
        assert np.array_equal(heads.cpu().numpy(), mc.heads_of(_u64(keys)))
        for bad in (0, K + 1):
            assert near(0, p(sig), S, K, p(heads), B, bad, None, p(first), C.byref(nc)) == _lib.ERR_INVALID, bad
            assert "min_agree" in lib.tgx_last_error().decode()
        assert near(0, p(sig), S, K, None, B, 64, None, p(first), C.byref(nc)) == _lib.ERR_INVALID
        assert near(0, p(sig), S, K, p(heads), B, 64, None, None, C.byref(nc)) == _lib.ERR_INVALID
        assert near(0, p(sig), S, K, p(heads), B, 64, None, _lib.ptr(h_first), C.byref(nc)) == _lib.ERR_INVALID
        assert near(0, p(sig), S, K, _lib.ptr(h_heads), B, 64, None, p(first), C.byref(nc)) == _lib.ERR_INVALID
        assert near(0, p(sig), S, K, p(heads), 0, 64, None, p(first), C.byref(nc)) == _lib.ERR_INVALID
        torch.cuda.synchronize()
        assert (first.cpu().numpy() == -5).all() and (h_first == 9).all()
        assert near(0, p(sig), S, K, p(heads), B, 64, None, p(first), None) == 0                                  # n_clusters may be NULL
        assert np.array_equal(first.cpu().numpy(), mc.near_first(c["sig"][0], heads.cpu().numpy(), 64)[0])
    finally:
        src.free()


@pytest.mark.parametrize("kind", minhash_cases.KINDS)
def test_no_rows_and_rows_that_are_all_empty(kind):
    import torch
    dt = np.uint32 if kind == "ids" else np.uint8
    src = _source(dict(kind=kind, data=np.zeros(0, dt), offs=np.zeros(1, np.uint64), vocab_size=10))
    try:
        src.minhash(0)
        sig = tgx.minhash(src)
        assert sig.shape == (0, 128)
        keys, heads = tgx.minhash_bands(sig, 32)
        assert keys.shape == heads.shape == (0, 32)
        assert tgx.near_first(sig, 32, 0.7).shape == (0,) and tgx.near_unique_rows(sig, 32, 0.7).shape == (0,)
    finally:
        src.free()
    # rows, but none with an element: one shingle each, the empty one, and one cluster
    src = _source(dict(kind=kind, data=np.zeros(0, dt), offs=np.zeros(6, np.uint64), vocab_size=10))
    try:
        sig = tgx.minhash(src, 5, 65)
        want = mc.signatures(np.zeros(0, dt), np.zeros(6, np.uint64), 5, 65)
        assert np.array_equal(_u32(sig), want) and (want == want[0]).all()
        assert tgx.near_first(sig, 13, 1.0).tolist() == [0] * 5 and tgx.near_unique_rows(sig, 13, 1.0).tolist() == [0]
    finally:
        src.free()
