"""Shared n-grams on the GPU (tgx_result_gramset_create, tgx_corpus_gramset_create, tgx_gramset_create_from_keys,
tgx_result_gram_hits_device, tgx_corpus_gram_hits_device; csrc/gram.hip) against the independent checker
(tests/gram_checker.py), the host twins and plain tuple membership, on the batches of tests/gram_cases.py for both kinds
(one of them past the cap of the kernels' grid), on key sets that no source would give, and on real text:
test_dedup_gpu.py's corpus under the spec 32 000 vocabulary with slices of held-out rows pasted into training rows.
Everything is compared exactly: this is integer work."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import dedup_checker as dc
import gram_cases
import gram_checker as gc

STAGES = ["gram_keys_kernel", "gram_sort", "gram_dir", "gram_hits_kernel"]
SEED = 0xC0FFEE1234567890


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """a case with the checker's answers: computed once, never changed"""
    c = gram_cases.past_cap_case(kind) if name == "past_cap" else gram_cases.case(name, kind)
    w = c["width"]
    c["keys"] = {seed: gc.keys_of(c["eval_data"], c["eval_offs"], w, seed) for seed in (0, SEED)}
    c["hits"] = {seed: gc.hits(c["data"], c["offs"], w, seed, c["keys"][seed]) for seed in (0, SEED)}
    c["true"] = gc.true_hits(c["data"], c["offs"], w, c["eval_data"], c["eval_offs"])
    for a in (c["data"], c["offs"], c["eval_data"], c["eval_offs"]):
        a.setflags(write=False)
    return c


def _obj(kind, data, offs):
    return _lib.NativeResult.from_ids(data, offs, gram_cases.V) if kind == "ids" else _lib.NativeCorpus(data, offs)


def _read(obj, kind):
    return (obj.ids(), obj.offsets()) if kind == "ids" else (obj.bytes(), obj.offsets())


def _np(t):
    return t.cpu().numpy()


def _check_case(c):
    import torch
    kind, w = c["kind"], c["width"]
    src, ev = _obj(kind, c["data"], c["offs"]), _obj(kind, c["eval_data"], c["eval_offs"])
    try:
        for seed in (0, SEED):
            gs = tgx.gram_set(ev, w, seed)
            assert (gs.size, gs.width, gs.kind, gs.seed, gs.device) == (c["keys"][seed].size, w, kind, seed, 0)
            assert gs.dir_bits == gram_cases.dir_bits(gs.size)
            keys = gs.keys()
            assert np.array_equal(keys, c["keys"][seed]) and np.array_equal(keys, _lib.gram_keys_host(c["eval_data"], c["eval_offs"], w, seed)), seed
            times = _lib.gram_last_times()
            assert list(times) == STAGES and all(t >= 0 for t in times.values())
            assert times["gram_keys_kernel"] > 0 and times["gram_dir"] > 0 and (times["gram_sort"] > 0 or gs.size == 0)
            count, mask = tgx.gram_hits(src, gs, return_mask=True)
            assert count.dtype == torch.int64 and count.shape == (len(c["offs"]) - 1,) and count.device.type == "cuda"
            assert mask.dtype == torch.uint8 and mask.shape == (c["data"].size,)
            want_count, want_mask = c["hits"][seed]
            twin_count, twin_mask = _lib.gram_hits_host(c["data"], c["offs"], w, seed, keys)
            assert np.array_equal(_np(count), want_count) and np.array_equal(_np(mask), want_mask), seed
            assert np.array_equal(_np(count), twin_count) and np.array_equal(_np(mask), twin_mask), seed
            assert np.array_equal(_np(count), c["true"][0]) and np.array_equal(_np(mask), c["true"][1]), seed
            assert (_np(mask)[c["planted"]] == 1).all()
            assert np.array_equal(_np(tgx.gram_hits(src, gs)), want_count), "the counts alone"
            assert _lib.gram_last_times()["gram_hits_kernel"] > 0
            assert np.array_equal(_np(tgx.clean_rows(src, gs)), np.flatnonzero(want_count == 0))
            assert np.array_equal(_np(tgx.clean_rows(src, gs, 1)), np.flatnonzero(want_count <= 1))
            gs.free()
        for obj, data, offs in ((src, c["data"], c["offs"]), (ev, c["eval_data"], c["eval_offs"])):
            got = _read(obj, kind)
            assert np.array_equal(got[0], data) and np.array_equal(got[1], offs), "the inputs are only read"
    finally:
        src.free()
        ev.free()


@pytest.mark.parametrize("name,kind", gram_cases.all_cases())
def test_device_matches_checker_twin_and_truth(name, kind):
    _check_case(_case(name, kind))


@pytest.mark.parametrize("kind", gram_cases.KINDS)
def test_past_the_cap(kind):
    """2048·256 + 2·256 + 70 elements: a block takes two tiles, and in the second a wave gallops from the `hi` of its
    chunk of the first; one row goes from a run's first tile into its second, one from one block's run into the next, so
    that two blocks add to one count; the last working block takes one short tile (tests/test_gram_cpu.py holds the
    batch to this)"""
    _check_case(_case("past_cap", kind))


@pytest.mark.parametrize("name,kind", gram_cases.all_cases())
def test_a_source_against_its_own_set(name, kind):
    c = _case(name, kind)
    w = c["width"]
    src = _obj(kind, c["data"], c["offs"])
    try:
        gs = tgx.gram_set(src, w, SEED)
        assert np.array_equal(gs.keys(), gc.keys_of(c["data"], c["offs"], w, SEED))
        count, mask = tgx.gram_hits(src, gs, return_mask=True)
        lens = np.diff(c["offs"].astype(np.int64))
        assert np.array_equal(_np(count), np.maximum(0, lens - w + 1))
        assert np.array_equal(_np(mask).astype(bool), gc.validity(c["offs"], w))
    finally:
        src.free()


@pytest.mark.parametrize("kind", gram_cases.KINDS)
@pytest.mark.parametrize("name", gram_cases.HOSTILE)
def test_hostile_sets_from_keys(name, kind):
    """a hostile key set, half of a source's own keys and the neighbours of the rest, through from_keys, probed by the source"""
    c = _case("edges_chunk", kind)
    w = c["width"]
    hostile = gram_cases.hostile_keys(name)
    mine = gc.keys_of(c["data"], c["offs"], w, SEED)
    with np.errstate(over="ignore"):
        mixed = np.concatenate([hostile, mine[::2], mine[1::2] + np.uint64(1), mine[1::4] - np.uint64(1)])
    src = _obj(kind, c["data"], c["offs"])
    try:
        for given in (hostile, mixed):
            gs = _lib.NativeGramSet.from_keys(given, w, kind, SEED)
            want = np.unique(given)
            assert np.array_equal(gs.keys(), want) and gs.size == want.size and gs.dir_bits == gram_cases.dir_bits(want.size)
            assert (gs.width, gs.kind, gs.seed) == (w, kind, SEED)
            times = _lib.gram_last_times()
            assert times["gram_keys_kernel"] == 0 and times["gram_dir"] > 0
            count, mask = tgx.gram_hits(src, gs, return_mask=True)
            want_count, want_mask = gc.hits(c["data"], c["offs"], w, SEED, given)
            assert np.array_equal(_np(count), want_count) and np.array_equal(_np(mask), want_mask)
            assert (given is hostile) == (not want_mask.any())
            gs.free()
    finally:
        src.free()


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


def _paste(text, piece):
    """piece into the middle of text, at a space or line end when one is near"""
    at = len(text) // 2
    near = [p for p in (text.find(b" ", at), text.find(b"\n", at)) if 0 <= p < at + 200]
    at = min(near) + 1 if near else at
    return text[:at] + piece + text[at:]


def test_planted_contamination_on_real_text():
    texts = _texts()
    rng = np.random.default_rng(41)
    tk = _tokenizer()
    nat = tk.native_model()
    flat, offs = tgx.pack(texts)
    base = _lib.NativeCorpus(flat, offs)
    res0 = nat.encode_corpus(base)
    ids0, offs0 = res0.ids(), res0.offsets().astype(np.int64)
    res0.free()
    base.free()
    by_len = np.argsort([-len(t) for t in texts], kind="stable")
    big, held = int(by_len[0]), [int(r) for r in by_len[1:11]]      # the 70 000-byte row; ten held-out rows, the longest of the rest
    assert len(texts[big]) == 70_000
    # the eval set: 20 slices of 40 to 200 tokens, two from each held-out row, decoded to their text
    slices = []
    for k in range(20):
        r, half = held[k % 10], k // 10
        n = int(offs0[r + 1] - offs0[r])
        assert n // 2 >= 200
        a = int(offs0[r]) + half * (n // 2) + int(rng.integers(0, n // 2 - 200 + 1))
        slices.append(ids0[a:a + 40 + (k * 37) % 161])
    assert min(s.size for s in slices) == 40 and max(s.size for s in slices) <= 200
    s_offs = np.zeros(21, np.uint64)
    np.cumsum([s.size for s in slices], out=s_offs[1:])
    as_result = _lib.NativeResult.from_ids(np.concatenate(slices), s_offs, 32000)
    dec, dec_offs = tk.decode_result_flat(as_result, False)
    as_result.free()
    pieces = dc.row_bytes(np.asarray(dec, np.uint8), np.asarray(dec_offs, np.uint64))
    print("eval slices: tokens", [s.size for s in slices], "bytes", [len(p) for p in pieces])
    assert min(len(p) for p in pieces) >= 50, "every slice holds a gram of 50 bytes"
    # the training rows: everything but the held-out rows; 12 slices pasted into the middle of rows, the long one among them
    train = [t for r, t in enumerate(texts) if r not in held]
    big_t = big - sum(r < big for r in held)
    others = [r for r, t in enumerate(train) if r != big_t and len(t) >= 200]
    into = [big_t] + [int(r) for r in rng.choice(others, 11, replace=False)]
    for k, r in enumerate(into):
        train[r] = _paste(train[r], pieces[k])
    S = len(train)
    t_flat, t_offs = tgx.pack(train)
    e_flat, e_offs = tgx.pack(pieces)
    corpus, ev_corpus = _lib.NativeCorpus(t_flat, t_offs), _lib.NativeCorpus(e_flat, e_offs)
    res, ev_res = nat.encode_corpus(corpus), nat.encode_corpus(ev_corpus)
    try:
        for src, ev, w, data, o, e_data, e_o in ((res, ev_res, 13, res.ids(), res.offsets(), ev_res.ids(), ev_res.offsets()),
                                               (corpus, ev_corpus, 50, t_flat, t_offs, e_flat, e_offs)):
            grams = tgx.gram_set(ev, w)
            want_keys = gc.keys_of(e_data, e_o, w)
            assert np.array_equal(grams.keys(), want_keys) and grams.size > 0
            want_count, want_mask = gc.hits(data, o, w, 0, want_keys)
            count, mask = tgx.gram_hits(src, grams, return_mask=True)
            assert np.array_equal(_np(count), want_count) and np.array_equal(_np(mask), want_mask), w
            keep = tgx.clean_rows(src, grams)
            want_keep = np.flatnonzero(want_count == 0)
            assert np.array_equal(_np(keep), want_keep), w
            print(f"w = {w}: hits of the pasted rows {want_count[into].tolist()}, rows flagged {S - want_keep.size} of {S}")
            assert (want_count[into] > 0).all() and not set(into) & set(want_keep.tolist()), "every pasted row is flagged"
            assert want_keep.size >= S - 30
            # corpus and result stay aligned under the same rows: the re-encode of the kept text equals the kept ids
            k_corpus, k_res = tgx.select(corpus, keep), tgx.select(res, keep)
            assert dc.row_bytes(k_corpus.bytes(), k_corpus.offsets()) == [train[int(r)] for r in want_keep]
            enc = nat.encode_corpus(k_corpus)
            assert np.array_equal(k_res.ids(), enc.ids()) and np.array_equal(k_res.offsets(), enc.offsets())
            for obj in (enc, k_res, k_corpus, grams):
                obj.free()
    finally:
        for obj in (res, ev_res, corpus, ev_corpus):
            obj.free()


# ---- streams, devices, refusals ---------------------------------------------------------------------------------------------

def test_a_stream_of_the_caller_the_null_stream_and_the_current_device():
    import torch
    cases = (_case("long_among_short", "bytes"), _case("edges_tile", "ids"))
    objs = [(_obj(c["kind"], c["data"], c["offs"]), _obj(c["kind"], c["eval_data"], c["eval_offs"]), c) for c in cases]
    stream = torch.cuda.Stream(device=0)
    other = 1 if torch.cuda.device_count() >= 2 else 0
    try:
        for st in (0, stream.cuda_stream):
            torch.cuda.synchronize()
            with torch.cuda.device(other):     # the objects live on device 0
                before = torch.cuda.current_device()
                for src, ev, c in objs:
                    gs = ev.gram_set(c["width"], SEED, stream=st)
                    count = torch.full((len(c["offs"]) - 1,), -5, dtype=torch.int64, device="cuda:0")
                    mask = torch.full((c["data"].size,), 5, dtype=torch.uint8, device="cuda:0")
                    src.gram_hits(gs, count.data_ptr(), mask.data_ptr(), stream=st)
                    assert torch.cuda.current_device() == before == other
                    assert np.array_equal(gs.keys(), c["keys"][SEED])
                    assert np.array_equal(_np(count), c["hits"][SEED][0]) and np.array_equal(_np(mask), c["hits"][SEED][1])
                    gs.free()
        src, ev, c = objs[0]
        with torch.cuda.stream(stream):        # tensors.* pick up torch's current stream
            gs = tgx.gram_set(ev, c["width"])
            count, mask = tgx.gram_hits(src, gs, return_mask=True)
            keep = tgx.clean_rows(src, gs)
        assert np.array_equal(_np(count), c["hits"][0][0]) and np.array_equal(_np(mask), c["hits"][0][1])
        assert np.array_equal(_np(keep), np.flatnonzero(c["hits"][0][0] == 0))
    finally:
        for src, ev, _ in objs:
            src.free()
            ev.free()


@pytest.mark.parametrize("kind", gram_cases.KINDS)
def test_bad_arguments_are_refused_before_anything_is_queued(kind):
    import torch
    lib = _lib.lib
    c = _case("edges_chunk", kind)
    other_kind = "ids" if kind == "bytes" else "bytes"
    w, w_max = c["width"], gram_cases.W_MAX[kind]
    src, ev = _obj(kind, c["data"], c["offs"]), _obj(kind, c["eval_data"], c["eval_offs"])
    S, N = src.num_samples, c["data"].size
    create = lib.tgx_result_gramset_create if kind == "ids" else lib.tgx_corpus_gramset_create
    hits = lib.tgx_result_gram_hits_device if kind == "ids" else lib.tgx_corpus_gram_hits_device
    gs = tgx.gram_set(ev, w)
    foreign = _lib.NativeGramSet.from_keys(c["keys"][0], 2, other_kind)       # a set of the other element size
    count = torch.full((S,), -5, dtype=torch.int64, device="cuda")
    mask = torch.full((N,), 5, dtype=torch.uint8, device="cuda")
    h_count, h_mask = np.full(S, 9, np.int64), np.full(N, 9, np.uint8)
    p = lambda t: t.data_ptr()
    try:
        out = C.c_void_p(7)
        for bad_w in (0, w_max + 1):
            assert create(ev._h, bad_w, 0, 0, None, C.byref(out)) == _lib.ERR_INVALID and not out.value, bad_w
            assert "width" in lib.tgx_last_error().decode()
        assert create(ev._h, w, 0, 1, None, C.byref(out)) == _lib.ERR_INVALID and not out.value                   # flags
        assert create(None, w, 0, 0, None, C.byref(out)) == _lib.ERR_INVALID and create(ev._h, w, 0, 0, None, None) == _lib.ERR_INVALID
        keys = np.asarray([3, 1, 2], np.uint64)
        for dev, kp, n, bw, eb in ((0, _lib.ptr(keys), 3, 0, 1), (0, _lib.ptr(keys), 3, 65, 1), (0, _lib.ptr(keys), 3, 17, 4), (0, _lib.ptr(keys), 3, 2, 3),
                                   (0, None, 3, 2, 1), (99, _lib.ptr(keys), 3, 2, 1), (-1, _lib.ptr(keys), 3, 2, 1)):
            assert lib.tgx_gramset_create_from_keys(dev, kp, n, bw, eb, 0, C.byref(out)) == _lib.ERR_INVALID and not out.value, (dev, n, bw, eb)
        widest = tgx.gram_set(ev, w_max)                                                                          # the widest is accepted
        assert np.array_equal(widest.keys(), gc.keys_of(c["eval_data"], c["eval_offs"], w_max))
        widest.free()
        # the probe
        assert hits(src._h, foreign._h, 0, None, p(count), p(mask)) == _lib.ERR_INVALID                         # the element size differs
        assert "byte elements" in lib.tgx_last_error().decode()
        assert hits(src._h, gs._h, 0, None, _lib.ptr(h_count), p(mask)) == _lib.ERR_INVALID                      # host memory
        assert "not device memory" in lib.tgx_last_error().decode()
        assert hits(src._h, gs._h, 0, None, p(count), _lib.ptr(h_mask)) == _lib.ERR_INVALID
        assert hits(src._h, gs._h, 1, None, p(count), p(mask)) == _lib.ERR_INVALID                               # flags
        assert hits(src._h, gs._h, 0, None, None, None) == _lib.ERR_INVALID                                      # no output
        assert hits(src._h, None, 0, None, p(count), p(mask)) == _lib.ERR_INVALID
        assert hits(None, gs._h, 0, None, p(count), p(mask)) == _lib.ERR_INVALID
        if torch.cuda.device_count() >= 2:                                                                        # the set's device differs
            far = _lib.NativeGramSet.from_keys(c["keys"][0], w, kind, 0, device=1)
            assert far.device == 1 and hits(src._h, far._h, 0, None, p(count), p(mask)) == _lib.ERR_INVALID
            assert "device" in lib.tgx_last_error().decode()
            there = torch.full((S,), -5, dtype=torch.int64, device="cuda:1")
            assert hits(src._h, gs._h, 0, None, p(there), p(mask)) == _lib.ERR_INVALID                           # an output on another device
            far.free()
        torch.cuda.synchronize()
        assert (_np(count) == -5).all() and (_np(mask) == 5).all() and (h_count == 9).all() and (h_mask == 9).all()   # nothing was written
        assert hits(src._h, gs._h, 0, None, p(count), None) == 0 and (_np(mask) == 5).all()                      # either may be NULL
        assert hits(src._h, gs._h, 0, None, None, p(mask)) == 0
        assert np.array_equal(_np(count), c["hits"][0][0]) and np.array_equal(_np(mask), c["hits"][0][1])
    finally:
        for obj in (src, ev, gs, foreign):
            obj.free()


@pytest.mark.parametrize("kind", gram_cases.KINDS)
def test_no_rows_and_no_grams(kind):
    import torch
    dt = gram_cases.DTYPE[kind]
    c = _case("edges_chunk", kind)
    nothing = _obj(kind, np.zeros(0, dt), np.zeros(1, np.uint64))
    empties = _obj(kind, np.zeros(0, dt), np.zeros(6, np.uint64))
    src = _obj(kind, c["data"], c["offs"])
    full = tgx.gram_set(src, c["width"])
    try:
        for ev in (nothing, empties):
            gs = tgx.gram_set(ev, 5)
            assert gs.size == 0 and gs.dir_bits == 0 and gs.keys().size == 0
            count, mask = tgx.gram_hits(src, gs, return_mask=True)
            assert not _np(count).any() and not _np(mask).any(), "an empty set contains nothing"
            gs.free()
        count, mask = tgx.gram_hits(nothing, full, return_mask=True)
        assert count.shape == (0,) and mask.shape == (0,) and tgx.clean_rows(nothing, full).shape == (0,)
        count = torch.full((5,), -5, dtype=torch.int64, device="cuda")
        empties.gram_hits(full, count.data_ptr(), 0)
        assert _np(count).tolist() == [0] * 5, "rows without elements are never visited and keep the pre-set 0"
        assert _np(tgx.clean_rows(empties, full)).tolist() == [0, 1, 2, 3, 4]
    finally:
        for obj in (nothing, empties, src, full):
            obj.free()
