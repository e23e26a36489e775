"""Passes of different kinds and different models in hostile orders on handles that stay alive.

A resident corpus keeps its scratch (back-pointers, the right-aligned ids, counts, status, the scan's room, the E-step's
work list) across passes, and a model its control words and its lazily built tables; nothing clears them between
passes.  Here ONE corpus (dirty_runs.pass_texts: about a hundred samples, empty ones, the trips of three and four
positions per lane, two above a lowered TGX_LONG_THRESHOLD) serves three models — A, tokens of at most 16 bytes; B, tokens
of 17 .. 32 bytes; C, which lacks a byte of one sample, so that its encode, sampling and n-best passes fail with the
oracle's no-path report after having written into the corpus's scratch — through twelve steps in three orders: as
listed, reversed, and one permutation from a fixed seed.  Every step's expectation is computed once, on fresh handles
with the pool as it is, and checked there against its reference exactly as in tests/dirty_runs.py; every step in every
order must then equal it: bit for bit, or through the E-step's gate for the atomically summed counts.  Once with the pool
as it is and once with every pooled buffer filled with 0xFF (TGX_POOL_FILL=255).

The same in small for the calls on a caller's stream: one result and one corpus through select, first_equal, minhash,
gram_hits, repeat_stats, text_stats, the padded layout and decode, forwards and backwards, with a failing call (a select
with an out-of-range row in device memory) between every two; the calls after a failure answer as on fresh handles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import dirty_runs as dr

KNOB = "TGX_POOL_FILL"
LT = {"TGX_LONG_THRESHOLD": str(dr.LONG_THRESHOLD)}
SNIPPET_2 = 900   # the second snippet length: the corpus's E-step work list is rebuilt


class Handles:
    def __init__(self):
        self.corpus = tgx.NativeCorpus(*dr.pass_batch())
        self.A, self.B, self.C = dr.native_of("A", for_estep=True), dr.native_of("B"), dr.native_of("C")

    def free(self):
        for h in (self.A, self.B, self.C, self.corpus):
            h.free()


def _refused(call):
    """the refusal of a pass as outputs"""
    with pytest.raises(tgx.TokenGeeXError) as e:
        call()
    return {"error": np.array([e.value.status, e.value.sample], np.int64), "_message": str(e.value)}


def _failing_c(h):
    out = {}
    for key, call in (("encode/", lambda: h.C.encode_corpus(h.corpus)), ("sample/", lambda: h.C.encode_corpus_sample(h.corpus, 0.5, 3)),
                      ("nbest/", lambda: h.C.encode_corpus_nbest(h.corpus, 4))):
        out.update({key + k: v for k, v in _refused(call).items()})
    return out


def _check_failing_c(out):
    want = dr.oracle_encode("C")
    assert isinstance(want, dr.orc.NoPath)
    for key in ("encode/", "sample/", "nbest/"):
        assert out[key + "error"].tolist() == [_lib.ERR_NO_PATH, want.sample] and out[key + "_message"] == str(want), key


def _rows4_then_in_place(h, monkeypatch):
    """rows4 writes its ids through the corpus's d_tmp; rows5 in place after it does not"""
    monkeypatch.setenv("TGX_PATH", "rows4")
    a = dr.run_encode(h.A, h.corpus)
    monkeypatch.setenv("TGX_PATH", "rows5")
    monkeypatch.setenv("TGX_LONG_THRESHOLD", "0")
    b = dr.run_encode(h.A, h.corpus)
    assert not a["_flags"]["in_place"] and b["_flags"]["in_place"], (a["_flags"], b["_flags"])
    return {"rows4_ids": a["ids"], "rows4_offs": a["offs"], "ids": b["ids"], "offs": b["offs"]}


def _check_two_encodes(out):
    dr.check_encode(out, "A")
    dr.check_encode({"ids": out["rows4_ids"], "offs": out["rows4_offs"]}, "A")


def _estep(model, env, snippet_len, kernels, dropout=0.0, seed=0):
    def run(h, monkeypatch):
        return dr._estep_out(h.A, h.corpus, snippet_len, dropout, seed)

    def check(out):
        dr.check_estep(out, dr.oracle_of(model), snippet_len, dropout, seed, kernels)

    return env, run, check


# name -> (env, run(handles, monkeypatch), check(outputs))
STEPS = {
    "encode A": (LT, lambda h, mp: dr.run_encode(h.A, h.corpus), lambda out: dr.check_encode(out, "A")),
    "encode A with dropout": (LT, lambda h, mp: dr.run_encode(h.A, h.corpus, 0.2, 7), lambda out: dr.check_encode(out, "A", 0.2, 7)),
    "encode A rows4, then rows5 in place": ({}, _rows4_then_in_place, _check_two_encodes),
    "encode B": (LT, lambda h, mp: dr.run_encode(h.B, h.corpus), lambda out: dr.check_encode(out, "B")),
    "the failing passes of C": ({}, lambda h, mp: _failing_c(h), _check_failing_c),
    "sample A": ({}, lambda h, mp: dr.run_sample(h.A, h.corpus), lambda out: dr.check_sample(out, "A")),
    "n-best A": ({}, lambda h, mp: dr.run_nbest(h.A, h.corpus), lambda out: dr.check_nbest(out, "A", dr.NBEST_K)),
    "lattice statistics A": ({"TGX_STATS_PATH": "rows"}, lambda h, mp: dr.run_stats(h.A, h.corpus), lambda out: dr.check_stats(out, "A", dr.STATS_ALPHA, True)),
    "E-step A, estep7": _estep("A", {}, 81920, ("estep7_kernel",)),
    "E-step A, chained": _estep("A", {"TGX_ESTEP": "chain"}, 81920, ("estep4l_bwd_kernel",)),
    "counts A": ({}, lambda h, mp: dr.run_counts(h.A, h.corpus, 50), lambda out: dr.check_counts(out, "A", 50)),
    "E-step A, a second snippet length": _estep("A", {}, SNIPPET_2, ("estep7_kernel",), 0.1, 5),
}
ORDERS = {"as listed": list(STEPS), "reversed": list(STEPS)[::-1],
          "permuted": [list(STEPS)[i] for i in np.random.default_rng(20240611).permutation(len(STEPS))]}


def _run_step(name, h, monkeypatch):
    env, run, _ = STEPS[name]
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return run(h, mp)


@pytest.fixture(scope="module")
def expected():
    """every step on fresh handles, checked against its reference: computed once, never changed"""
    mp = pytest.MonkeyPatch()
    mp.delenv(KNOB, raising=False)
    want = {}
    try:
        for name, (_, _, check) in STEPS.items():
            h = Handles()
            try:
                want[name] = _run_step(name, h, mp)
            finally:
                h.free()
            check(want[name])
    finally:
        mp.undo()
    return want


def _same_as_fresh(name, got, want):
    check = STEPS[name][2]
    for k in want:
        if k.startswith("_") or k.endswith("/_message"):
            continue
        if k in dr.SUMMED:
            continue   # (through the gate below)
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
    check(got)


@pytest.mark.parametrize("fill", [None, "255"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_every_step_in_every_order_equals_its_fresh_handle_expectation(monkeypatch, expected, order, fill):
    assert sorted(ORDERS[order]) == sorted(STEPS) and ORDERS["permuted"] not in (ORDERS["as listed"], ORDERS["reversed"])
    if fill is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, fill)
    before = _lib.pool_filled_bytes()
    h = Handles()
    try:
        for name in ORDERS[order]:
            _same_as_fresh(name, _run_step(name, h, monkeypatch), expected[name])
    finally:
        h.free()
    assert (_lib.pool_filled_bytes() > before) == (fill is not None)


# ---- the calls on a caller's stream ---------------------------------------------------------------------------------------
W, K_PERM = 5, 16
EVAL_ROWS = list(range(12, 24))
PICK = [3, 0, 40, 40, 12, 99, 1, 57]


class Sources:
    """one result (the oracle's ids of the corpus under A), one corpus, a model for decode, a gram set of each kind"""

    def __init__(self):
        ids, offs = dr.oracle_encode("A")
        self.model = dr.native_of("A")
        self.obj = {"ids": _lib.NativeResult.from_ids(ids, offs, len(dr.vocab("A")[0])), "bytes": tgx.NativeCorpus(*dr.pass_batch())}
        self.grams = {}
        for kind, src in self.obj.items():
            ev = src.select(EVAL_ROWS)
            self.grams[kind] = ev.gram_set(W, dr.SEED)
            ev.free()

    def free(self):
        for h in list(self.grams.values()) + list(self.obj.values()) + [self.model]:
            h.free()


def _data(kind):
    return dr.oracle_encode("A") if kind == "ids" else dr.pass_batch()


def _both(fn):
    """a call of both kinds -> outputs keyed by kind"""
    def run(s, ctx):
        out = {}
        for kind in ("ids", "bytes"):
            out.update({f"{kind}/{k}": v for k, v in fn(s.obj[kind], kind, s, ctx).items()})
        return out
    return run


def _select(src, kind, s, ctx):
    got = src.select(ctx.dev(np.asarray(PICK, np.int64)), stream=ctx.stream)
    out = {"data": got.ids() if kind == "ids" else got.bytes(), "offs": got.offsets()}
    got.free()
    return out


def _first_equal(src, kind, s, ctx):
    first = ctx.full((src.num_samples,), "int64", -5)
    return {"unique": np.array([src.first_equal(first.data_ptr(), stream=ctx.stream)]), "first": dr._np(first)}


def _minhash(src, kind, s, ctx):
    sig = ctx.full((src.num_samples, K_PERM), "int32", dr.POISON)
    src.minhash(sig.data_ptr(), W, K_PERM, dr.SEED, stream=ctx.stream)
    return {"sig": dr._np(sig).view(np.uint32)}


def _gram_hits(src, kind, s, ctx):
    count, mask = ctx.full((src.num_samples,), "int64", -7), ctx.full((_data(kind)[0].size,), "uint8", 7)
    src.gram_hits(s.grams[kind], count.data_ptr(), mask.data_ptr(), stream=ctx.stream)
    return {"count": dr._np(count), "mask": dr._np(mask)}


def _repeat_stats(src, kind, s, ctx):
    stats = ctx.full((6, src.num_samples), "int64", -7)   # (no mask: the flag array is pooled scratch)
    src.repeat_stats(W, dr.SEED, stats.data_ptr(), 0, stream=ctx.stream)
    return {"stats": dr._np(stats)}


def _text_stats(s, ctx):
    corpus = s.obj["bytes"]
    table, marks = ctx.full((11, corpus.num_samples), "int64", -7), ctx.full((corpus.num_bytes,), "uint8", 7)
    corpus.text_stats(table.data_ptr(), marks.data_ptr(), 40, "char", stream=ctx.stream)
    return {"table": dr._np(table), "marks": dr._np(marks)}


PAD_L = 48


def _to_padded(s, ctx):
    res = s.obj["ids"]
    S = res.num_samples
    ids, mask, ln = ctx.full((S, PAD_L), "int32", dr.POISON), ctx.full((S, PAD_L), "uint8", 9), ctx.full((S,), "int32", dr.POISON)
    nt = res.pad_device(PAD_L, dr.PAD, ids.data_ptr(), mask_ptr=mask.data_ptr(), lengths_ptr=ln.data_ptr(), bos_id=1, stream=ctx.stream)
    return {"ids": dr._np(ids), "mask": dr._np(mask), "lengths": dr._np(ln), "truncated": np.array([nt])}


def _decode(s, ctx):
    out = {}
    dr._take_text(s.model.decode_result(s.obj["ids"], np.zeros(0, np.uint8), np.zeros(1, np.uint64), True, stream=ctx.stream), out)
    return out


def _check_select(out):
    import select_checker
    for kind in ("ids", "bytes"):
        d, o = select_checker.select(*_data(kind), np.asarray(PICK, np.int64))
        dr._eq(out[f"{kind}/offs"], o, kind)
        dr._eq(out[f"{kind}/data"], d, kind)


def _check_first_equal(out):
    import dedup_checker
    for kind in ("ids", "bytes"):
        first, unique = dr._ref(("seq first", kind), lambda: dedup_checker.first_equal(*_data(kind)))
        dr._eq(out[f"{kind}/first"], first, kind)
        assert int(out[f"{kind}/unique"][0]) == unique


def _check_minhash(out):
    import minhash_checker
    for kind in ("ids", "bytes"):
        dr._eq(out[f"{kind}/sig"], dr._ref(("seq sig", kind), lambda: minhash_checker.signatures(*_data(kind), W, K_PERM, dr.SEED)), kind)


def _check_gram_hits(out):
    import gram_checker
    import select_checker
    for kind in ("ids", "bytes"):
        def want():
            ev = select_checker.select(*_data(kind), np.asarray(EVAL_ROWS, np.int64))
            return gram_checker.hits(*_data(kind), W, dr.SEED, gram_checker.keys_of(ev[0], ev[1], W, dr.SEED))
        count, mask = dr._ref(("seq gram", kind), want)
        dr._eq(out[f"{kind}/count"], count, kind)
        dr._eq(out[f"{kind}/mask"], mask, kind)
        assert count[EVAL_ROWS].sum() > 0


def _check_repeat_stats(out):
    import repeat_checker
    for kind in ("ids", "bytes"):
        dr._eq(out[f"{kind}/stats"], dr._ref(("seq repeat", kind), lambda: repeat_checker.stats(*_data(kind), W)[0]), kind)


def _check_text_stats(out):
    import textstat_checker
    table, marks = dr._ref("seq textstat", lambda: textstat_checker.stats_of(*dr.pass_batch(), 40, "char"))
    dr._eq(out["table"], table, "table")
    dr._eq(out["marks"], marks, "line starts")


def _check_to_padded(out):
    import layout_checker
    ids, offs = dr.oracle_encode("A")
    for key, want in zip(("ids", "mask", "lengths"), layout_checker.padded(ids, offs, PAD_L, dr.PAD, 1, None)):
        dr._eq(out[key], want, key)
    assert int(out["truncated"][0]) == layout_checker.padded(ids, offs, PAD_L, dr.PAD, 1, None)[3] > 0


def _check_decode(out):
    flat, offs = dr.pass_batch()   # the tokens of a row spell its text; the corpus's rows are cut out of UTF-8 text anywhere,
    import decode_checker           # so the checker's lossy decode of each row is the reference, not the text itself
    ids, id_offs = dr.oracle_encode("A")
    dr._same_text(out, "", dr._ref("seq decode", lambda: decode_checker.decode_rows(dr._rows(ids, id_offs), dr.vocab("A")[0], [], True)), "decode")


CALLS = {
    "select": (_both(_select), _check_select), "first_equal": (_both(_first_equal), _check_first_equal), "minhash": (_both(_minhash), _check_minhash),
    "gram_hits": (_both(_gram_hits), _check_gram_hits), "repeat_stats": (_both(_repeat_stats), _check_repeat_stats),
    "text_stats": (_text_stats, _check_text_stats), "to_padded": (_to_padded, _check_to_padded), "decode": (_decode, _check_decode),
}


@pytest.fixture(scope="module")
def expected_calls():
    mp = pytest.MonkeyPatch()
    mp.delenv(KNOB, raising=False)
    ctx, want = dr.Ctx(), {}
    try:
        for name, (run, check) in CALLS.items():
            s = Sources()
            try:
                want[name] = run(s, ctx)
            finally:
                s.free()
            check(want[name])
    finally:
        mp.undo()
    return want


def _failing_select(s, ctx):
    """a select with an out-of-range row in device memory: refused after its check kernel has run, for either kind"""
    for kind, src in s.obj.items():
        rows = ctx.dev(np.asarray([0, 2, src.num_samples, 1], np.int64))
        with pytest.raises(tgx.TokenGeeXError) as e:
            src.select(rows, stream=ctx.stream)
        assert e.value.status == _lib.ERR_INVALID, (kind, str(e.value))


@pytest.mark.parametrize("fill", [None, "255"])
def test_calls_on_a_stream_forwards_backwards_and_after_a_failure(monkeypatch, expected_calls, fill):
    if fill is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, fill)
    ctx = dr.Ctx()
    s = Sources()
    try:
        for name in list(CALLS) + list(CALLS)[::-1]:
            got, want = CALLS[name][0](s, ctx), expected_calls[name]
            assert sorted(got) == sorted(want), name
            for k in want:
                a, b = np.asarray(got[k]), np.asarray(want[k])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
            _failing_select(s, ctx)
    finally:
        s.free()
