"""GPU parity of the lean relaxation step of encode5_kernel / encode6_kernel (csrc/device_common.h: relax5_lean_step,
TGX_E5_LEAN): a finalised lane is reset by its high word to a finite sentinel, "not reached" is a
class of values instead of -inf alone, and only the groups that hold a sample's end run the full step.  In every case
the ids, offsets and errors equal the CPU oracle's and those of TGX_E5_LEAN=0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import synth

from test_walk_compaction_gpu import _deep_texts, _distinct_scores, _vocab_with_runs
from util import corpus_and_vocab


def _outcome(fn):
    """('ok', ids, offsets) or ('nopath', sample, pos, length) of one encode call."""
    try:
        ids, offs = fn()
        return ("ok", ids, offs)
    except orc.NoPath as e:
        return ("nopath", int(e.sample), int(e.pos), int(e.length))
    except tgx.TokenGeeXError as e:
        assert e.status == 4, e
        return ("nopath", int(e.sample), int(e.pos), int(e.length))


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0], a[1:] if a[0] == "nopath" else None, b[1:] if b[0] == "nopath" else None)
    if a[0] == "ok":
        np.testing.assert_array_equal(a[2], b[2], err_msg=what)
        np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    else:
        assert a[1:] == b[1:], what


def _native(nat, flat, offs, dropout=0.0, seed=0):
    def run():
        res = nat.encode_batch_flat(flat, offs, dropout, seed)
        out = res.ids(), res.offsets()
        res.free()
        return out
    return _outcome(run)


FETCH = 4  # the one-instruction score fetch: part of every lean build (tgx_last_encode_lean_items)


def check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=None, dropout=0.0, seed=0, want=None, kernel="encode5_kernel",
                        lean_build=True):
    """The oracle's outcome (computed here unless given), the default build's and TGX_E5_LEAN=0's are the same.  The
    default pass must have run the lean build of `kernel` (lean_build=False: the kernel as it was — dropout, long
    tokens), TGX_E5_LEAN=0 none.  `lean`: whether encode5_kernel must have relaxed with the lean step (the COLD build at
    three positions per lane does when the model's scores pass the gate; None: the build decides).
    -> the oracle's outcome"""
    if want is None:
        want = _outcome(lambda: ora.encode_batch_flat(flat, offs, dropout, seed, threads=8))
    monkeypatch.delenv("TGX_E5_LEAN", raising=False)
    got = _native(nat, flat, offs, dropout, seed)
    assert kernel in nat.last_kernel_times()
    e5, e6 = nat.last_encode_lean_items()
    if lean_build:
        assert (e6 if kernel == "encode6_kernel" else e5) & FETCH, (e5, e6)
    else:
        assert (e5, e6) == (0, 0)
    assert lean is None or nat.last_encode_lean_step() == lean
    _same(got, want, "default build against the oracle")
    monkeypatch.setenv("TGX_E5_LEAN", "0")
    full = _native(nat, flat, offs, dropout, seed)
    assert nat.last_encode_lean_items() == (0, 0) and not nat.last_encode_lean_step()
    _same(full, want, "TGX_E5_LEAN=0 against the oracle")
    monkeypatch.delenv("TGX_E5_LEAN", raising=False)
    return want


@pytest.mark.parametrize("vocab", [32000, 65536])
def test_spec_vocabularies(monkeypatch, vocab):
    toks, scores, _ = synth.load_spec_vocab(vocab)
    flat, offs = synth.make_corpus(3 << 20, "mixed", seed_offset=1000, max_len=30000)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    want = check_lean_and_full(monkeypatch, nat, ora, flat, offs)
    assert want[0] == "ok" and want[1].size > 0


@pytest.mark.parametrize("ppl", ["2", "3", "4"])
@pytest.mark.parametrize("cold", [False, True])
def test_positions_per_lane_hot_and_cold(monkeypatch, ppl, cold):
    """Two to four groups per trip, every value in LDS or 500 of them with every token its own score (COLD builds),
    deep and shallow samples mixed."""
    rng = np.random.default_rng(int(ppl) * 10 + cold)
    flat, offs, toks, scores = corpus_and_vocab(1 << 20, "mixed", 8000, 16, seed_offset=61, max_len=20000)
    toks, scores = _vocab_with_runs(toks, scores)
    if cold:
        scores = _distinct_scores(scores, rng)
        monkeypatch.setenv("TGX_E5_HOT", "500")
    monkeypatch.setenv("TGX_PPL", ppl)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=True if cold and ppl == "3" else None)
    if cold:
        assert nat.last_encode_hot_values() == 500
    f2, o2 = tgx.pack(_deep_texts(rng, 1500))
    check_lean_and_full(monkeypatch, nat, ora, f2, o2, lean=True if cold and ppl == "3" else None)


def _sparse_vocab(seed, max_len=16):
    """No single-byte cover: most positions of a text are not reached, and a token's interior never is unless another
    token ends there."""
    rng = np.random.default_rng(seed)
    flat, _ = synth.make_corpus(64 << 10, "ascii", max_len=256)
    toks, scores = synth.random_vocab(rng, bytes(flat), n_multi=3000, max_len=max_len, all_bytes=False)
    return rng, bytes(flat), toks, scores


@pytest.mark.parametrize("cold", [False, True])
@pytest.mark.parametrize("ppl", [None, "2", "3", "4"])
def test_unreachable_stretches_bridged_by_long_tokens(monkeypatch, ppl, cold):
    """Concatenations of tokens: every sample has a path, and the stretches inside its long tokens are reached by nothing
    (values of the sentinel class travel through lean and full groups, across groups and trips)."""
    rng, _, toks, scores = _sparse_vocab(5)
    long_toks = [t for t in toks if len(t) >= 12]
    assert len(long_toks) > 100
    texts = []
    for i in range(1200):
        k = int(rng.integers(1, 40))
        pool = long_toks if i % 3 == 0 else toks
        texts.append(b"".join(pool[int(j)] for j in rng.integers(0, len(pool), k)))
    texts += [long_toks[i] for i in range(40)] + [b""]
    if ppl:
        monkeypatch.setenv("TGX_PPL", ppl)
    if cold:
        monkeypatch.setenv("TGX_E5_HOT", "100")
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    flat, offs = tgx.pack(texts)
    want = check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=True if cold and ppl == "3" else None)
    assert want[0] == "ok"


@pytest.mark.parametrize("cold", [False, True])
def test_unreachable_ends_and_the_lowest_failing_sample(monkeypatch, cold):
    """Samples whose end is not reached, at every length 1 .. 200 (every lane, every group of a trip): alone, and in
    batches with several failing samples, where the oracle's sample, position and length must come back."""
    rng, text, toks, scores = _sparse_vocab(6, max_len=8)
    if cold:
        monkeypatch.setenv("TGX_E5_HOT", "100")
        monkeypatch.setenv("TGX_PPL", "3")
    lean = True if cold else None
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    ok_texts, bad_texts = [], []
    for n in list(range(1, 201)) * 3:
        o = int(rng.integers(0, len(text) - 256))
        t = text[o:o + n]
        try:
            ora.encode(t)
            ok_texts.append(t)
        except orc.NoPath:
            bad_texts.append(t)
    good = [b"".join(toks[int(j)] for j in rng.integers(0, len(toks), int(rng.integers(1, 50)))) for _ in range(300)] + ok_texts
    assert len(bad_texts) > 200
    # every failing sample in a batch of its own kind: one launch, the first one is reported
    for first in range(0, 24):
        batch = bad_texts[first::24]
        flat, offs = tgx.pack(batch)
        want = check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=lean)
        assert want[0] == "nopath" and want[1] == 0 and want[2] == len(batch[0])
    # failing samples among good ones: the lowest failing sample wins, wherever the longest-first order puts it
    for trial in range(6):
        batch = list(good)
        where = sorted(int(x) for x in rng.choice(np.arange(20, len(batch)), 5, replace=False))
        for k, w in enumerate(where):
            batch[w] = bad_texts[(trial * 5 + k) % len(bad_texts)]
        flat, offs = tgx.pack(batch)
        want = check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=lean)
        assert want[0] == "nopath" and want[1] == where[0]
    flat, offs = tgx.pack(good)
    assert check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=lean)[0] == "ok"


@pytest.mark.parametrize("cold", [False, True])
@pytest.mark.parametrize("ppl", [None, "2", "3", "4"])
def test_sample_ends_at_every_lane_and_group(monkeypatch, ppl, cold):
    """Lengths 0 .. 100, 190 .. 194, 47 / 48 / 49, 63 / 64 / 65, several of each and neighbours of the longest-first
    order in one wave, so that the rows of a wave end in different groups of one trip."""
    rng = np.random.default_rng(77)
    flat, offs, toks, scores = corpus_and_vocab(256 << 10, "mixed", 3000, 16, seed_offset=5, max_len=4096)
    text = bytes(flat)
    lengths = list(range(0, 101)) + list(range(190, 195)) + [47, 48, 49, 63, 64, 65] * 4 + [16, 32, 80, 96, 112, 128, 144, 160, 176, 192] * 2
    texts = []
    for rep in range(4):
        for n in lengths:
            o = int(rng.integers(0, len(text) - 256))
            texts.append(text[o:o + n])
    if ppl:
        monkeypatch.setenv("TGX_PPL", ppl)
    if cold:
        scores = _distinct_scores(scores, rng)
        monkeypatch.setenv("TGX_E5_HOT", "100")
    lean = True if cold and ppl == "3" else None
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    f2, o2 = tgx.pack(texts)
    assert check_lean_and_full(monkeypatch, nat, ora, f2, o2, lean=lean)[0] == "ok"
    # the same lengths where many ends are not reached: each batch holds one length per residue, the first fails or not
    _, stext, stoks, sscores = _sparse_vocab(8, max_len=6)
    snat, sora = tgx.NativeModel(stoks, sscores), orc.OracleModel(stoks, sscores)
    for n in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 190, 191, 192, 193, 194):
        batch = [stext[o:o + n] for o in range(0, 4000, 97)]
        f3, o3 = tgx.pack(batch)
        check_lean_and_full(monkeypatch, snat, sora, f3, o3, lean=lean)


@pytest.mark.parametrize("cold", [False, True])
def test_exact_ties_and_positive_scores(monkeypatch, cold):
    rng = np.random.default_rng(4025)
    if cold:
        monkeypatch.setenv("TGX_E5_HOT", "100")
        monkeypatch.setenv("TGX_PPL", "3")
    lean = True if cold else None
    flat, offs = synth.make_corpus(512 << 10, "mixed", seed_offset=75, max_len=20000)
    toks, scores = synth.random_vocab(rng, bytes(flat[: 96 << 10]), n_multi=4000, max_len=16, tie_fraction=0.6)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    assert check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=lean)[0] == "ok"
    pos = np.abs(np.asarray(scores, np.float64)) + 0.25  # every score positive: the longest segmentation in tokens wins
    nat2, ora2 = tgx.NativeModel(toks, pos), orc.OracleModel(toks, pos)
    assert check_lean_and_full(monkeypatch, nat2, ora2, flat, offs, lean=lean)[0] == "ok"
    mixed = np.where(rng.random(len(toks)) < 0.5, pos, np.asarray(scores, np.float64))
    nat3, ora3 = tgx.NativeModel(toks, mixed), orc.OracleModel(toks, mixed)
    assert check_lean_and_full(monkeypatch, nat3, ora3, flat, offs, lean=lean)[0] == "ok"


@pytest.mark.parametrize("inside", [True, False])
def test_lowest_score_at_the_gate(monkeypatch, inside):
    """A vocabulary whose lowest score has a magnitude just below 2^960 runs the lean step, one at 2^960 the full step in
    the build without the lean step, which keeps the other items (the COLD build at three positions per lane: the one
    that has the lean step); the tokens with that score are on every path (the only cover of their byte)."""
    rng = np.random.default_rng(960)
    monkeypatch.setenv("TGX_E5_HOT", "100")
    monkeypatch.setenv("TGX_PPL", "3")
    flat, offs = synth.make_corpus(256 << 10, "ascii", seed_offset=76, max_len=3000)
    toks, scores = synth.random_vocab(rng, bytes(flat[: 64 << 10]), n_multi=2000, max_len=16, tie_fraction=0.3)
    scores = np.asarray(scores, np.float64).copy()
    edge = 2.0 ** 960
    low = -np.nextafter(edge, 0.0) if inside else -edge
    for b in (b"e", b" ", b"t"):
        scores[toks.index(b)] = low
    scores[toks.index(b"a")] = -low if inside else edge  # and a positive one of the same magnitude
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    assert check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=inside)[0] == "ok"
    # the same where positions are not reached
    _, stext, stoks, sscores = _sparse_vocab(9, max_len=8)
    sscores = np.asarray(sscores, np.float64).copy()
    sscores[:: 7] = low
    snat, sora = tgx.NativeModel(stoks, sscores), orc.OracleModel(stoks, sscores)
    texts = [b"".join(stoks[int(j)] for j in rng.integers(0, len(stoks), int(rng.integers(1, 60)))) for _ in range(600)]
    f2, o2 = tgx.pack(texts)
    assert check_lean_and_full(monkeypatch, snat, sora, f2, o2, lean=inside)[0] == "ok"
    f3, o3 = tgx.pack(texts[:300] + [stext[100:177]] + texts[300:] + [stext[5:300]])
    check_lean_and_full(monkeypatch, snat, sora, f3, o3, lean=inside)


@pytest.mark.parametrize("pool", [None, "0"])
@pytest.mark.parametrize("cold", [False, True])
def test_long_sample_kernel(monkeypatch, cold, pool):
    """Samples of 2 .. 4 KiB go to encode6_kernel (its relaxer shares the steps), hot and COLD, with and without the
    walkers' pool; ends at every lane of the last trip; a sparse vocabulary's bridged stretches and a failing sample."""
    rng = np.random.default_rng(66 + cold)
    flat, offs, toks, scores = corpus_and_vocab(1 << 20, "mixed", 8000, 16, seed_offset=62, max_len=20000)
    if cold:
        scores = _distinct_scores(scores, rng)
        monkeypatch.setenv("TGX_E5_HOT", "500")
    if pool is not None:
        monkeypatch.setenv("TGX_E6_POOL", pool)
    monkeypatch.setenv("TGX_LONG_THRESHOLD", "2048")
    text = bytes(flat)
    texts = [text[o:o + 2048 + (i * 37) % 2048] for i, o in enumerate(range(0, len(text) - 4096, 9000))]
    texts += [text[o:o + int(n)] for o, n in zip(range(0, 200000, 1000), rng.integers(0, 2048, 200))]
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    f2, o2 = tgx.pack(texts)
    assert check_lean_and_full(monkeypatch, nat, ora, f2, o2, kernel="encode6_kernel")[0] == "ok"
    assert nat.last_encode_long_samples() >= 100
    _, stext, stoks, sscores = _sparse_vocab(10)
    if cold:
        sscores = _distinct_scores(sscores, rng)
    snat, sora = tgx.NativeModel(stoks, sscores), orc.OracleModel(stoks, sscores)
    stexts = []
    for i in range(60):
        t = b""
        while len(t) < 2048 + 31 * i:
            t += stoks[int(rng.integers(0, len(stoks)))]
        stexts.append(t)
    f3, o3 = tgx.pack(stexts)
    assert check_lean_and_full(monkeypatch, snat, sora, f3, o3, kernel="encode6_kernel")[0] == "ok"
    f4, o4 = tgx.pack(stexts[:20] + [stexts[20] + stext[:40], stexts[21][:-1] + b"\x00"] + stexts[22:])
    want = check_lean_and_full(monkeypatch, snat, sora, f4, o4, kernel="encode6_kernel")
    assert want[0] == "nopath" and want[1] in (20, 21)


def test_long_token_and_dropout_builds_keep_the_step(monkeypatch):
    """Tokens of up to 24 bytes (the LONG build) and dropout: no lean variant, and the switch changes nothing."""
    rng = np.random.default_rng(4024)
    flat, offs = synth.make_corpus(384 << 10, "mixed", seed_offset=74, max_len=20000)
    toks, scores = synth.random_vocab(rng, bytes(flat[: 96 << 10]), n_multi=4000, max_len=24, tie_fraction=0.5)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    assert 16 < nat.max_token_len <= 24
    assert check_lean_and_full(monkeypatch, nat, ora, flat, offs, lean=False, lean_build=False)[0] == "ok"
    toks2, scores2 = synth.random_vocab(rng, bytes(flat[: 96 << 10]), n_multi=4000, max_len=16, tie_fraction=0.5)
    nat2, ora2 = tgx.NativeModel(toks2, scores2), orc.OracleModel(toks2, scores2)
    assert check_lean_and_full(monkeypatch, nat2, ora2, flat, offs, lean=False, lean_build=False, dropout=0.25, seed=7)[0] == "ok"
    monkeypatch.setenv("TGX_E5_HOT", "100")
    monkeypatch.setenv("TGX_PPL", "3")
    assert check_lean_and_full(monkeypatch, nat2, ora2, flat, offs, lean=True)[0] == "ok"
