"""GPU parity of encode5_kernel's top-table builds (csrc/encode5.hip: TOP; csrc/top_table.h): a walk's first two trie
levels from one table indexed by the first two text bytes, no copy of the root's records in LDS, and the geometry that
the freed 2 KiB allow (three positions per lane x 14 waves).  Ids and no-path reports bit-exact against the CPU oracle
(reference src/model.rs:59-129), with TGX_E5_TOP=1 (the default) and 0 (the kernels and the geometry as they were)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import synth

TOPS = ["1", "0"]


def _same(nat, ora, texts):
    """The batch through both: equal ids and offsets, or the same no-path report (lowest failing sample, message)."""
    f, o = tgx.pack(texts)
    try:
        want_ids, want_offs = ora.encode_batch_flat(f, o, threads=4)
    except orc.NoPath as want:
        with pytest.raises(tgx.TokenGeeXError) as e:
            nat.encode_batch_flat(f, o)
        assert str(e.value) == str(want) and e.value.sample == want.sample, (texts, str(e.value), str(want))
        return
    res = nat.encode_batch_flat(f, o)
    got_ids, got_offs = res.ids(), res.offsets()
    res.free()
    np.testing.assert_array_equal(got_offs, want_offs)
    np.testing.assert_array_equal(got_ids, want_ids)


def _ran_top(nat, top):
    assert "encode5_kernel" in nat.last_kernel_times()
    assert nat.last_encode_top_table() == (top == "1")


TINY_VOCABS = {
    # a 2-byte token whose first byte is no token: "a" alone has no path, "ab" has
    "first_byte_no_token": ([b"ab", b"b", b"c", b"abc", b"ca"], [-1.0, -2.0, -2.5, -1.5, -3.0]),
    # 1-byte tokens without children
    "leaves_only": ([b"a", b"b", b"c", b"\x00", b"\xff"], [-1.0, -2.0, -3.0, -1.5, -2.5]),
    # 0x00 / 0xFF in either place of the pair, 0xFF alone no token
    "edge_bytes": ([b"\x00", b"\x00\x00", b"\x00\xff", b"\xff\x00", b"\xff\xff", b"\xff\xff\xff", b"a", b"a\x00", b"a\xffq", b"q"],
                   [-3.0, -4.0, -1.0, -1.25, -1.5, -2.0, -2.5, -2.25, -0.5, -3.5]),
    # pairs that are tokens AND go on, beside single bytes: the last byte of one sample and the first of the next make "ab"
    "pairs": ([b"a", b"b", b"x", b"ab", b"abx", b"ba", b"xa"], [-2.0, -2.0, -2.0, -1.0, -0.5, -3.0, -1.0]),
}
TINY_TEXTS = {
    "first_byte_no_token": [[b"ab", b"abc", b"cab", b"b", b"", b"bcab" * 9, b"c"], [b"ab", b"a"], [b"a"], [b"cab", b"ca", b"aab"], [b"abca"]],
    "leaves_only": [[b"", b"a", b"ab", b"\x00\xff", b"abc\x00\xff" * 13, b"\xff"], [b"a", b"ad", b"d"]],
    "edge_bytes": [[b"\x00", b"\x00\x00", b"\x00\xff\xff\x00", b"\xff\xff\xff\xff\xff", b"a\x00a\xffq", b"", b"a"], [b"a\xff"], [b"\xff"],
                   [b"\x00\xff", b"\xff\x00\xff"]],
    # "xa" | "bx": "ab" straddles the samples and must not be taken; the batch's last sample ends the text (1 and 2 bytes)
    "pairs": [[b"xa", b"bx", b"a", b"b", b"ab", b"", b"abx", b"xab" * 21, b"a"], [b"b", b"xa", b"ab"], [b"abxa"], [b"a" * 47, b"ab" * 24, b"b" * 49]],
}


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("name", sorted(TINY_VOCABS))
def test_tiny_vocabularies_and_texts(monkeypatch, name, top):
    monkeypatch.setenv("TGX_E5_TOP", top)
    monkeypatch.setenv("TGX_PATH", "rows5")
    toks, scores = TINY_VOCABS[name]
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    for texts in TINY_TEXTS[name]:
        _same(nat, ora, texts)
    _ran_top(nat, top)


@pytest.mark.parametrize("top", TOPS)
def test_sample_lengths_around_the_trips(monkeypatch, top):
    """Samples of 0, 1, 2 bytes and of 47 / 48 / 49 and 63 / 64 / 65 (a trip of three and of four positions per lane),
    each also as the last sample of the text, whose walks read the padding."""
    monkeypatch.setenv("TGX_E5_TOP", top)
    monkeypatch.setenv("TGX_PATH", "rows5")
    rng = np.random.default_rng(3)
    toks = [bytes([c]) for c in range(97, 123)] + [b"ab", b"bc", b"abc", b"za", b"zz", b"abcdefgh", b"q" * 16]
    scores = -(rng.random(len(toks)) * 4.0 + 1.0)
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    raw = bytes(rng.integers(97, 123, size=4096, dtype=np.uint8))
    lens = (0, 1, 2, 47, 48, 49, 63, 64, 65)
    for ppl in ("3", "4"):
        monkeypatch.setenv("TGX_PPL", ppl)
        _same(nat, ora, [raw[7 * n:7 * n + n] for n in lens])
        for n in lens:  # as the last sample
            _same(nat, ora, [raw[:100], raw[200:200 + n]])
        _ran_top(nat, top)


@pytest.fixture(scope="module")
def mixed():
    flat, offs = synth.make_corpus(1 << 20, "mixed", seed_offset=23, max_len=3000)
    toks, scores = synth.build_vocab(flat, 6000, 16)
    rng = np.random.default_rng(5)
    scores = np.asarray(scores, np.float64) - rng.random(len(scores)) * 1e-3   # every token its own value
    ora = orc.OracleModel(toks, scores)
    return flat, offs, toks, scores, ora.encode_batch_flat(flat, offs, threads=8)


def _check(nat, flat, offs, want):
    res = nat.encode_batch_flat(flat, offs)
    got_ids, got_offs = res.ids(), res.offsets()
    res.free()
    np.testing.assert_array_equal(got_offs, want[1])
    np.testing.assert_array_equal(got_ids, want[0])


@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("hot", [None, "500"])
@pytest.mark.parametrize("ppl", ["2", "3", "4"])
def test_positions_per_lane_hot_and_cold(monkeypatch, mixed, ppl, hot, top):
    flat, offs, toks, scores, want = mixed
    monkeypatch.setenv("TGX_E5_TOP", top)
    monkeypatch.setenv("TGX_PPL", ppl)
    if hot:
        monkeypatch.setenv("TGX_E5_HOT", hot)
    nat = tgx.NativeModel(toks, scores)
    _check(nat, flat, offs, want)
    _ran_top(nat, top)
    assert (nat.last_encode_hot_values() < nat.score_values()) == (hot is not None)


@pytest.mark.parametrize("top", TOPS)
def test_value_rerank_remaps_the_table(monkeypatch, mixed, top):
    """TGX_VALUE_RANK=counts: the first encode re-ranks the score values by match counts — the records' ranks and both
    halves of the top table's — and encodes as the oracle does, with every value in LDS and with most of them cold."""
    flat, offs, toks, scores, want = mixed
    monkeypatch.setenv("TGX_E5_TOP", top)
    monkeypatch.setenv("TGX_VALUE_RANK", "counts")
    nat = tgx.NativeModel(toks, scores)
    _check(nat, flat, offs, want)
    _ran_top(nat, top)
    monkeypatch.setenv("TGX_E5_HOT", "300")
    _check(nat, flat, offs, want)
    monkeypatch.setenv("TGX_VALUE_RANK", "model")
    plain = tgx.NativeModel(toks, scores)   # (not re-ranked: the same ids)
    _check(plain, flat, offs, want)


@pytest.mark.parametrize("top", TOPS)
def test_derived_model_has_its_own_table(monkeypatch, mixed, top):
    """A derived model (the parent's slots, dead branches) encodes as the oracle of its own vocabulary: single bytes and
    pairs dropped from the parent must be gone from the child's top table."""
    flat, offs, toks, scores, _ = mixed
    monkeypatch.setenv("TGX_E5_TOP", top)
    rng = np.random.default_rng(11)
    parent = tgx.NativeModel(toks, scores)
    short = [i for i, t in enumerate(toks) if len(t) <= 2]
    drop = set(rng.choice(short, size=len(short) // 3, replace=False).tolist()) | set(rng.choice(len(toks), size=len(toks) // 4, replace=False).tolist())
    drop -= {i for i, t in enumerate(toks) if len(t) == 1 and t[0] < 128}   # (keep ASCII single bytes: most samples keep a path)
    keep = np.array([i for i in range(len(toks)) if i not in drop], np.uint32)
    sc = -(rng.random(keep.size) * 8.0 + 1.0)
    child = parent.derive(keep, sc)
    ora = orc.OracleModel([toks[i] for i in keep], sc)
    n = 300
    sub_o = offs[: n + 1]
    for a in range(0, n, 60):   # a no-path sample fails its batch: several batches, each as the oracle reports it
        _same(child, ora, [flat[int(sub_o[i]):int(sub_o[i + 1])].tobytes() for i in range(a, a + 60)])
    _ran_top(child, top)


@pytest.fixture(scope="module")
def spec16():
    """The committed 32 000-entry vocabulary and 16 MiB of samples of at most 256 bytes (more samples than the chip has
    rows: the shape of test_launch_geometry_fits_the_device)."""
    toks, scores, _ = synth.load_spec_vocab(32000)
    flat, offs = synth.make_corpus(16 << 20, "mixed", seed_offset=1000, max_len=256)
    return toks, np.asarray(scores, np.float64), flat, offs


def test_spec_vocabulary_runs_fourteen_waves(monkeypatch, spec16):
    toks, scores, flat, offs = spec16
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    want = ora.encode_batch_flat(flat, offs, threads=8)
    _check(nat, flat, offs, want)
    _ran_top(nat, "1")
    assert nat.last_encode_waves_per_cu() == 14
    assert nat.last_encode_hot_values() == nat.score_values() == 9652
    monkeypatch.setenv("TGX_E5_TOP", "0")
    _check(nat, flat, offs, want)
    _ran_top(nat, "0")
    assert nat.last_encode_waves_per_cu() == 13 and nat.last_encode_hot_values() == nat.score_values()


def _with_distinct_values(scores, n_values):
    """The scores with tokens split off their shared values, one by one, until there are n_values distinct ones."""
    sc = scores.copy()
    vals, counts = np.unique(sc, return_counts=True)
    have = set(vals.tolist())
    shared = {v for v, c in zip(vals.tolist(), counts.tolist()) if c > 1}
    left = dict(zip(vals.tolist(), counts.tolist()))
    k = 0
    for i in range(sc.size):
        if len(have) >= n_values:
            break
        v = float(sc[i])
        if v in shared and left[v] > 1:
            k += 1
            nv = v - k * 1e-9
            assert nv not in have
            left[v] -= 1
            sc[i] = nv
            have.add(nv)
    assert np.unique(sc).size == n_values
    return sc


@pytest.mark.parametrize("n_values,waves", [(9727, 14), (9728, 13)])
def test_the_last_vocabulary_that_fits_beside_fourteen_waves(spec16, n_values, waves):
    """9 727 values are the most that fit beside 14 waves x 3 positions without the root copy; one more takes the
    13-wave geometry, still with every value in LDS."""
    toks, scores, flat, offs = spec16
    sc = _with_distinct_values(scores, n_values)
    nat, ora = tgx.NativeModel(toks, sc), orc.OracleModel(toks, sc)
    res = nat.encode_batch_flat(flat, offs)
    got_ids, got_offs = res.ids(), res.offsets()
    res.free()
    _ran_top(nat, "1")
    assert nat.score_values() == n_values == nat.last_encode_hot_values()
    assert nat.last_encode_waves_per_cu() == waves
    n = 2000   # (the oracle over the first samples: the whole batch is the case above's)
    want_ids, want_offs = ora.encode_batch_flat(flat[: int(offs[n])], offs[: n + 1], threads=8)
    np.testing.assert_array_equal(got_offs[: n + 1], want_offs)
    np.testing.assert_array_equal(got_ids[: int(want_offs[n])], want_ids)
