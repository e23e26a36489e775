"""GPU parity of "ids in place" (DESIGN.md section R8): encode5_kernel's counting builds carry every position's token
count through the relaxation (csrc/device_common.h: relax5_step's CNT), the counts are scanned into the result's offsets
before the trace, and trace_kernel writes each id where it belongs (csrc/trace_body.h: INPLACE) — no scratch of 4 bytes
per text byte, no compact_kernel.  In every case the ids, offsets and errors equal the CPU oracle's and those of the same
call with TGX_IDS_IN_PLACE=0, bit for bit, and the pass that claims to have run in place did (and the other did not):
otherwise the comparison proves nothing.

The shapes are the smallest at which this can go wrong: sample lengths around the 16-position groups, the trips of 32 /
48 / 64 positions, the trace's 64-position windows and its ring's 64-token flush."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from oracle import oracle as orc
from tokengeex_amd import synth

import hostile_cases as hc

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 4097)

# Which builds of encode5_kernel count by default (csrc/encode5.hip: kE5CntHot, kE5CntHot2, kE5CntCold, kE5CntCold3; decided
# per build by measurement, profiles/ids_in_place).  A build that does not count keeps its passes on the old path, and the
# cases that run it must then see the accessor false with the switch at 1 as well.
COUNTS = {"hot": True, "hot2": True, "cold": True, "cold3": True}


def _build(cold: bool, ppl: int) -> str:
    return ("cold3" if ppl == 3 else "cold") if cold else ("hot2" if ppl == 2 else "hot")


def _outcome(fn):
    """('ok', ids, offsets) or ('nopath', sample, pos, length) of one encode call."""
    try:
        ids, offs = fn()
        return ("ok", ids, offs)
    except orc.NoPath as e:
        return ("nopath", int(e.sample), int(e.pos), int(e.length))
    except tgx.TokenGeeXError as e:
        assert e.status == 4, e  # TGX_ERR_NO_PATH: anything else (TGX_ERR_DEVICE: the trace's self-check) is a failure
        return ("nopath", int(e.sample), int(e.pos), int(e.length))


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0], a[1:] if a[0] == "nopath" else None, b[1:] if b[0] == "nopath" else None)
    if a[0] == "ok":
        assert a[1].dtype == b[1].dtype and a[2].dtype == b[2].dtype, what
        np.testing.assert_array_equal(a[2], b[2], err_msg=what)
        np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    else:
        assert a[1:] == b[1:], what


def _native(nat, flat, offs):
    def run():
        res = nat.encode_batch_flat(flat, offs)
        out = res.ids(), res.offsets()
        res.free()
        return out
    return _outcome(run)


def check_both_paths(monkeypatch, nat, want, flat, offs, in_place=True):
    """The switch at 1 and at 0 against the oracle's outcome `want`, and which path each pass took.  in_place: whether the
    pass with the switch at 1 must have written its ids in place (False: a batch that is on the old path by construction, or
    a build that does not count)."""
    monkeypatch.setenv("TGX_IDS_IN_PLACE", "1")
    new = _native(nat, flat, offs)
    assert nat.last_encode_ids_in_place() == in_place
    times = nat.last_kernel_times()
    assert "trace_kernel" in times and ("compact_kernel" in times) == (not in_place and new[0] == "ok"), sorted(times)
    _same(new, want, "TGX_IDS_IN_PLACE=1 against the oracle")
    monkeypatch.setenv("TGX_IDS_IN_PLACE", "0")
    old = _native(nat, flat, offs)
    assert not nat.last_encode_ids_in_place()
    assert "compact_kernel" in nat.last_kernel_times() or old[0] != "ok"
    _same(old, want, "TGX_IDS_IN_PLACE=0 against the oracle")
    _same(new, old, "TGX_IDS_IN_PLACE=1 against 0")
    monkeypatch.delenv("TGX_IDS_IN_PLACE", raising=False)
    return new


# ---- the shared, unmodified inputs and references -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spec():
    toks, scores, _ = synth.load_spec_vocab(32000)
    return toks, np.asarray(scores, np.float64)


@functools.lru_cache(maxsize=None)
def _distinct():
    """The vocabulary of bench.py --distinct-scores: every token that occurs a score of its own, the single bytes that never
    occur on a floor value."""
    toks, scores = _spec()
    scores = scores + np.random.default_rng(5).uniform(-0.4, 0.4, len(toks))
    seen = np.zeros(256, bool)
    seen[np.unique(synth.make_corpus(8 << 20, "mixed", seed_offset=1000)[0])] = True
    floor = float(scores.min()) - 1.0
    for i, t in enumerate(toks):
        if len(t) == 1 and not seen[t[0]]:
            scores[i] = floor
    return toks, scores


@functools.lru_cache(maxsize=None)
def _models(which: str):
    toks, scores = _spec() if which == "spec" else _distinct()
    return tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)


@functools.lru_cache(maxsize=None)
def _length_texts():
    flat, _ = synth.make_corpus(64 << 10, "mixed", seed_offset=77)
    text, at, out = bytes(flat), 0, []
    for n in LENGTHS:
        out.append(text[at:at + n])
        at += n + 13
    assert [len(t) for t in out] == list(LENGTHS)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _length_batch(which: str, shuffled: bool):
    """(flat, offsets, the oracle's outcome) of the length list, in its order or shuffled"""
    texts = list(_length_texts())
    if shuffled:
        texts = [texts[i] for i in np.random.default_rng(24).permutation(len(texts))]
        assert [len(t) for t in texts] != list(LENGTHS)
    flat, offs = tgx.pack(texts)
    want = _outcome(lambda: _models(which)[1].encode_batch_flat(flat, offs, threads=4))
    assert want[0] == "ok" and want[2][-1] == want[1].size > 0
    return flat, offs, want


# ---- sample lengths ---------------------------------------------------------------------------------------------------
def _keep_the_long_sample_in_encode5(monkeypatch):
    """In a batch of a few kilobytes the host would send the 4097-byte sample to encode6_kernel (a lone long sample is a
    serial chain), and the pass would take the old path: these cases are about the in-place path at every length."""
    monkeypatch.setenv("TGX_LONG_THRESHOLD", "0")


@pytest.mark.parametrize("shuffled", [False, True])
def test_lengths_in_order_and_shuffled(monkeypatch, shuffled):
    _keep_the_long_sample_in_encode5(monkeypatch)
    nat, _ = _models("spec")
    flat, offs, want = _length_batch("spec", shuffled)
    check_both_paths(monkeypatch, nat, want, flat, offs)


def test_forced_restart_of_the_finalised_lane(monkeypatch):
    """40 repetitions of one 16-byte token: every position's winner is the 16-byte token from the same lane one group
    back, i.e. the candidate that the finalised lane is restarted with, and the count rides on it all the way."""
    toks, _ = _spec()
    nat, ora = _models("spec")
    for tid, t in enumerate(toks):
        if len(t) != 16:
            continue
        ids = ora.encode(t * 40)
        if len(ids) == 40 and all(int(i) == tid for i in ids):
            break
    else:
        pytest.fail("no 16-byte token of the vocabulary repeats as itself")
    flat, offs = tgx.pack([t * 40, t * 3, t])
    want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=2))
    assert want[0] == "ok" and list(want[2]) == [0, 40, 43, 44] and set(int(i) for i in want[1]) == {tid}
    check_both_paths(monkeypatch, nat, want, flat, offs)


def test_one_token_per_byte(monkeypatch):
    """b"a" and sixteen of them, scored so that single bytes win: 1 000 bytes are 1 000 tokens — count = n, the densest path,
    the trace's ring flushed fifteen times."""
    toks, scores = [b"a", b"a" * 16], np.array([-1.0, -20.0])
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    flat, offs = tgx.pack([b"a" * 1000, b"a" * 17, b""])
    want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=2))
    assert want[0] == "ok" and list(want[2]) == [0, 1000, 1017, 1017] and not want[1].any()
    check_both_paths(monkeypatch, nat, want, flat, offs)
    nat.free()


# ---- geometries and steps, each on the length list ---------------------------------------------------------------------
# (environment, vocabulary, whether the COLD build must run (None: the host's choice), positions per lane (None: the
# four that the host chooses for a batch this small), whether it must relax with the lean step (None: the build decides))
GEOMETRIES = [
    ({"TGX_PPL": "2", "TGX_BPC": "1"}, "spec", False, 2, None),
    ({"TGX_PPL": "2"}, "spec", None, 2, None),
    ({"TGX_PPL": "3"}, "spec", False, 3, None),
    ({"TGX_PPL": "4"}, "spec", False, 4, None),
    ({"TGX_E5_HOT": "500"}, "spec", True, None, None),
    ({"TGX_E5_HOT": "500", "TGX_PPL": "2"}, "spec", True, 2, None),
    ({"TGX_E5_LEAN": "0"}, "spec", False, None, False),
    ({"TGX_E5_LEAN": "1"}, "spec", False, None, None),
    ({"TGX_E5_LEAN": "0", "TGX_PPL": "3", "TGX_E5_HOT": "500"}, "spec", True, 3, False),
    ({"TGX_PPL": "3"}, "distinct", True, 3, True),
    ({"TGX_PPL": "3", "TGX_E5_LEAN": "0"}, "distinct", True, 3, False),
    ({"TGX_TRACE_CARRY": "0"}, "spec", False, None, None),
    ({"TGX_TRACE_CARRY": "1"}, "spec", False, None, None),
    ({"TGX_TRACE_STRIDE": "0"}, "spec", False, None, None),
    ({"TGX_TRACE_STRIDE": "2"}, "spec", False, None, None),
    ({"TGX_TRACE_CARRY": "1", "TGX_TRACE_STRIDE": "0"}, "spec", False, None, None),
]


def _case_id(v):
    return "-".join(f"{k[4:]}={x}" for k, x in v.items()) if isinstance(v, dict) else None


@pytest.mark.parametrize("env,which,want_cold,ppl,lean_step", GEOMETRIES, ids=_case_id)
def test_geometries_and_steps(monkeypatch, env, which, want_cold, ppl, lean_step):
    _keep_the_long_sample_in_encode5(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nat, _ = _models(which)
    for shuffled in (False, True):
        flat, offs, want = _length_batch(which, shuffled)
        monkeypatch.setenv("TGX_IDS_IN_PLACE", "1")
        _native(nat, flat, offs)  # which build runs: COLD iff some score values stay out of the block's LDS
        cold = nat.last_encode_hot_values() < nat.score_values()
        assert want_cold is None or cold == want_cold
        check_both_paths(monkeypatch, nat, want, flat, offs, in_place=COUNTS[_build(cold, ppl if ppl is not None else 4)])
        if lean_step is not None:
            monkeypatch.delenv("TGX_IDS_IN_PLACE", raising=False)
            _native(nat, flat, offs)
            assert nat.last_encode_lean_step() == lean_step
            if env.get("TGX_E5_LEAN") == "0":
                assert nat.last_encode_lean_items() == (0, 0)


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_no_path_names_the_same_sample_and_position(monkeypatch):
    """A vocabulary without the byte 'q' and one sample that holds it, between valid ones: TGX_ERR_NO_PATH with the
    oracle's sample and position on both paths; the kernels do not fault on it, and the count of such a sample is 0."""
    toks, scores = hc.bytes_heavy(-6.0, without=(ord("q"),))
    nat, ora = tgx.NativeModel(toks, scores), orc.OracleModel(toks, scores)
    good = [b"sampling the lattice", b"range fallback " * 9, b"", b"x" * 65, b"lattice" * 30]
    for bad in (b"sampling q lattice", b"q", b"fallback " * 20 + b"q", b"q" + b"range" * 40):
        texts = good[:3] + [bad] + good[3:]
        flat, offs = tgx.pack(texts)
        want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=2))
        assert want[0] == "nopath" and want[1] == 3
        check_both_paths(monkeypatch, nat, want, flat, offs)
    # two failing samples: the lowest is named, wherever the longest-first order puts it
    flat, offs = tgx.pack(good[:2] + [b"q" * 3] + good[2:] + [b"lattice q" * 50])
    want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=2))
    assert want[0] == "nopath" and want[1] == 2
    check_both_paths(monkeypatch, nat, want, flat, offs)
    flat, offs = tgx.pack(good)
    want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=2))
    assert want[0] == "ok"
    check_both_paths(monkeypatch, nat, want, flat, offs)
    nat.free()


# ---- the old path is kept -------------------------------------------------------------------------------------------------
def test_a_long_sample_keeps_the_old_path(monkeypatch):
    """2 MiB holding one 64 KiB sample: the host sends that sample to encode6_kernel, which does not count, so the pass
    writes through the scratch and compacts as it always did — whatever the switch says."""
    nat, ora = _models("spec")
    flat, offs = synth.make_corpus(2 << 20, "mixed", seed_offset=78, max_len=2048)
    text = bytes(flat)
    texts = [text[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    at = len(texts) // 2
    long_one = text[: 64 << 10]
    total, k = 0, 0
    while total < (64 << 10):  # (the batch stays at 2 MiB)
        total += len(texts[k])
        k += 1
    texts = texts[k:at] + [long_one] + texts[at:]
    flat, offs = tgx.pack(texts)
    assert abs(int(flat.size) - (2 << 20)) < 8192 and int(np.diff(offs.astype(np.int64)).max()) == 64 << 10
    want = _outcome(lambda: ora.encode_batch_flat(flat, offs, threads=8))
    assert want[0] == "ok"
    check_both_paths(monkeypatch, nat, want, flat, offs, in_place=False)
    assert nat.last_encode_long_samples() >= 1 and "encode6_kernel" in nat.last_kernel_times()
