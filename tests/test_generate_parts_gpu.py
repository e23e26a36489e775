"""The raw interface of the document-frequency pass (tgx_substring_df, tgx_substring_df_top; csrc/generate.hip) on the part
geometries of tests/generate_cases.py against the brute-force enumeration there: the table of each block's first part,
parts against the blocks of 256 positions, several parts of one sample, part_origin, multi-byte characters at the limits,
the top-k cut through ties.  Every comparison is ==; no expected value comes from the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import generate_cases as gc


def _table(c, pos, ln, df):
    """The device's entries as {substring: df}; one entry per distinct substring, each inside the text."""
    text = c["text"]
    assert pos.size == ln.size == df.size
    assert all(int(p) + int(l) <= len(text) for p, l in zip(pos, ln))
    got = {text[int(p):int(p) + int(l)]: int(d) for p, l, d in zip(pos, ln, df)}
    assert len(got) == pos.size, "a substring came back twice"
    return got


def _df(c, mtl, prob=1.0, seed=0, **kw):
    flat, pb, pe, ps, po = gc.arrays(c)
    return _lib.substring_df(flat, pb, pe, ps, mtl, prob, seed, part_origin=po, **kw)


def _df_top(c, mtl, k, prob=1.0, seed=0):
    flat, pb, pe, ps, po = gc.arrays(c)
    return _lib.substring_df_top(flat, pb, pe, ps, mtl, k, prob, seed, part_origin=po)


@pytest.mark.parametrize("name", gc.GEOMETRY_NAMES)
def test_geometry(name):
    c = gc.case(name)
    for mtl in gc.MTLS:
        for prob, seed in ((1.0, 0), (0.3, 9)):
            want, want_windows = gc.brute_force(c["text"], c["parts"], c["origin"], mtl, prob, seed)
            pos, ln, df, n_windows = _df(c, mtl, prob, seed)
            assert n_windows == want_windows, (name, mtl, prob)
            assert _table(c, pos, ln, df) == want, (name, mtl, prob)
            if mtl < 32:
                assert int(ln.max(initial=0)) <= mtl
    if name == "no_position_inside_a_part":
        pos, ln, df, n_windows = _df(c, 32)
        assert pos.size == 0 and n_windows == 0


def test_invalid_parts_are_refused():
    c = gc.case("sample_ids")
    flat, pb, pe, ps, _ = gc.arrays(c)

    def refused(pb, pe, ps, po=None):
        for call in (lambda: _lib.substring_df(flat, pb, pe, ps, 8, part_origin=po), lambda: _lib.substring_df_top(flat, pb, pe, ps, 8, 5, part_origin=po)):
            with pytest.raises(tgx.TokenGeeXError) as e:
                call()
            assert e.value.status == _lib.ERR_INVALID, e.value

    big = ps.astype(np.uint64)
    big[-1] = 1 << 27
    refused(pb, pe, big.astype(np.uint32))                                  # the sample id 2^27
    refused(pb[::-1].copy(), pe[::-1].copy(), ps)                           # unsorted
    refused(pb[[1, 0, 2, 3]], pe[[1, 0, 2, 3]], ps)
    over = pb.copy()
    over[1] = pe[0] - 1
    refused(over, pe, ps)                                                   # overlapping
    down = ps.copy()
    down[1], down[2] = 5, 4
    refused(pb, pe, down)                                                   # descending sample ids
    end = pe.copy()
    end[-1] = flat.size + 1
    refused(pb, end, ps)                                                    # beyond the text
    origin = pb.copy()
    origin[2] = pb[2] + 1
    refused(pb, pe, ps, origin)                                             # a part_origin beyond its part's begin
    origin[2] = pb[2]                                                       # ... and at its begin it is accepted
    pos, ln, df, _ = _lib.substring_df(flat, pb, pe, ps, 8, part_origin=origin)
    assert _table(c, pos, ln, df) == gc.brute_force(c["text"], c["parts"], None, 8)[0]


def test_placement_invariance():
    """The same samples tight at the start of the buffer, at other offsets with filler between them, and in two calls with
    their global sample ids: the same strings and frequencies at insert probability 0.3, those of the brute force."""
    mtl, prob, seed = gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED
    tight = gc.place(range(6), 0, 0)
    want, want_windows = gc.brute_force(tight["text"], tight["parts"], tight["origin"], mtl, prob, seed)
    for c in (tight, gc.place(range(6), 300, 517), gc.place(range(6), 255, 1), gc.place(range(6), 1, 256)):
        pos, ln, df, n_windows = _df(c, mtl, prob, seed)
        assert _table(c, pos, ln, df) == want and n_windows == want_windows, c["name"]
    for cut in (1, 3, 5):
        total, windows = {}, 0
        for which, lead, gap in ((range(cut), 0, 0), (range(cut, 6), 77, 300)):
            c = gc.place(which, lead, gap)
            pos, ln, df, n_windows = _df(c, mtl, prob, seed)
            part = _table(c, pos, ln, df)
            assert (part, n_windows) == gc.brute_force(c["text"], c["parts"], c["origin"], mtl, prob, seed)
            for sub, d in part.items():
                total[sub] = total.get(sub, 0) + d
            windows += n_windows
        assert total == want and windows == want_windows, cut


@pytest.mark.parametrize("name,mtl", [("utf8", 7), ("gaps", 7), ("once_per_sample", 4), ("300_one_byte_parts", 1), ("sample_ids", 32)])
def test_top_k(name, mtl):
    c = gc.case(name)
    want, want_windows = gc.brute_force(c["text"], c["parts"], c["origin"], mtl)
    ks = gc.top_ks(want)
    assert "tie" in ks or name == "300_one_byte_parts"
    for kind, k in ks.items():
        pos, ln, df, n_windows, n_distinct, cutoff = _df_top(c, mtl, k)
        got = _table(c, pos, ln, df)
        top, cut = gc.top_expectation(want, k)
        assert n_distinct == len(want) and n_windows == want_windows, (kind, k)
        assert sorted(df.tolist(), reverse=True) == top, (kind, k)          # the k largest frequencies
        assert k >= len(want) or df.tolist() == top, (kind, k)              # ... in descending order when something is cut
        assert all(want.get(sub) == d for sub, d in got.items()), (kind, k)  # every returned string with its exact frequency
        assert cutoff == cut, (kind, k, cutoff, cut)


def test_forced_collisions_give_the_same_counts(monkeypatch):
    """TGX_GENERATE_COLLIDE=4: the first attempt sorts by 4 bits of the keys, so different substrings share runs, are told
    apart byte by byte, and the pass is sorted again under another hash."""
    monkeypatch.setenv("TGX_GENERATE_COLLIDE", "4")
    for name, mtl in (("one_part_over_three_blocks", 7), ("utf8", 5)):
        c = gc.case(name)
        want, want_windows = gc.brute_force(c["text"], c["parts"], c["origin"], mtl)
        pos, ln, df, n_windows, collisions = _df(c, mtl, with_collisions=True)
        assert _table(c, pos, ln, df) == want and n_windows == want_windows and collisions > 0
    monkeypatch.delenv("TGX_GENERATE_COLLIDE")
    pos, ln, df, n_windows, collisions = _df(c, mtl, with_collisions=True)
    assert _table(c, pos, ln, df) == want and collisions == 0
