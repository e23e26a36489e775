"""What tests/test_generate_parts_gpu.py relies on, established without a GPU: the brute-force reference of
tests/generate_cases.py against hand-counted frequencies and against the oracle's VocabularyGenerator, and every case on
the edge it is named for."""
import re

import pytest

from oracle.generate_oracle import OracleVocabularyGenerator

import generate_cases as gc


def test_brute_force_by_hand():
    text = b"abab" + b"ab" + b"xyz"
    parts = [(0, 4, 0), (4, 6, 1), (6, 9, 3)]
    df, n = gc.brute_force(text, parts, None, 4)
    assert df == {b"a": 2, b"b": 2, b"ab": 2, b"ba": 1, b"aba": 1, b"bab": 1, b"abab": 1, b"x": 1, b"y": 1, b"z": 1, b"xy": 1, b"yz": 1,
                  b"xyz": 1} and n == 10 + 3 + 6
    # characters: "中文中" at mtl 4 has no pair (6 bytes), at mtl 6 it has; a part that ends inside a character keeps the cut window
    t = "中文中".encode()
    assert gc.brute_force(t, [(0, 9, 0)], None, 4) == ({"中".encode(): 1, "文".encode(): 1}, 3)
    assert set(gc.brute_force(t, [(0, 9, 0)], None, 6)[0]) == {"中".encode(), "文".encode(), "中文".encode(), "文中".encode()}
    assert gc.brute_force(t, [(0, 4, 0)], None, 4) == ({t[:3]: 1, t[3:4]: 1, t[:4]: 1}, 3)
    assert gc.brute_force(t, [(1, 3, 0)], None, 4) == ({}, 0)
    # two parts of one sample count once, two samples twice
    assert gc.brute_force(b"ab-ab", [(0, 2, 0), (3, 5, 0)], None, 2) == ({b"a": 1, b"b": 1, b"ab": 1}, 6)
    assert gc.brute_force(b"ab-ab", [(0, 2, 0), (3, 5, 1)], None, 2) == ({b"a": 2, b"b": 2, b"ab": 2}, 6)


@pytest.mark.parametrize("prob,seed", [(1.0, 0), (0.3, 5)])
def test_brute_force_equals_the_oracle_generator(prob, seed):
    """Whole samples, and the parts of a split pattern with their origins, against VocabularyGenerator::feed restated
    (oracle/generate_oracle.py) — sample ids 0, 1, ... as the generator numbers them."""
    samples = [gc.make_text(n, 50 + n).decode("utf-8", "ignore") for n in (40, 100, 257, 300)] + ["", "中文中文", "é" * 9, "𝒳𝒴 ab"]
    split = re.compile(r"[^ ]+")
    for mtl in (1, 4, 7, 32):
        for use_split in (False, True):
            ora = OracleVocabularyGenerator(mtl, prob, split if use_split else None, None, seed=seed)
            ora.feed(samples)
            buf, parts, origin = bytearray(), [], []
            for i, s in enumerate(samples):
                at, b = len(buf), s.encode()
                if use_split:
                    for m in split.finditer(s):
                        parts.append((at + len(s[:m.start()].encode()), at + len(s[:m.end()].encode()), i))
                        origin.append(at)
                elif b:
                    parts.append((at, at + len(b), i))
                    origin.append(at)
                buf += b + b"\n"
            df, _ = gc.brute_force(bytes(buf), parts, origin, mtl, prob, seed)
            assert {k.decode(): v for k, v in df.items()} == ora.frequencies, (mtl, use_split)


def _blocks(b, e):
    return set(range(b // gc.BLOCK, (e - 1) // gc.BLOCK + 1)) if e > b else set()


def test_geometry_cases_sit_on_their_edges():
    assert tuple(c["name"] for c in gc.geometry_cases()) == gc.GEOMETRY_NAMES
    for c in gc.geometry_cases():
        parts, n = c["parts"], len(c["text"])
        assert n <= 4096
        for k, (b, e, s) in enumerate(parts):  # what tgx_substring_df accepts
            assert 0 <= b <= e <= n and 0 <= s <= gc.MAX_SAMPLE
            assert k == 0 or (b >= parts[k - 1][1] and s >= parts[k - 1][2])
    c = gc.case("on_block_boundaries")
    assert all(b % 256 == 0 and e % 256 == 0 for b, e, _ in c["parts"])
    c = gc.case("one_part_over_three_blocks")
    assert len(c["parts"]) == 1 and _blocks(*c["parts"][0][:2]) == {0, 1, 2}
    c = gc.case("300_one_byte_parts")
    assert len(c["parts"]) == 300 > gc.BLOCK and all(e == b + 1 for b, e, _ in c["parts"])
    assert all(c["parts"][i][1] == c["parts"][i + 1][0] for i in range(299)) and len({s for _, _, s in c["parts"]}) == 100
    c = gc.case("gaps")
    gaps = [c["parts"][i + 1][0] - c["parts"][i][1] for i in range(len(c["parts"]) - 1)]
    assert sum(g > 512 for g in gaps) >= 2 and c["parts"][-1][1] == len(c["text"])
    covered = set().union(*(_blocks(b, e) for b, e, _ in c["parts"]))
    assert any(blk not in covered and blk + 1 not in covered for blk in range(7))   # blocks without any part
    for n in (512, 513, 511):
        c = gc.case(f"last_part_ends_at_{n}")
        assert len(c["text"]) == n == c["parts"][-1][1]
    assert {len(gc.case(f"last_part_ends_at_{n}")["text"]) % 256 for n in (512, 513, 511)} == {0, 1, 255}
    c = gc.case("no_position_inside_a_part")
    assert all(not gc.is_start(c["text"], p) for b, e, _ in c["parts"] for p in range(b, e)) and any(e > b for b, e, _ in c["parts"])
    assert all(gc.brute_force(c["text"], c["parts"], None, m) == ({}, 0) for m in gc.MTLS)
    c = gc.case("once_per_sample")
    df, _ = gc.brute_force(c["text"], c["parts"], None, 7)
    assert df[b"abcabc"] == 2 and df[b"bca"] == 2 and [s for _, _, s in c["parts"]] == [3, 3, 4, 4]
    c = gc.case("sample_ids")
    assert {s for _, _, s in c["parts"]} == {0, 5, (1 << 27) - 1}


def test_utf8_case_sits_on_its_edges():
    c = gc.case("utf8")
    text, parts = c["text"], c["parts"]
    inside = lambda p: any(b <= p < e for b, e, _ in parts)
    # a character of every width straddles a block boundary, inside a part
    for start, width in ((255, 2), (510, 3), (766, 4)):
        assert gc.is_start(text, start) and all(not gc.is_start(text, start + i) for i in range(1, width)) and gc.is_start(text, start + width)
        assert start // 256 != (start + width - 1) // 256 and inside(start) and inside(start + width - 1)
        text[start:start + width].decode()
    # windows that end, with a multi-byte character, exactly at mtl bytes
    for mtl, want in ((4, "abé"), (5, "ab中"), (7, "abc𝒳"), (32, "abcd" * 7 + "𝒳"), (32, "abcd" * 7 + "ab" + "é"), (32, "abcd" * 7 + "a" + "中")):
        df, _ = gc.brute_force(text, parts, None, mtl)
        assert len(want.encode()) == mtl and want.encode() in df
        assert want.encode() not in gc.brute_force(text, parts, None, mtl - 1)[0]
    # parts that end inside a character: the cut window is kept (it ends at the part's end), the whole character is not there
    for (b, e, s), ch in zip(parts[2:5], (gc.E2, gc.E3, gc.E4)):
        assert not gc.is_start(text, e)
        start = max(p for p in range(b, e) if gc.is_start(text, p))
        assert text[start:start + len(ch)] == ch and start + len(ch) > e
        df, _ = gc.brute_force(text, [(b, e, s)], None, 32)
        assert text[start:e] in df and ch not in df
    # at mtl 1 no multi-byte character gives a window, except cut ones
    df, _ = gc.brute_force(text, parts, None, 1)
    assert all(len(k) == 1 for k in df) and gc.E2[:1] in df


def test_placement_cases():
    samples = gc.placement_samples()
    assert len(samples) == len(gc.PLACE_IDS) and all(len(parts) >= 5 for _, parts in samples)
    a, b = gc.place(range(6), 0, 0), gc.place(range(6), 300, 517)
    assert len(a["parts"]) == len(b["parts"]) and a["text"] != b["text"] and max(len(a["text"]), len(b["text"])) < 8192
    assert any(o < p[0] for o, p in zip(b["origin"], b["parts"])) and {o % 256 for o in a["origin"]} != {o % 256 for o in b["origin"]}
    want = gc.brute_force(a["text"], a["parts"], a["origin"], gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED)
    assert gc.brute_force(b["text"], b["parts"], b["origin"], gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED) == want
    full = gc.brute_force(a["text"], a["parts"], a["origin"], gc.PLACE_MTL)
    assert 0.2 * full[1] < want[1] < 0.4 * full[1] and 0 < len(want[0]) < len(full[0])   # the keep rule really thins
    # without the origins the draws differ: the origin matters
    assert gc.brute_force(b["text"], b["parts"], None, gc.PLACE_MTL, gc.PLACE_PROB, gc.PLACE_SEED) != want


def test_top_k_cuts_through_a_tie():
    for name in ("utf8", "gaps"):
        c = gc.case(name)
        df, _ = gc.brute_force(c["text"], c["parts"], c["origin"], 7)
        ks = gc.top_ks(df)
        d = sorted(df.values(), reverse=True)
        assert set(ks) == {"1", "tie", "n-1", "n", "n+1"} and d[ks["tie"] - 1] == d[ks["tie"]] > d[-1]
        assert gc.top_expectation(df, ks["tie"]) == (d[:ks["tie"]], d[ks["tie"]]) and gc.top_expectation(df, len(d))[1] == 0
    assert gc.top_expectation({b"a": 3, b"b": 1, b"c": 3}, 1) == ([3], 3) and gc.top_expectation({b"a": 3}, 2) == ([3], 0)
