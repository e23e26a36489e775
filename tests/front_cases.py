"""The fixed cases of the device front end (tgx_corpus_split_specials / tgx_front_host): batches whose special tokens, sample
ends and "\\r\\n" pairs sit where the kernels' tiles (T bytes) and thread slots (16 bytes) end, and the overlap and CRLF
cases of the split rule.  test_front_cpu.py runs them through the host twin, test_front_gpu.py through the kernels; the
ground truth of both is split_specials_flat + pack_segments on the host."""
import functools

import numpy as np

from tokengeex_amd import _lib

T = 4096          # csrc/front.h: kFrontTile
SP = b"<|special|>"
M = len(SP)


def truth(samples, specials, crlf):
    """-> (seg_offs, seg_special, segments' flat, segments' offsets) of the host route"""
    flat, offs = _lib.pack(samples)
    return truth_flat(flat, offs, specials, crlf)


def truth_flat(flat, offs, specials, crlf):
    """truth() of a packed batch"""
    flat = np.ascontiguousarray(flat)
    seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, specials)
    pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
    return seg_offs, ss, pflat, poffs


def segments(samples, specials, crlf=False):
    """the host route's split as a list of (bytes, special index or -1) per sample: what a case states in words"""
    seg_offs, ss, pflat, poffs = truth(samples, specials, crlf)
    raw, e, out = pflat.tobytes(), 0, []
    for i in range(len(samples)):
        row = []
        for k in range(int(seg_offs[i]), int(seg_offs[i + 1])):
            if ss[k] >= 0:
                row.append((specials[ss[k]], int(ss[k])))
            else:
                row.append((raw[int(poffs[e]):int(poffs[e + 1])], -1))
                e += 1
        out.append(row)
    return out


def _filler(n, salt=0):
    return bytes(97 + (i * 7 + salt) % 23 for i in range(n))


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """-> list of (name, samples, specials); every case runs with the CRLF pass on and off"""
    cases = []
    # a special starting at every offset T-M .. T+1 of a tile (and of the second tile's end), so that it straddles the boundary at each split point
    for base in (T, 2 * T):
        for o in range(base - M, base + 2):
            cases.append((f"straddle_{o}", [_filler(o) + SP + _filler(40, 3)], [SP]))
    cases.append(("straddle_two_samples", [_filler(T - 5) + SP[:5], SP[5:] + _filler(30), _filler(T - 40) + SP], [SP]))
    # sample i ends with each proper prefix of a special, sample i+1 starts with the rest: no match
    for j in range(1, M):
        cases.append((f"prefix_across_samples_{j}", [b"ab" + SP[:j], SP[j:] + b"cd"], [SP]))
        cases.append((f"prefix_across_samples_at_tile_end_{j}", [_filler(T - j) + SP[:j], SP[j:] + b"cd"], [SP]))
    cases.append(("complete_at_end_and_start", [b"ab" + SP, SP + b"cd", SP, SP + SP], [SP]))
    cases.append(("list_order_short_first", [b"x<abx"], [b"<a", b"<ab"]))
    cases.append(("list_order_long_first", [b"x<abx"], [b"<ab", b"<a"]))
    nine = [b"<%d>" % k for k in range(9)]
    cases.append(("first_byte_shared_by_nine", [b"a<0>b<8><7>c<9><3", b"<4><5>x<6<1>", b"<2>"], nine))
    cases.append(("first_byte_shared_longer_later", [b"<|a<|ab|><|a|>", b"<|"], [b"<|a|>", b"<|ab|>", b"<|a", b"<|", b"<"]))
    cases.append(("multibyte_lead", ["caféé<x>é è<x>".encode(), "é".encode()], ["é<x>".encode(), "€".encode()]))
    cases.append(("invalid_utf8", [b"\xfe\x80<s>\xc3", b"\xc3<s>\xa9\xf0\x9f", b"\x80\x80"], [b"<s>", b"\xc3\xa9"]))
    cases.append(("overlap_aa_on_runs", [b"a" * n for n in range(0, 12)] + [b"xaaaaax", b"aaa" + b"b" + b"aaaa"], [b"aa"]))
    cases.append(("overlap_aba", [b"ababababa"], [b"aba"]))
    cases.append(("overlap_ab_ba", [b"ababa", b"babab"], [b"ab", b"ba"]))
    cases.append(("overlap_ba_ab", [b"ababa", b"babab"], [b"ba", b"ab"]))
    cases.append(("overlap_run_across_tiles", [b"a" * (3 * T + 1)], [b"aa"]))
    cases.append(("overlap_run_across_tiles_aaa", [b"b" + b"a" * (2 * T + 5), b"a" * 7], [b"aaa", b"a"]))
    cases.append(("empty_samples", [b"", b"", b"x<s>y", b"", b"", b"", b"<s>", b"z", b""], [b"<s>"]))
    cases.append(("only_empty_samples", [b"", b"", b""], [b"<s>"]))
    cases.append(("sample_is_one_special", [b"<s>", b"a", b"</s>"], [b"<s>", b"</s>"]))
    cases.append(("only_specials_adjacent", [b"<s><s></s><s>", b"</s></s>"], [b"<s>", b"</s>"]))
    cases.append(("no_special_anywhere", [_filler(5000), _filler(17, 2), b"", _filler(4096, 5)], [b"<s>", b"</s>"]))
    cases.append(("no_specials_in_the_list", [_filler(5000) + b"\r\n", b"", b"\r\nab\r", b"\n", _filler(33)], []))
    body = bytearray()
    for k in range(70_000 // 64 + 1):
        body += _filler(64 - M, k) + SP
    cases.append(("special_every_64_bytes", [bytes(body[:70_000])], [SP]))
    cases.append(("mixed_corpus_with_specials", _mixed_with_specials(), [b"<|endoftext|>", b"<|fim", b"<|fim|>", b"<pad>", b"<s>", b"</s>"]))
    # CRLF
    cases.append(("crlf_cr_last_byte_of_tile", [_filler(T - 1) + b"\r\n" + _filler(20), _filler(T - 2) + b"\r\n\r\n"], [b"<s>"]))
    cases.append(("crlf_cr_last_byte_of_slot", [_filler(15) + b"\r\n" + _filler(14) + b"\r\r\n\n\r"], [b"<s>"]))
    cases.append(("crlf_runs", [b"a\r\r\nb", b"\r\n\r\n", b"a\rb", b"\r", b"\n\r", b"\r\r\r\n\n"], [b"<s>"]))
    cases.append(("crlf_cr_ends_segment_before_special", [b"ab\r\n<x>cd", b"\r\n<x>", b"\r\r\n<x>\r\n"], [b"\n<x>"]))
    cases.append(("crlf_across_samples", [b"ab\r", b"\ncd", b"\r", b"\n"], [b"<s>"]))
    cases.append(("crlf_inside_special", [b"a<\r\n>b\r\n<\r\n>", b"<\r\n", b">"], [b"<\r\n>"]))
    return cases


def _mixed_with_specials():
    """test_assemble_gpu.py's mixed corpus (samples of up to 4 KiB, one of 70 000 bytes, empty samples at the start, in the
    middle and at the end) with special tokens written into the samples"""
    from tokengeex_amd import synth
    flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
    big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
    rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
    half = len(rows) // 2
    rows = [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]
    out = []
    for k, t in enumerate(rows):
        cut = len(t) // 3
        if not t:
            out.append(t)
        elif k % 4 == 0:
            out.append(t)
        else:
            out.append(t[:cut] + b"<|fim|>" + t[cut:2 * cut] + b"<s>" * (k % 3) + b"\r\n" + t[2 * cut:] + (b"<|endoftext|>" if k % 2 else b""))
    return out


def random_batch(rng, max_bytes=64 << 10):
    """a small batch whose sample ends and special tokens sit around the tile edges -> (samples, specials)"""
    alphabet = b"ab<>\r\n|x"
    n_sp = int(rng.integers(0, 7))
    specials = []
    for _ in range(n_sp):
        n = int(rng.integers(1, 7))
        specials.append(bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n)))
    samples, total = [], 0
    for _ in range(int(rng.integers(0, 9))):
        kind = int(rng.integers(0, 6))
        n = [0, int(rng.integers(1, 40)), T - total % T - int(rng.integers(0, 8)), T + int(rng.integers(-3, 4)), int(rng.integers(1, 3 * T)),
             int(rng.integers(1, 300))][kind]
        n = max(0, min(n, max_bytes - total))
        body = bytearray(alphabet[int(x)] for x in rng.integers(0, len(alphabet), n))
        if specials and n:   # and whole specials, some right at the sample's end
            for _ in range(int(rng.integers(0, 4))):
                sp = specials[int(rng.integers(0, len(specials)))]
                at = int(rng.integers(0, n))
                body[at:at + len(sp)] = sp
            body = body[:n]
        samples.append(bytes(body))
        total += len(body)
    return samples, specials


# ---- one corpus past the caps of csrc/front.hip's grids -----------------------------------------------------------------

CAP = 4096            # csrc/front.hip: kFrontMaxBlocks, of the kernels over tiles and of those over candidates, samples and segments
BLOCK = 256           # csrc/front.hip: kFrontBlock, items per block of the kernels with a thread per candidate, sample or segment
PAST_SPECIALS = [SP, b"<s>", b"</s>", b"aa"]
# the short rows, cycled: a row that is one special, empty rows, overlapping candidates ("aa" on a run), a prefix of a special
# at a row's end, a special in text, "\r\n" inside a row and with a row's end between the two, specials back to back, and a
# row of 102 bytes.  167 bytes, 13 rows, 14 accepted candidates and 11 segments to encode a round; 167 is odd, so over the rounds every row begins at every
# byte of a 16-byte slot and of a tile: the specials straddle the slots' and tiles' edges at every split, and so do the "\r\n"
PAST_POOL = (b"<s>", b"", b"aaaa", b"x<s", b"bc" + SP + b"d", b"e\r\nf\r", b"\n<s></s>", b"", SP, b"aaab", b"<s>aa<s", b"q<s>\r\n",
             bytes(98 + (i * 7) % 20 for i in range(47)) + SP + bytes(98 + (i * 5) % 20 for i in range(44)))


@functools.lru_cache(maxsize=None)
def past_cap_corpus():
    """-> (flat, offs, specials): the short rows of PAST_POOL over the first 4096·4096 bytes and a little more, so that the
    kernels over tiles (front_mark, front_candidates, front_keep, front_pack) go round twice, with over 256·4096 rows and
    over 256·4096 candidates, segments and segments to encode, so that the kernels with a thread per one of these do too.  Behind them, in
    the second trip's tiles, two rows of three tiles each: one without a byte that begins a special (tiles without a
    candidate: front_candidates_kernel's `continue`) and one of 4096 "<s>" (tiles of which nothing is kept:
    front_pack_kernel's), then a round of the short rows."""
    unit = np.frombuffer(b"".join(PAST_POOL), np.uint8)
    unit_lens = np.asarray([len(r) for r in PAST_POOL], np.int64)
    reps = CAP * T // unit.size + 8
    plain = np.frombuffer(bytes(98 + (i * 7) % 20 for i in range(3 * T)), np.uint8)
    only = np.frombuffer(b"<s>" * T, np.uint8)
    flat = np.concatenate([np.tile(unit, reps), plain, only, unit])
    lens = np.concatenate([np.tile(unit_lens, reps), [plain.size, only.size], unit_lens])
    offs = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    for a in (flat, offs):
        a.setflags(write=False)
    return flat, offs, list(PAST_SPECIALS)
