"""Literal phrase matching on the device (csrc/phrase.hip) on bench.py's mixed corpus resident in HBM, against three sets:
(a) a list of about 400 phrases, half cut from the text and half that never occur; (b) 50 000 phrases of 4 to 24 bytes,
half cut from the text; (c) one phrase of the greatest length, 255 bytes, cut from the text.  For each: the call with
the counts alone and with all three outputs, the stage of tgx_phrase_last_times, GB/s of text, the occurrences found,
and the share of start positions that pass the first-level filter (computed here with torch from the phrases' first
byte pairs, over the flat text: the few starts that are a row's last byte are counted with the next row's first byte).
Set (a) also runs under fold_case and whole_word.

Beside them, from the same process and on the same corpus, for context: gram_hits at width 13 against the grams of a
held-out megabyte, text_stats, and a device-to-device copy of the text.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: phrase_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from layout_bench import _hip, rate
from select_bench import d2d, timed
from textstat_bench import put
from wordstat_bench import staged

STAGES = ("phrase_hits_kernel",)


def cut(flat, rng, n, lo, hi):
    """n slices of lo .. hi bytes of the text, none with a '\\n' (a phrase of a blocklist stays inside a line)"""
    out = []
    while len(out) < n:
        a = int(rng.integers(0, flat.size - hi))
        p = bytes(flat[a:a + int(rng.integers(lo, hi + 1))])
        if b"\n" not in p:
            out.append(p)
    return out


def absent(rng, n, lo, hi):
    """n lower-case phrases with a '~' inside, which the synthetic text does not hold"""
    out = []
    for _ in range(n):
        w = bytearray(rng.integers(97, 123, int(rng.integers(lo, hi + 1))).astype(np.uint8).tobytes())
        w[len(w) // 2] = 126
        out.append(bytes(w))
    return out


def filter_share(d_text, phrases, fold_case):
    """the share of positions whose byte pair begins some phrase (or whose byte is a one-byte phrase)"""
    table = np.zeros(65536, bool)
    for p in phrases:
        p = p.lower() if fold_case else p   # (ASCII phrases here)
        if len(p) == 1:
            table[p[0] * 256:p[0] * 256 + 256] = True
        else:
            table[p[0] * 256 + p[1]] = True
    t = torch.from_numpy(table).cuda()
    n, passed = d_text.shape[0], 0
    for a in range(0, n, 1 << 25):
        b0 = d_text[a:min(a + (1 << 25), n)].to(torch.int64)
        b1 = torch.zeros_like(b0)
        m = min(a + (1 << 25) + 1, n) - (a + 1)
        b1[:m] = d_text[a + 1:a + 1 + m]
        if fold_case:
            b0 = torch.where((b0 >= 65) & (b0 <= 90), b0 | 32, b0)
            b1 = torch.where((b1 >= 65) & (b1 <= 90), b1 | 32, b1)
        passed += int(t[b0 * 256 + b1].sum().item())
    return round(passed / max(n, 1), 6), int(table.sum())


def phrase_run(corpus, d_text, what, phrases, outs, args, stream, fold_case=False, whole_word=False):
    S, N = corpus.num_samples, corpus.num_bytes
    ps = tgx.phrase_set(phrases, fold_case=fold_case, whole_word=whole_word)
    count = torch.empty(S, dtype=torch.int64, device="cuda")
    longest = torch.empty(N, dtype=torch.uint8, device="cuda") if outs == "all" else None
    per = torch.empty(len(phrases), dtype=torch.int64, device="cuda") if outs == "all" else None
    t_call, t_stage = staged(lambda: corpus.phrase_hits(ps, count.data_ptr(), longest.data_ptr() if outs == "all" else 0,
                                                        per.data_ptr() if outs == "all" else 0, stream=stream), args, _lib.phrase_last_times, STAGES)
    rec = {"what": what, "phrases": len(phrases), "distinct": ps.distinct, "max_len": ps.max_len, "table_bytes": ps.table_bytes, "outputs": outs,
           "fold_case": fold_case, "whole_word": whole_word}
    put(rec, "call", t_call)
    for k in STAGES:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(N, t_call["ms"])
    rec["kernel_gb_s"] = rate(N, t_stage[STAGES[0]]["ms"])
    rec["occurrences"] = int(count.sum().item())
    rec["rows_hit"] = int((count > 0).sum().item())
    rec["filter_pass_share"], rec["filter_pairs"] = filter_share(d_text, phrases, fold_case)
    ps.free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("phrase_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        d_text = torch.from_numpy(flat).cuda()
        S, N = corpus.num_samples, corpus.num_bytes
        rng = np.random.default_rng(1234)
        list_a = cut(flat, rng, 200, 6, 20) + absent(rng, 200, 6, 20)
        list_b = cut(flat, rng, 25000, 4, 24) + absent(rng, 25000, 4, 24)
        list_c = cut(flat, rng, 1, 255, 255)
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for what, phrases in (("a_400_phrases", list_a), ("b_50000_phrases", list_b), ("c_one_phrase_of_255", list_c)):
            for outs in ("count", "all"):
                rec["runs"].append(phrase_run(corpus, d_text, what, phrases, outs, args, stream))
        rec["runs"].append(phrase_run(corpus, d_text, "a_400_phrases", list_a, "count", args, stream, fold_case=True))
        rec["runs"].append(phrase_run(corpus, d_text, "a_400_phrases", list_a, "count", args, stream, fold_case=True, whole_word=True))
        # for context, on the same object: gram_hits at width 13, text_stats, a copy of the text
        held, held_offs = synth.make_corpus(1 << 20, "mixed", seed_offset=2000)
        held_out = tgx.NativeCorpus(held, held_offs)
        grams = held_out.gram_set(13, 0, stream=stream)
        g_count = torch.empty(S, dtype=torch.int64, device="cuda")
        t_call, t_stage = staged(lambda: corpus.gram_hits(grams, g_count.data_ptr(), 0, stream=stream), args, _lib.gram_last_times, ("gram_hits_kernel",))
        put(rec, "gram_hits_w13_call", t_call)
        put(rec, "gram_hits_kernel", t_stage["gram_hits_kernel"])
        rec["gram_hits_w13_gb_s"], rec["gram_set_keys"] = rate(N, t_call["ms"]), grams.size
        t_table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
        put(rec, "text_stats_call", timed(lambda: corpus.text_stats(t_table.data_ptr(), 0, 1000, "char", stream=stream), args.steps, args.warmup))
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        for r in rec["runs"]:
            r["call_x_gram_hits_w13"] = round(r["call_ms"] / rec["gram_hits_w13_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        for o in (grams, held_out, corpus):
            o.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
