"""Per-row word statistics on the device (csrc/wordstat.hip) on bench.py's mixed corpus resident in HBM: word_stats with
0, 8 and 63 stop words, with and without the marks, with the stages of tgx_wordstat_last_times.  Beside them, in the same
process and on the same object: text_stats (csrc/textstat.hip, whose walk the kernels share), row_hashes, which reads
the text once and hashes it, and a device-to-device copy of the text.

Then the same-address case: one row of the same size without a space byte, so that every chunk of the corpus adds its
part of one word onto the same words of the table.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: wordstat_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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
from select_bench import d2d, spread, timed
from textstat_bench import put

STAGES = ("wordstat_summary_kernel", "wordstat_scan", "wordstat_kernel")


def stop_table(n):
    """n stop words: Gopher's eight first, then three-letter words that are none of them"""
    more = [bytes([97 + k % 26, 97 + (7 * k) % 26, 120 + k // 26]) for k in range(64)]
    return (list(_lib.GOPHER_STOP_WORDS) + more)[:n]


def staged(call, args, last_times, stages):
    """call() timed, with the stages of the timed calls -> (call's spread, {stage: spread})"""
    seen = {k: [] for k in stages}

    def fn():
        call()
        t = last_times()
        for k in stages:
            seen[k].append(t[k])
    t_call = timed(fn, args.steps, args.warmup)
    return t_call, {k: spread(v[-args.steps:]) for k, v in seen.items()}


def words_run(corpus, label, n_stop, with_marks, args, stream):
    S, N = corpus.num_samples, corpus.num_bytes
    table = torch.empty((_lib.WORDSTAT_N, S), dtype=torch.int64, device="cuda")
    marks = torch.empty(N, dtype=torch.uint8, device="cuda") if with_marks else None
    stops = stop_table(n_stop)
    t_call, t_stage = staged(lambda: corpus.word_stats(table.data_ptr(), marks.data_ptr() if with_marks else 0, 20, stops, "char", True, stream=stream), args,
                             _lib.wordstat_last_times, STAGES)
    rec = {"what": label, "stop_words": n_stop, "marks": with_marks}
    put(rec, "call", t_call)
    for k in STAGES:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(N, t_call["ms"])
    rec["words"] = int(table[0].sum().item())
    rec["max_word"] = int(table[2].max().item())
    rec["stop_word_ends"] = int(table[12].sum().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("wordstat_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for n_stop, with_marks in ((0, False), (8, False), (63, False), (8, True)):
            rec["runs"].append(words_run(corpus, "word_stats", n_stop, with_marks, args, stream))
        # text_stats and the floors, on the same object
        t_table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
        ts_stages = ("textstat_summary_kernel", "textstat_scan", "textstat_kernel")
        t_call, t_stage = staged(lambda: corpus.text_stats(t_table.data_ptr(), 0, 1000, "char", stream=stream), args, _lib.textstat_last_times, ts_stages)
        put(rec, "text_stats_call", t_call)
        for k in ts_stages:
            put(rec, k, t_stage[k])
        d_hash = torch.empty(S, dtype=torch.int64, device="cuda")
        put(rec, "row_hashes_call", timed(lambda: corpus.row_hashes(d_hash.data_ptr(), 0, stream=stream), args.steps, args.warmup))
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        for r in rec["runs"]:
            r["call_x_text_stats"] = round(r["call_ms"] / rec["text_stats_call_ms"], 2)
            r["call_x_row_hashes"] = round(r["call_ms"] / rec["row_hashes_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        corpus.free()
        # the same-address case: one row that is one word
        spaces = (flat == 32) | ((flat >= 9) & (flat <= 13))
        c = tgx.NativeCorpus(np.where(spaces, np.uint8(95), flat), np.asarray([0, flat.size], np.uint64))
        r = words_run(c, "one_row_one_word", 8, False, args, stream)
        r["call_x_word_stats"] = round(r["call_ms"] / rec["runs"][1]["call_ms"], 3)
        rec["runs"].append(r)
        c.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
