"""Word ids on the device (csrc/words.hip) on bench.py's mixed corpus resident in HBM: word_rows with and without the
fold, with the stages of tgx_words_last_times.  Beside it, in the same process and on the same object, the yardstick:
word_stats (csrc/wordstat.hip) with counts only and no stop words, which makes the same two walks and one scan; and a
device-to-device copy of the text.

Then the corpus's lines as rows (line_rows' shape: very many short rows, which is what the offsets kernel's serial
rebuild per row has to stand), and the case the design is for: the same bytes as one row without a space byte, one word of the whole corpus, which
must take the time of the many words.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: words_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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
from select_bench import d2d
from textstat_bench import put
from wordstat_bench import staged

STAGES = ("words_summary_kernel", "words_scan", "words_kernel", "words_offsets_kernel")
WS_STAGES = ("wordstat_summary_kernel", "wordstat_scan", "wordstat_kernel")


def words_run(corpus, label, fold, args, stream):
    made = []

    def call():
        made[:] = [corpus.words(_lib.words_flags(fold), 0, stream=stream)]   # (the call before's result goes back to the pool)
    t_call, t_stage = staged(call, args, _lib.words_last_times, STAGES)
    rec = {"what": label, "fold": fold}
    put(rec, "call", t_call)
    for k in STAGES:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(corpus.num_bytes, t_call["ms"])
    rec["words"] = made[0].num_tokens
    made[0].free()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("words_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for fold in (True, False):
            rec["runs"].append(words_run(corpus, "word_rows", fold, args, stream))
        # the yardstick and the floor, on the same object
        table = torch.empty((_lib.WORDSTAT_N, S), dtype=torch.int64, device="cuda")
        t_call, t_stage = staged(lambda: corpus.word_stats(table.data_ptr(), 0, 20, (), "byte", False, stream=stream), args, _lib.wordstat_last_times, WS_STAGES)
        put(rec, "word_stats_call", t_call)
        for k in WS_STAGES:
            put(rec, k, t_stage[k])
        rec["word_stats_words"] = int(table[0].sum().item())
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        for r in rec["runs"]:
            r["call_x_word_stats"] = round(r["call_ms"] / rec["word_stats_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        # very many short rows: the corpus's lines as rows (the offsets kernel rebuilds up to 63 bytes a row)
        lines = corpus.lines(stream=stream)
        r = words_run(lines, "lines_as_rows", True, args, stream)
        r["rows"] = lines.num_samples
        r["call_x_word_rows"] = round(r["call_ms"] / rec["runs"][0]["call_ms"], 3)
        rec["runs"].append(r)
        lines.free()
        corpus.free()
        # one row that is one word
        spaces = (flat == 32) | ((flat >= 9) & (flat <= 13))
        c = tgx.NativeCorpus(np.where(spaces, np.uint8(95), flat), np.asarray([0, flat.size], np.uint64))
        r = words_run(c, "one_row_one_word", True, args, stream)
        r["call_x_word_rows"] = round(r["call_ms"] / rec["runs"][0]["call_ms"], 3)
        rec["runs"].append(r)
        c.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
