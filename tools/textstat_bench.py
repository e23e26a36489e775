"""Per-row text statistics and the line view on the device (csrc/textstat.hip) on bench.py's mixed corpus resident in HBM:
text_stats under both units, with and without the line-start mask, and line_rows' corpus (NativeCorpus.lines), with the
stages of tgx_textstat_last_times.  Beside them, in the same process and on the same object, two floors that read the
same bytes:

  (a) row_hashes, which reads the text once and hashes it;
  (b) a device-to-device copy of the text.

Then the design condition, that a line's length does not enter the time: the same corpus with every '\\n' replaced by a
space, so that each row is one line, and one row of the same size with no '\\n' at all.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: textstat_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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

STAGES = ("textstat_summary_kernel", "textstat_scan", "textstat_kernel", "textstat_lines")


def staged(call, args):
    """call() timed, with the stages of tgx_textstat_last_times of the timed calls -> (call's spread, {stage: spread})"""
    seen = {k: [] for k in STAGES}

    def fn():
        call()
        t = _lib.textstat_last_times()
        for k in STAGES:
            seen[k].append(t[k])
    t_call = timed(fn, args.steps, args.warmup)
    return t_call, {k: spread(v[-args.steps:]) for k, v in seen.items()}


def put(out, name, s):
    out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]


def stats_run(corpus, label, unit, with_mask, args, stream):
    S, N = corpus.num_samples, corpus.num_bytes
    table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
    marks = torch.empty(N, dtype=torch.uint8, device="cuda") if with_mask else None
    t_call, t_stage = staged(lambda: corpus.text_stats(table.data_ptr(), marks.data_ptr() if with_mask else 0, 1000, unit, stream=stream), args)
    rec = {"what": label, "unit": unit, "mask": with_mask}
    put(rec, "call", t_call)
    for k in STAGES[:3]:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(N, t_call["ms"])
    rec["lines"] = int(table[3].sum().item())
    rec["max_line"] = int(table[4].max().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("textstat_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for unit in ("char", "byte"):
            for with_mask in (False, True):
                rec["runs"].append(stats_run(corpus, "text_stats", unit, with_mask, args, stream))
        made = {}

        def lines():
            if "c" in made:
                made["c"].free()
            made["c"] = corpus.lines(stream=stream)
        t_call, t_stage = staged(lines, args)
        put(rec, "lines_call", t_call)
        for k in STAGES:
            put(rec, "lines_" + k, t_stage[k])
        rec["n_lines"] = made["c"].num_samples
        made["c"].free()
        # the floors, on the same object
        d_hash = torch.empty(S, dtype=torch.int64, device="cuda")
        put(rec, "row_hashes_call", timed(lambda: corpus.row_hashes(d_hash.data_ptr(), 0, stream=stream), args.steps, args.warmup))
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        for r in rec["runs"]:
            r["call_x_row_hashes"] = round(r["call_ms"] / rec["row_hashes_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        corpus.free()
        # long lines: every row one line, then one row that is one line
        one_line_rows = np.where(flat == 10, np.uint8(32), flat)
        for label, f, o in (("rows_of_one_line", one_line_rows, offs), ("one_row_one_line", one_line_rows, np.asarray([0, flat.size], np.uint64))):
            c = tgx.NativeCorpus(f, o)
            r = stats_run(c, label, "char", False, args, stream)
            r["call_x_text_stats"] = round(r["call_ms"] / rec["runs"][0]["call_ms"], 3)
            rec["runs"].append(r)
            c.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
