"""Shapes on the device (csrc/shape.hip) on bench.py's mixed corpus resident in HBM: shape_hits and shape_cover with
`AKIA[0-9A-Z]{16}` alone (20 positions: one 64-bit word, NW = 1) and with a guarded `[0-9a-f]{32}` beside
`ghp_[0-9a-zA-Z]{36}` (72 positions: two words, NW = 2), with the stages of tgx_shapes_last_times.  Beside them, in the same
process and on the same object, the yardsticks: pattern_hits with the e-mail pattern (csrc/dfa.hip: a summary kernel, a
scan and a second kernel where the shapes take one), text_stats (csrc/textstat.hip, whose walk the kernels share), and a
device-to-device copy.

Then the same bytes as one row without a newline, which must take the time of the many rows.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: shapes_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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
from patterns_bench import PATTERNS, dfa_run
from select_bench import d2d
from textstat_bench import put
from wordstat_bench import staged

STAGES = ("shape_ends_kernel", "shape_cover_kernel")
HEX = "[0-9a-f]"
SHAPES = {"akia": ["AKIA[0-9A-Z]{16}"], "hex32+ghp": [(HEX + "{32}", HEX, HEX), "ghp_[0-9a-zA-Z]{36}"]}


def shape_run(corpus, label, name, cover, per_byte, args, stream):
    shp = tgx.compile_shapes(SHAPES[name])
    rows = torch.empty(corpus.num_samples, dtype=torch.int64, device="cuda")
    byts = torch.empty(corpus.num_bytes, dtype=torch.uint8, device="cuda") if per_byte else None
    call = corpus.shape_cover if cover else corpus.shape_hits
    t_call, t_stage = staged(lambda: call(shp, rows.data_ptr(), byts.data_ptr() if per_byte else 0, stream=stream), args, _lib.shapes_last_times, STAGES)
    positions = int(shp.len.sum())
    rec = {"what": label, "call": "shape_cover" if cover else "shape_hits", "shapes": name, "positions": positions, "nw": 1 if positions <= 64 else 2, "per_byte": per_byte}
    put(rec, "call", t_call)
    for k in STAGES[:2 if cover else 1]:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(corpus.num_bytes, t_call["ms"])
    rec["marked"] = int(rows.sum().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("shapes_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for name in SHAPES:
            for cover, per_byte in ((False, False), (False, True), (True, False), (True, True)):
                rec["runs"].append(shape_run(corpus, "many_rows", name, cover, per_byte, args, stream))
        # the yardsticks and the floor, on the same object
        rec["pattern_hits_email"] = dfa_run(corpus, "pattern_hits", "email", False, args, stream)
        t_table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
        ts_stages = ("textstat_summary_kernel", "textstat_scan", "textstat_kernel")
        t_call, _ = staged(lambda: corpus.text_stats(t_table.data_ptr(), 0, 1000, "char", stream=stream), args, _lib.textstat_last_times, ts_stages)
        put(rec, "text_stats_call", t_call)
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        corpus.free()
        # one row without a newline: nothing about the time may depend on the text or the rows
        c = tgx.NativeCorpus(np.where(flat == 10, np.uint8(32), flat), np.asarray([0, flat.size], np.uint64))
        for name in SHAPES:
            for cover in (False, True):
                r = shape_run(c, "one_row_no_newline", name, cover, False, args, stream)
                many = next(x for x in rec["runs"] if x["what"] == "many_rows" and x["shapes"] == name and x["call"] == r["call"] and not x["per_byte"])
                r["call_x_many_rows"] = round(r["call_ms"] / many["call_ms"], 3)
                rec["runs"].append(r)
        c.free()
        for r in rec["runs"]:
            r["call_x_pattern_hits_email"] = round(r["call_ms"] / rec["pattern_hits_email"]["call_ms"], 2)
            r["call_x_text_stats"] = round(r["call_ms"] / rec["text_stats_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        nw1 = next(x for x in rec["runs"] if x["what"] == "many_rows" and x["nw"] == 1 and x["call"] == "shape_hits" and not x["per_byte"])
        nw2 = next(x for x in rec["runs"] if x["what"] == "many_rows" and x["nw"] == 2 and x["call"] == "shape_hits" and not x["per_byte"])
        rec["hits_nw2_x_nw1"] = round(nw2["call_ms"] / nw1["call_ms"], 3)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
