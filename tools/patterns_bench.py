"""Byte patterns on the device (csrc/dfa.hip) on bench.py's mixed corpus resident in HBM: pattern_hits with the e-mail
pattern (7 states: the 32-bit maps, NS = 8) and the IPv4 pattern (14 states: the 64-bit maps, NS = 16), the counts alone
and with the per-byte ends, with the stages of tgx_dfa_last_times.  Beside them, in the same process and on the same
object, the yardstick: text_stats (csrc/textstat.hip, whose walk the kernels share), and a device-to-device copy.

Then the case the design is for: the same bytes as one row without a newline, which must take the time of the many rows.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: patterns_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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

STAGES = ("dfa_summary_kernel", "dfa_scan", "dfa_kernel")
PATTERNS = {"email": r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}", "ipv4": r"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}"}


def dfa_run(corpus, label, name, with_ends, args, stream):
    pat = tgx.compile_pattern(PATTERNS[name])
    count = torch.empty(corpus.num_samples, dtype=torch.int64, device="cuda")
    ends = torch.empty(corpus.num_bytes, dtype=torch.uint8, device="cuda") if with_ends else None
    t_call, t_stage = staged(lambda: corpus.dfa_hits(pat, count.data_ptr(), ends.data_ptr() if with_ends else 0, stream=stream), args, _lib.dfa_last_times,
                             STAGES)
    rec = {"what": label, "pattern": name, "n_states": pat.n_states, "map_bits": 32 if pat.n_states <= 8 else 64, "ends": with_ends}
    put(rec, "call", t_call)
    for k in STAGES:
        put(rec, k, t_stage[k])
    rec["call_gb_s"] = rate(corpus.num_bytes, t_call["ms"])
    rec["match_ends"] = int(count.sum().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("patterns_bench.py needs a GPU")
    hip = _hip()
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        for name in PATTERNS:
            for with_ends in (False, True):
                rec["runs"].append(dfa_run(corpus, "pattern_hits", name, with_ends, args, stream))
        # the yardstick and the floor, on the same object
        t_table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
        ts_stages = ("textstat_summary_kernel", "textstat_scan", "textstat_kernel")
        t_call, t_stage = staged(lambda: corpus.text_stats(t_table.data_ptr(), 0, 1000, "char", stream=stream), args, _lib.textstat_last_times, ts_stages)
        put(rec, "text_stats_call", t_call)
        for k in ts_stages:
            put(rec, k, t_stage[k])
        put(rec, "d2d_copy", d2d(hip, N, args.steps, args.warmup))
        corpus.free()
        # one row without a newline: nothing about the time may depend on the text or the rows
        c = tgx.NativeCorpus(np.where(flat == 10, np.uint8(32), flat), np.asarray([0, flat.size], np.uint64))
        for name in PATTERNS:
            r = dfa_run(c, "one_row_no_newline", name, False, args, stream)
            r["call_x_many_rows"] = round(r["call_ms"] / next(x for x in rec["runs"] if x["pattern"] == name and not x["ends"])["call_ms"], 3)
            rec["runs"].append(r)
        c.free()
        for r in rec["runs"]:
            r["call_x_text_stats"] = round(r["call_ms"] / rec["text_stats_call_ms"], 2)
            r["call_x_d2d_copy"] = round(r["call_ms"] / rec["d2d_copy_ms"], 2)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
