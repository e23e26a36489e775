"""Byte patterns of up to 64 states on the device (csrc/dfa64.hip) on bench.py's mixed corpus resident in HBM: the phone
shape of 17 states, the counts alone and with the per-byte ends; the e-mail, IPv4 and SSN patterns as ONE automaton
against the separate 16-state calls of pattern_hits that it replaces; and the same bytes as one row, which must take
the time of the many rows.  Beside them, in the same process and on the same object, the yardsticks: pattern_hits with
the IPv4 pattern (14 states, csrc/dfa.hip), the 7-state e-mail pattern through both paths, and text_stats.  Every dfa64
run carries the stages of tgx_dfa64_last_times.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: patterns64_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
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

from layout_bench import rate
from textstat_bench import put
from wordstat_bench import staged

STAGES16 = ("dfa_summary_kernel", "dfa_scan", "dfa_kernel")
STAGES64 = ("dfa64_map_kernel", "dfa64_scan", "dfa64_replay_kernel", "dfa64_count_kernel")
EMAIL, IPV4, SSN = r"[a-zA-Z0-9._%+-]+@[a-zA-Z0-9.-]+\.[a-zA-Z]{2,}", r"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}", r"\d{3}-\d{2}-\d{4}"
PHONE = r"\+\d{2} \d{3} \d{3} \d{4}"


def run(corpus, label, sources, wide, with_ends, args, stream):
    """one pattern or list through the 64-state call (wide) or the 16-state one"""
    pat = tgx.compile_pattern(sources, max_states=64 if wide else 16)
    count = torch.empty(corpus.num_samples, dtype=torch.int64, device="cuda")
    ends = torch.empty(corpus.num_bytes, dtype=torch.uint8, device="cuda") if with_ends else None
    call, times, stages = (corpus.dfa64_hits, _lib.dfa64_last_times, STAGES64) if wide else (corpus.dfa_hits, _lib.dfa_last_times, STAGES16)
    t_call, t_stage = staged(lambda: call(pat, count.data_ptr(), ends.data_ptr() if with_ends else 0, stream=stream), args, times, stages)
    rec = {"what": label, "n_states": pat.n_states, "path": "dfa64" if wide else "dfa", "ends": with_ends}
    put(rec, "call", t_call)
    for k in stages:
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
        raise SystemExit("patterns64_bench.py needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        runs = rec["runs"]
        runs.append(run(corpus, "phone", PHONE, True, False, args, stream))
        runs.append(run(corpus, "phone", PHONE, True, True, args, stream))
        runs.append(run(corpus, "email+ipv4+ssn", [EMAIL, IPV4, SSN], True, False, args, stream))
        # what the combined automaton replaces, and the yardsticks
        separate = [run(corpus, name, src, False, False, args, stream) for name, src in (("email", EMAIL), ("ipv4", IPV4), ("ssn", SSN))]
        runs += separate
        runs.append(run(corpus, "email", EMAIL, True, False, args, stream))
        rec["separate_calls_ms"] = round(sum(r["call_ms"] for r in separate), 3)
        rec["combined_x_separate"] = round(runs[2]["call_ms"] / rec["separate_calls_ms"], 3)
        t_table = torch.empty((_lib.TEXTSTAT_N, S), dtype=torch.int64, device="cuda")
        ts_stages = ("textstat_summary_kernel", "textstat_scan", "textstat_kernel")
        t_call, _ = staged(lambda: corpus.text_stats(t_table.data_ptr(), 0, 1000, "char", stream=stream), args, _lib.textstat_last_times, ts_stages)
        put(rec, "text_stats_call", t_call)
        corpus.free()
        # one row without a newline: nothing about the time may depend on the text or the rows
        c = tgx.NativeCorpus(np.where(flat == 10, np.uint8(32), flat), np.asarray([0, flat.size], np.uint64))
        r = run(c, "one_row email+ipv4+ssn", [EMAIL, IPV4, SSN], True, False, args, stream)
        r["call_x_many_rows"] = round(r["call_ms"] / runs[2]["call_ms"], 3)
        runs.append(r)
        c.free()
        for r in runs:
            r["call_x_text_stats"] = round(r["call_ms"] / rec["text_stats_call_ms"], 2)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
