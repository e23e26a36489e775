"""Leftmost-first matches and the mine on the device (csrc/find.hip) on two sources resident in HBM, because the walk's time
depends on the text: bench.py's mixed corpus, and an adversarial one, the same bytes with every letter turned into a
space, long runs of spaces under \\s+.  Per source and pattern: find_matches (counts, lens and truncated) and the mine
(top 1000), each with the stages of tgx_find_last_times; beside them, in the same process and on the same object, the
yardstick, pattern_hits with the max_states=64 automaton of the same pattern (the text-independent cost of one automaton
pass), and re.finditer on the host over the first --host-mib MiB for scale.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per source.
usage: find_bench.py [--size 256] [--steps 10] [--warmup 3] [--host-mib 16]"""
import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from layout_bench import rate
from textstat_bench import put
from wordstat_bench import staged

FIND_STAGES = ("find_walk_kernel", "find_scan", "find_replay_kernel")
MINE_STAGES = FIND_STAGES + ("find_keys", "find_sort_runs", "find_order")
STAGES64 = ("dfa64_map_kernel", "dfa64_scan", "dfa64_replay_kernel", "dfa64_count_kernel")
WORDS, SPACE = r" ?[A-Za-z_][A-Za-z0-9_]*|[0-9]{1,3}|\n[ ]+", r"\s+"


def run(corpus, flat, src, args, stream):
    S, N = corpus.num_samples, corpus.num_bytes
    pat = tgx.compile_pattern(src, find=True)
    count, truncated = (torch.empty(S, dtype=torch.int64, device="cuda") for _ in range(2))
    lens = torch.empty(N, dtype=torch.uint8, device="cuda")
    rec = {"pattern": src, "n_states": pat.n_states}
    t_find, t_stage = staged(lambda: corpus.find(pat, count.data_ptr(), lens.data_ptr(), truncated.data_ptr(), stream=stream), args, _lib.find_last_times, FIND_STAGES)
    put(rec, "find", t_find)
    for k in FIND_STAGES:
        put(rec, k, t_stage[k])
    rec["find_gb_s"], rec["matches"], rec["truncated"] = rate(N, t_find["ms"]), int(count.sum().item()), int(truncated.sum().item())
    mined = []
    t_mine, t_stage = staged(lambda: mined.append(corpus.mine(pat, 1000, stream=stream)), args, _lib.find_last_times, MINE_STAGES)
    put(rec, "mine", t_mine)
    for k in MINE_STAGES[3:]:
        put(rec, k, t_stage[k])
    rec["distinct"] = int(mined[-1][3])
    # the yardstick: one text-independent automaton pass with the search automaton of the same pattern
    hits = tgx.compile_pattern(src, max_states=64)
    call = corpus.dfa64_hits if hits.n_states > 16 else corpus.dfa_hits
    times = _lib.dfa64_last_times if hits.n_states > 16 else _lib.dfa_last_times
    t_hits, _ = staged(lambda: call(hits, count.data_ptr(), 0, stream=stream), args, times, ())
    put(rec, "pattern_hits", t_hits)
    rec["pattern_hits_states"], rec["find_x_pattern_hits"] = hits.n_states, round(t_find["ms"] / t_hits["ms"], 3)
    head = flat[:args.host_mib << 20].tobytes()
    t0 = time.perf_counter()
    n_host = sum(1 for _ in re.finditer(src.encode(), head))
    rec["host_re_finditer_s"], rec["host_re_mib"], rec["host_re_matches"] = round(time.perf_counter() - t0, 3), args.host_mib, n_host
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="corpus size in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-mib", type=int, default=16)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("find_bench.py needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    flat, offs = synth.make_corpus(args.size << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
    letters = ((flat | 0x20) >= ord("a")) & ((flat | 0x20) <= ord("z"))
    for source, text, patterns in (("mixed", flat, (WORDS, SPACE)), ("adversarial", np.where(letters, np.uint8(32), flat), (SPACE,))):
        corpus = tgx.NativeCorpus(text, offs)
        rec = {"source": source, "corpus_mib": args.size, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "steps": args.steps,
               "runs": [run(corpus, text, src, args, stream) for src in patterns]}
        corpus.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
