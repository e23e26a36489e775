"""Cover and redaction on the device (csrc/cover.hip, csrc/redact.hip) on bench.py's mixed corpus resident in HBM: the
cover pass with the e-mail pattern (7 / 10 states: 32-bit forward maps, 64-bit backward ones) and the IPv4 pattern
(14 / 13: 64-bit maps on both sides), counts and mask, and the redact pass over the OR of the two masks, each with the
stages of tgx_redact_last_times.  Beside them, in the same process and on the same object, the yardstick: pattern_hits
(csrc/dfa.hip) with the same pattern, counts and ends.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end),
the median of --steps calls after --warmup with the smallest and the largest beside it.  One JSON line per size.
usage: redact_bench.py [--sizes 256] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from layout_bench import rate
from patterns_bench import PATTERNS, dfa_run
from textstat_bench import put
from wordstat_bench import staged

COVER_STAGES = ("cover_summary_kernel", "cover_scan", "cover_kernel")
REDACT_STAGES = ("redact_length_kernel", "redact_scan", "redact_offsets_kernel", "redact_fill_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("redact_bench.py needs a GPU")
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        S, N = corpus.num_samples, corpus.num_bytes
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "steps": args.steps, "runs": []}
        covered = torch.empty(S, dtype=torch.int64, device="cuda")
        masks = []
        for k, name in enumerate(PATTERNS):
            pat = tgx.compile_pattern(PATTERNS[name], cover=True)
            mask = torch.empty(N, dtype=torch.uint8, device="cuda")
            t_call, t_stage = staged(lambda: corpus.dfa_cover(pat, covered.data_ptr(), mask.data_ptr(), stream=stream), args, _lib.redact_last_times, COVER_STAGES)
            r = {"what": "pattern_cover", "pattern": name, "fwd_states": pat.n_states, "bwd_states": pat.back.n_states}
            put(r, "call", t_call)
            for s in COVER_STAGES:
                put(r, s, t_stage[s])
            r["call_gb_s"] = rate(N, t_call["ms"])
            r["covered_bytes"] = int(covered.sum().item())
            hits = dfa_run(corpus, "pattern_hits", name, True, args, stream)  # the yardstick, in the same run
            r["call_x_pattern_hits"] = round(r["call_ms"] / hits["call_ms"], 2)
            rec["runs"] += [r, hits]
            masks.append(mask << k if k else mask)
        both = masks[0] | masks[1]
        made = []

        def call():
            for c in made:
                c.free()
            made[:] = [corpus.redact(both.data_ptr(), ["<EMAIL>", "<IP_ADDRESS>"], stream=stream)]

        t_call, t_stage = staged(call, args, _lib.redact_last_times, REDACT_STAGES)
        r = {"what": "redact", "masked_bytes": int((both != 0).sum().item()), "bytes_out": made[0].num_bytes}
        put(r, "call", t_call)
        for s in REDACT_STAGES:
            put(r, s, t_stage[s])
        r["call_gb_s"] = rate(N, t_call["ms"])
        rec["runs"].append(r)
        made[0].free()
        corpus.free()
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
