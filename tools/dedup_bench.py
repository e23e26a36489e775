"""Exact row deduplication on the device (csrc/dedup.hip) on bench.py's mixed corpus resident in HBM, and on the same
corpus with a share of its rows duplicated through NativeCorpus.select (0 %, 10 %, 50 % more rows, each a copy of a random
row, the whole in a seeded order): time of NativeCorpus.first_equal — the whole call, and the stages summed over the
call's rounds (tgx_dedup_last_times) — and of NativeCorpus.row_hashes, which is the hash stage alone, beside a thing
measured in the same run and process:

  hipMemcpyAsync device-to-device of the text's N bytes: the hash kernel reads N bytes and writes 8 S, the copy reads N and
  writes N, so a hash that takes longer than the copy is leaving bandwidth unused.

With --result the same for the rows of the corpus's encode (NativeResult.first_equal: u32 ids, the spec 32 000 vocabulary).
Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup, with the smallest and the largest beside it.  One JSON line per corpus.
usage: dedup_bench.py [--sizes 256,1024] [--shares 0,10,50] [--steps 10] [--warmup 3] [--result]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

from layout_bench import _hip, rate
from select_bench import d2d, spread, timed

STAGES = ("dedup_hash_kernel", "dedup_sort", "dedup_compare_kernel", "dedup_resolve")


def dedup_run(obj, what, n_bytes, steps, warmup, stream):
    """first_equal and row_hashes of obj timed -> the record's part; n_bytes: the bytes of obj's rows"""
    S = obj.num_samples
    d_first = torch.empty(S, dtype=torch.int64, device="cuda")
    d_hash = torch.empty(S, dtype=torch.int64, device="cuda")
    stages = {k: [] for k in STAGES}
    seen = {}

    def call():
        seen["n_unique"] = obj.first_equal(d_first.data_ptr(), stream=stream)
        seen["rounds"] = _lib.dedup_last_rounds()
        for k, v in _lib.dedup_last_times().items():
            stages[k].append(v)
    whole = timed(call, steps, warmup)
    hashes = timed(lambda: obj.row_hashes(d_hash.data_ptr(), 0, stream=stream), steps, warmup)
    out = {"what": what, "rows": S, "bytes": n_bytes, "n_unique": seen["n_unique"], "rounds": seen["rounds"], "call_ms": whole["ms"],
           "call_ms_min": whole["ms_min"], "call_ms_max": whole["ms_max"], "row_hashes_call_ms": hashes["ms"],
           "row_hashes_call_ms_min": hashes["ms_min"], "row_hashes_call_ms_max": hashes["ms_max"]}
    for k in STAGES:
        s = spread(stages[k][-steps:])
        out[k + "_ms"], out[k + "_ms_min"], out[k + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]
    out["hash_stage_gb_s"] = rate(n_bytes + 24 * S, out["dedup_hash_kernel_ms"])   # the rows' bytes; per row the offsets' scan and the sums
    out["duplicate_rows"] = int((d_first != torch.arange(S, device="cuda")).sum().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024", help="corpus sizes in MiB")
    ap.add_argument("--shares", default="0,10,50", help="rows added as copies, in percent of the corpus's rows")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--result", action="store_true", help="also the rows of the corpus's encode")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("dedup_bench.py needs a GPU")
    hip = _hip()
    model = None
    if args.result:
        toks, scores, _ = synth.load_spec_vocab(32000)
        model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        base = tgx.NativeCorpus(flat, offs)
        S0 = base.num_samples
        for share in [int(x) for x in args.shares.split(",")]:
            rng = np.random.default_rng(100 + share)
            extra = S0 * share // 100
            rows = np.concatenate([np.arange(S0), rng.integers(0, S0, extra)])[rng.permutation(S0 + extra)].astype(np.int64)
            corpus = base.select(torch.from_numpy(rows).cuda()) if share else base
            N, S = corpus.num_bytes, corpus.num_samples
            rec = {"corpus_mib": mib, "share_percent": share, "bytes": N, "samples": S, "mean_row_bytes": round(N / S, 1), "steps": args.steps, "runs": []}
            rec["runs"].append(dedup_run(corpus, "corpus_first_equal", N, args.steps, args.warmup, stream))
            copy = d2d(hip, N, args.steps, args.warmup)
            rec["runs"].append({"what": "d2d text", "bytes": N, **copy, "gb_s": rate(2 * N, copy["ms"])})
            run = rec["runs"][0]
            run["hash_stage_x_d2d"] = round(run["dedup_hash_kernel_ms"] / copy["ms"], 2)
            run["call_x_d2d"] = round(run["call_ms"] / copy["ms"], 2)
            if model is not None:
                res = model.encode_corpus(corpus)
                T = res.num_tokens
                rec["tokens"] = T
                rec["runs"].append(dedup_run(res, "result_first_equal", 4 * T, args.steps, args.warmup, stream))
                copy_ids = d2d(hip, 4 * T, args.steps, args.warmup)
                rec["runs"].append({"what": "d2d ids", "bytes": 4 * T, **copy_ids, "gb_s": rate(8 * T, copy_ids["ms"])})
                run = rec["runs"][2]
                run["hash_stage_x_d2d"] = round(run["dedup_hash_kernel_ms"] / copy_ids["ms"], 2)
                run["call_x_d2d"] = round(run["call_ms"] / copy_ids["ms"], 2)
                res.free()
            print(json.dumps(rec), flush=True)
            if corpus is not base:
                corpus.free()
            torch.cuda.empty_cache()
        base.free()


if __name__ == "__main__":
    main()
