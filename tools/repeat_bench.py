"""Repeated n-grams within a row on the device (csrc/repeat.hip) on bench.py's mixed corpus resident in HBM and on its
encode under the spec 32 000 vocabulary: repeat_stats (table and mask) of the encode under w = 3 and w = 10 ids and of the
text under w = 50 bytes, as whole calls and per stage (tgx_repeat_last_times), the nine calls of repetition_rows with
Gopher's defaults on the encode, and a source that is one long row of one byte: a single run of its whole length, whose
chunks all add to the same row's sums.  Beside them, in the same process and on the same object, gram_hits against the
gram set of a held-out 1 MiB of the same generator (its gram_hits_kernel stage is the cover kernel's yardstick: the same
walk with a hash and a lookup in place of two flag loads).

Times are device events on torch's current stream around the call (which returns once the stream has reached its end) and
the stages of tgx_repeat_last_times, the median of --steps calls after --warmup with the smallest and the largest beside
it.  One JSON line per corpus size.
usage: repeat_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--one-row-mib 256]"""
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

from select_bench import spread, timed

STAGES = ("repeat_keys_kernel", "repeat_sort", "repeat_runs_kernel", "repeat_cover_kernel")
CLOCK_GHZ, SIMDS = 2.4, 256 * 4   # MI355X: the peak engine clock and the SIMDs, for the cycles-per-element figures


def put(out, name, s):
    out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]


def simd_cycles(ms, n_elems):
    return round(ms * 1e-3 * CLOCK_GHZ * 1e9 * SIMDS / max(n_elems, 1), 2)


def repeat_run(obj, what, width, elem_bytes, args, stream, steps=None):
    """repeat_stats of obj timed, the table and the mask -> the record"""
    steps = steps or args.steps
    S = obj.num_samples
    n_elems = obj.num_tokens if elem_bytes == 4 else obj.num_bytes
    table = torch.empty((_lib.REPEAT_N, S), dtype=torch.int64, device="cuda")
    mask = torch.empty(n_elems, dtype=torch.uint8, device="cuda")
    seen = {k: [] for k in STAGES}

    def call():
        obj.repeat_stats(width, 0, table.data_ptr(), mask.data_ptr(), stream=stream)
        t = _lib.repeat_last_times()
        for k in STAGES:
            seen[k].append(t[k])
    out = {"what": what, "rows": S, "elems": n_elems, "width": width, "steps": steps}
    put(out, "call", timed(call, steps, args.warmup))
    for k in STAGES:
        put(out, k, spread(seen[k][-steps:]))
    stages = sum(out[k + "_ms"] for k in STAGES)
    out["grams"] = int(table[0].sum().item())
    out["repeated"] = int(table[1].sum().item())
    out["covered"] = int(table[4].sum().item())
    out["sort_share_of_stages"] = round(out["repeat_sort_ms"] / stages, 3)
    out["cover_simd_cycles_per_elem"] = simd_cycles(out["repeat_cover_kernel_ms"], n_elems)
    out["gelems_s"] = round(n_elems / out["call_ms"] / 1e6, 3)
    return out


def hits_run(obj, held_out, what, width, elem_bytes, args, stream):
    """gram_hits of obj against the held-out set timed, counts and mask -> the record"""
    S = obj.num_samples
    n_elems = obj.num_tokens if elem_bytes == 4 else obj.num_bytes
    count = torch.empty(S, dtype=torch.int64, device="cuda")
    mask = torch.empty(n_elems, dtype=torch.uint8, device="cuda")
    gs = held_out.gram_set(width, 0, stream=stream)
    seen = []

    def call():
        obj.gram_hits(gs, count.data_ptr(), mask.data_ptr(), stream=stream)
        seen.append(_lib.gram_last_times()["gram_hits_kernel"])
    out = {"what": what, "width": width, "elems": n_elems, "n_keys": gs.size}
    put(out, "call", timed(call, args.steps, args.warmup))
    put(out, "gram_hits_kernel", spread(seen[-args.steps:]))
    out["hits_simd_cycles_per_elem"] = simd_cycles(out["gram_hits_kernel_ms"], n_elems)
    gs.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--held-out-mib", type=int, default=1)
    ap.add_argument("--one-row-mib", type=int, default=256, help="the one long row of one byte (0: skip)")
    ap.add_argument("--widths-ids", default="3,10")
    ap.add_argument("--width-bytes", type=int, default=50)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("repeat_bench.py needs a GPU")
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    stream = torch.cuda.current_stream().cuda_stream
    h_flat, h_offs = synth.make_corpus(args.held_out_mib << 20, "mixed", seed_offset=2000)   # held out: another seed of the same generator
    held_corpus = tgx.NativeCorpus(h_flat, h_offs)
    held_res = model.encode_corpus(held_corpus)
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        rec = {"corpus_mib": mib, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "tokens": res.num_tokens, "steps": args.steps, "runs": [],
               "yardsticks": []}
        for w in [int(x) for x in args.widths_ids.split(",") if x]:
            rec["runs"].append(repeat_run(res, "result_repeat_stats", w, 4, args, stream))
        rec["runs"].append(repeat_run(corpus, "corpus_repeat_stats", args.width_bytes, 1, args, stream))
        rec["yardsticks"].append(hits_run(res, held_res, "result_gram_hits", 10, 4, args, stream))
        rec["yardsticks"].append(hits_run(corpus, held_corpus, "corpus_gram_hits", args.width_bytes, 1, args, stream))
        kept = []
        put(rec, "repetition_rows_call", timed(lambda: kept.append(tgx.repetition_rows(res).shape[0]), args.steps, args.warmup))
        rec["repetition_rows_kept"] = kept[-1]
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()
    if args.one_row_mib:
        n = args.one_row_mib << 20
        one = tgx.NativeCorpus(np.full(n, ord("a"), np.uint8), np.asarray([0, n], np.uint64))
        rec = {"one_row_mib": args.one_row_mib, "runs": [repeat_run(one, "one_row_of_one_byte", args.width_bytes, 1, args, stream, steps=3)]}
        print(json.dumps(rec), flush=True)
        one.free()


if __name__ == "__main__":
    main()
