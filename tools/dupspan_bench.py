"""Duplicate spans across rows on the device (csrc/dupspan.hip) on bench.py's mixed corpus resident in HBM and on its encode
under the spec 32 000 vocabulary: dup_spans (table and mask) of the encode under w = 13 ids and of the text under w = 50
bytes, as whole calls and per stage (tgx_dupspan_last_times), for key_bits = 64, 48, 40 and 32 (sort time against match
time), and beside each source, in the same process and on the same object, repeat_stats at the same width
(tgx_repeat_last_times): the same keys, sort and cover work, with repeat_runs_kernel where dupspan_match_kernel stands.

Times are device events on torch's current stream around the call and the stages' own times, the median of --steps
calls after --warmup with the smallest and the largest beside it.  One JSON line per corpus size.
usage: dupspan_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--key-bits 64,48,40,32]"""
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

from repeat_bench import put, repeat_run
from select_bench import spread, timed

STAGES = ("dupspan_keys_kernel", "dupspan_sort", "dupspan_match_kernel", "dupspan_cover_kernel")


def dupspan_run(obj, what, width, key_bits, elem_bytes, args, stream):
    """dup_spans of obj timed, the table and the mask -> the record"""
    S = obj.num_samples
    n_elems = obj.num_tokens if elem_bytes == 4 else obj.num_bytes
    table = torch.empty((_lib.DUPSPAN_N, S), dtype=torch.int64, device="cuda")
    mask = torch.empty(n_elems, dtype=torch.uint8, device="cuda")
    seen = {k: [] for k in STAGES}

    def call():
        obj.dup_spans(width, key_bits, 0, table.data_ptr(), mask.data_ptr(), stream=stream)
        t = _lib.dupspan_last_times()
        for k in STAGES:
            seen[k].append(t[k])
    out = {"what": what, "rows": S, "elems": n_elems, "width": width, "key_bits": key_bits, "steps": args.steps}
    put(out, "call", timed(call, args.steps, args.warmup))
    for k in STAGES:
        put(out, k, spread(seen[k][-args.steps:]))
    out["grams"], out["dup"], out["covered"] = (int(table[k].sum().item()) for k in range(3))
    out["sort_share_of_stages"] = round(out["dupspan_sort_ms"] / sum(out[k + "_ms"] for k in STAGES), 3)
    out["gelems_s"] = round(n_elems / out["call_ms"] / 1e6, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width-ids", type=int, default=13)
    ap.add_argument("--width-bytes", type=int, default=50)
    ap.add_argument("--key-bits", default="64,48,40,32")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("dupspan_bench.py needs a GPU")
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        rec = {"corpus_mib": mib, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "tokens": res.num_tokens, "steps": args.steps, "runs": [],
               "yardsticks": []}
        for obj, what, w, eb in ((res, "result", args.width_ids, 4), (corpus, "corpus", args.width_bytes, 1)):
            rec["yardsticks"].append(repeat_run(obj, what + "_repeat_stats", w, eb, args, stream))
            for kb in [int(x) for x in args.key_bits.split(",")]:
                rec["runs"].append(dupspan_run(obj, what + "_dup_spans", w, kb, eb, args, stream))
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
