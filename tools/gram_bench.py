"""Shared n-grams on the device (csrc/gram.hip) on bench.py's mixed corpus resident in HBM and on its encode under the spec
32 000 vocabulary: the probe (gram_hits: counts and mask) of the encode under w = 13 ids and of the text under w = 50 bytes
against (1) the gram set of a held-out 1 MiB of the same generator, with the time of building that set, and (2) sets of
2^10, 2^16, 2^20 and 2^24 random keys made through from_keys, whose directory and keys sit in L2, in the Infinity Cache
and beyond.  Beside them, in the same process and on the same object:

  (a) row_hashes, which reads the same bytes once;
  (b) minhash at K = 64 and the same width: the same hash per position, then 64 multiply-adds in place of one lookup.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end) and
the stages of tgx_gram_last_times, the median of --steps calls after --warmup with the smallest and the largest beside
it.  One JSON line per object.
usage: gram_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--held-out-mib 1] [--set-bits 10,16,20,24]"""
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
from select_bench import spread, timed

STAGES = ("gram_keys_kernel", "gram_sort", "gram_dir", "gram_hits_kernel")


def staged(call, names, args):
    """call() timed, with the named stages of tgx_gram_last_times of the timed calls -> (call's spread, {stage: spread})"""
    seen = {k: [] for k in names}

    def fn():
        call()
        t = _lib.gram_last_times()
        for k in names:
            seen[k].append(t[k])
    t_call = timed(fn, args.steps, args.warmup)
    return t_call, {k: spread(v[-args.steps:]) for k, v in seen.items()}


def put(out, name, s):
    out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]


def gram_run(obj, held_out, what, width, elem_bytes, args, stream):
    """the probes of obj timed -> the record"""
    S = obj.num_samples
    n_elems = obj.num_tokens if elem_bytes == 4 else obj.num_bytes
    count = torch.empty(S, dtype=torch.int64, device="cuda")
    mask = torch.empty(n_elems, dtype=torch.uint8, device="cuda")
    d_hash = torch.empty(S, dtype=torch.int64, device="cuda")
    sig = torch.empty((S, 64), dtype=torch.int32, device="cuda")
    out = {"what": what, "rows": S, "elems": n_elems, "bytes": n_elems * elem_bytes, "width": width, "probes": []}
    made = {}

    def create():
        if "gs" in made:
            made["gs"].free()
        made["gs"] = held_out.gram_set(width, 0, stream=stream)
    t_call, t_stage = staged(create, STAGES[:3], args)
    put(out, "set_create_call", t_call)
    for k, s in t_stage.items():
        put(out, k, s)
    sets = [("held_out", made["gs"])]
    rng = np.random.default_rng(1)
    for bits in args.set_bits:
        sets.append((f"random_2^{bits}", _lib.NativeGramSet.from_keys(rng.integers(0, 1 << 64, 1 << bits, dtype=np.uint64), width, "ids" if elem_bytes == 4 else "bytes")))
    for name, gs in sets:
        rec = {"set": name, "n_keys": gs.size, "dir_bits": gs.dir_bits, "set_bytes": gs.size * 8 + ((1 << gs.dir_bits) + 1) * 4}
        for label, c_ptr, m_ptr in (("count_and_mask", count.data_ptr(), mask.data_ptr()), ("count_only", count.data_ptr(), 0)):
            t_call, t_stage = staged(lambda: obj.gram_hits(gs, c_ptr, m_ptr, stream=stream), STAGES[3:], args)
            put(rec, label + "_call", t_call)
            put(rec, label + "_kernel", t_stage["gram_hits_kernel"])
            rec[label + "_gb_s"] = rate(n_elems * elem_bytes, t_stage["gram_hits_kernel"]["ms"])
            rec[label + "_gelems_s"] = round(n_elems / t_stage["gram_hits_kernel"]["ms"] / 1e6, 2)
        rec["rows_hit"] = int((count > 0).sum().item())
        out["probes"].append(rec)
        gs.free()
    # the yardsticks, on the same object
    put(out, "row_hashes_call", timed(lambda: obj.row_hashes(d_hash.data_ptr(), 0, stream=stream), args.steps, args.warmup))
    sig_ms = []

    def call_sig():
        obj.minhash(sig.data_ptr(), width, 64, 0, stream=stream)
        sig_ms.append(_lib.minhash_last_times()["minhash_sig_kernel"])
    put(out, "minhash_k64_call", timed(call_sig, args.steps, args.warmup))
    put(out, "minhash_k64_sig_kernel", spread(sig_ms[-args.steps:]))
    for rec in out["probes"]:
        rec["kernel_x_row_hashes"] = round(rec["count_and_mask_kernel_ms"] / out["row_hashes_call_ms"], 2)
        rec["kernel_x_minhash_k64"] = round(rec["count_and_mask_kernel_ms"] / out["minhash_k64_sig_kernel_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--held-out-mib", type=int, default=1)
    ap.add_argument("--set-bits", default="10,16,20,24", help="log2 of the sizes of the random key sets")
    ap.add_argument("--width-ids", type=int, default=13)
    ap.add_argument("--width-bytes", type=int, default=50)
    args = ap.parse_args()
    args.set_bits = [int(x) for x in args.set_bits.split(",") if x]
    if tgx.device_count() < 1:
        raise SystemExit("gram_bench.py needs a GPU")
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
        rec = {"corpus_mib": mib, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "tokens": res.num_tokens, "held_out_bytes": held_corpus.num_bytes,
               "held_out_tokens": held_res.num_tokens, "steps": args.steps, "runs": []}
        rec["runs"].append(gram_run(res, held_res, "result_gram_hits", args.width_ids, 4, args, stream))
        rec["runs"].append(gram_run(corpus, held_corpus, "corpus_gram_hits", args.width_bytes, 1, args, stream))
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
