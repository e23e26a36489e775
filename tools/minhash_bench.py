"""Near-duplicate rows on the device (csrc/minhash.hip) on bench.py's mixed corpus resident in HBM and on its encode under
the spec 32 000 vocabulary: time of the signatures (NativeCorpus.minhash over shingles of 32 bytes, NativeResult.minhash
over 5-grams of ids; K = 128), of the band keys and heads (B = 32) and of the clustering (threshold 0.7), the whole calls
and the stages (tgx_minhash_last_times), beside two yardsticks measured or derived in the same process:

  (a) row_hashes of the same object, which reads the same bytes once;
  (b) an arithmetic floor of the signature kernel: its S·m·K (shingle, permutation) steps, --valu-per-step vector
      instructions each (counted in the disassembly of the build that ran: profiles/minhash/kernel_resources.txt), a
      wave-instruction every --cycles-per-valu cycles on each of --simds SIMDs at --clock-ghz.  measured / floor is reported.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup, with the smallest and the largest beside it.  One JSON line per object.
usage: minhash_bench.py [--sizes 256] [--steps 10] [--warmup 3] [--perm 128] [--bands 32]"""
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

STAGES = ("minhash_sig_kernel", "minhash_band_keys", "minhash_sort", "minhash_heads", "minhash_verify", "minhash_roots")


def minhash_run(obj, what, width, elem_bytes, offs, args, stream):
    """signatures, bands and clusters of obj timed -> the record; offs: the rows' offsets on the host (for the step count)"""
    S, K, B = obj.num_samples, args.perm, args.bands
    n = np.diff(offs.astype(np.int64))
    positions = int(np.maximum(n - width + 1, 1).sum())
    n_bytes = int(n.sum()) * elem_bytes
    sig = torch.empty((S, K), dtype=torch.int32, device="cuda")
    heads = torch.empty((S, B), dtype=torch.int64, device="cuda")
    first = torch.empty(S, dtype=torch.int64, device="cuda")
    d_hash = torch.empty(S, dtype=torch.int64, device="cuda")
    stages = {k: [] for k in STAGES}
    seen = {}
    min_agree = int(np.ceil(args.threshold * K))

    def keep(names):
        t = _lib.minhash_last_times()
        for k in names:
            stages[k].append(t[k])

    def call_sig():
        obj.minhash(sig.data_ptr(), width, K, 0, stream=stream)
        keep(STAGES[:1])

    def call_bands():
        _lib.minhash_bands(0, sig.data_ptr(), S, K, B, 0, 0, heads.data_ptr(), stream=stream)
        keep(STAGES[1:4])

    def call_near():
        seen["n_clusters"] = _lib.minhash_near_first(0, sig.data_ptr(), S, K, heads.data_ptr(), B, min_agree, first.data_ptr(), stream=stream)
        keep(STAGES[4:])
    t_sig = timed(call_sig, args.steps, args.warmup)
    t_bands = timed(call_bands, args.steps, args.warmup)
    t_near = timed(call_near, args.steps, args.warmup)
    t_hash = timed(lambda: obj.row_hashes(d_hash.data_ptr(), 0, stream=stream), args.steps, args.warmup)
    out = {"what": what, "rows": S, "bytes": n_bytes, "width": width, "n_perm": K, "bands": B, "min_agree": min_agree, "positions": positions,
           "steps": positions * K, "n_clusters": seen["n_clusters"]}
    for name, t in (("minhash_call", t_sig), ("bands_call", t_bands), ("near_first_call", t_near), ("row_hashes_call", t_hash)):
        out[name + "_ms"], out[name + "_ms_min"], out[name + "_ms_max"] = t["ms"], t["ms_min"], t["ms_max"]
    for k in STAGES:
        s = spread(stages[k][-args.steps:])
        out[k + "_ms"], out[k + "_ms_min"], out[k + "_ms_max"] = s["ms"], s["ms_min"], s["ms_max"]
    sig_ms = out["minhash_sig_kernel_ms"]
    out["sig_stage_gb_s"] = rate(n_bytes, sig_ms)
    out["sig_stage_gsteps_s"] = round(positions * K / sig_ms / 1e6, 1)
    out["sig_stage_x_row_hashes"] = round(sig_ms / out["row_hashes_call_ms"], 2)                       # yardstick (a)
    floor_ms = positions * K / 64 * args.valu_per_step * args.cycles_per_valu / args.simds / (args.clock_ghz * 1e6)
    out["floor"] = {"valu_per_step": args.valu_per_step, "cycles_per_valu": args.cycles_per_valu, "simds": args.simds, "clock_ghz": args.clock_ghz,
                    "ms": round(floor_ms, 4)}
    out["sig_stage_x_floor"] = round(sig_ms / floor_ms, 2)                                             # yardstick (b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--perm", type=int, default=128)
    ap.add_argument("--bands", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--width-ids", type=int, default=5)
    ap.add_argument("--width-bytes", type=int, default=32)
    ap.add_argument("--valu-per-step", type=float, default=6.0,
                    help="vector instructions of one (shingle, permutation) step: 5 of its own and the 2 broadcasts shared by ceil(K / 64); K = 128: 6")
    ap.add_argument("--cycles-per-valu", type=float, default=2.0, help="cycles of a SIMD per wave-instruction at full rate")
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("minhash_bench.py needs a GPU")
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        rec = {"corpus_mib": mib, "bytes": corpus.num_bytes, "samples": corpus.num_samples, "tokens": res.num_tokens, "steps": args.steps, "runs": []}
        rec["runs"].append(minhash_run(res, "result_minhash", args.width_ids, 4, res.offsets(), args, stream))
        rec["runs"].append(minhash_run(corpus, "corpus_minhash", args.width_bytes, 1, np.asarray(offs), args, stream))
        print(json.dumps(rec), flush=True)
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
