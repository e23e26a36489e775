"""The device front end (csrc/front.hip: special-token split and CRLF for a resident corpus) on bench.py's mixed corpus with
the spec 32 000 vocabulary and special tokens written into the text under the two plans of tools/assemble_bench.py (fim,
chat).  Per plan, in one run:

  (a) the stages of NativeCorpus.split_specials (the library's events around each stage's kernels and scans: mark,
      resolve, segments, keep, pack) and the whole call;
  (b) the yardstick: a device-to-device hipMemcpyAsync of the same text (the stage reads the text twice and writes it once);
  (c) the host route's wall time: split_specials_flat + pack_segments (host threads) + the upload of the packed segments;
  (d) end to end on the host clock: Tokenizer.encode_corpus_result (corpus resident) against encode_batch_result_flat.

(a) and (b) are device events on torch's current stream around calls that return once their stream has reached its end,
the median of --steps calls after --warmup, as tools/layout_bench.py; (c) and (d) are the median of --e2e-steps calls after
one.  One JSON line per plan.   usage: front_bench.py [--size 256] [--steps 10] [--warmup 3] [--e2e-steps 3] [--no-e2e]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth
from assemble_bench import SPECIALS, host_clock, with_specials
from layout_bench import _hip, d2d, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="corpus size in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-steps", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true", help="skip (d)")
    ap.add_argument("--plans", default="fim,chat")
    ap.add_argument("--crlf", type=int, default=1)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("front_bench.py needs a GPU")
    hip = _hip()
    toks, scores, _ = synth.load_spec_vocab(32000)
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [tgx.CrlfProcessor()] if args.crlf else [], SPECIALS)
    specials = [s.encode() for s in SPECIALS]
    crlf = bool(args.crlf)
    flat0, offs0 = synth.make_corpus(args.size << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
    for plan_name in args.plans.split(","):
        flat, offs = with_specials(flat0, offs0, plan_name)
        flat = np.ascontiguousarray(flat)
        corpus = tgx.NativeCorpus(flat, offs)
        stages = []

        def split():
            segs, plan = corpus.split_specials(specials, crlf)
            stages.append(_lib.front_last_times())
            return segs, plan

        def split_and_free():
            segs, plan = split()
            segs.free()
            plan.free()
        call = timed(split_and_free, args.steps, args.warmup)
        last = stages[-args.steps:]
        stage_ms = {k: round(statistics.median(s[k] for s in last), 4) for k in last[0]}
        # the device route against the host route, once
        segs, plan = split()
        seg_offs, sb, se, ss = _lib.split_specials_flat(flat, offs, specials)
        pflat, poffs = _lib.pack_segments(flat, sb, se, ss, crlf)
        assert np.array_equal(plan.seg_offs(), seg_offs) and np.array_equal(plan.seg_special(), ss)
        assert np.array_equal(segs.offsets(), poffs) and np.array_equal(segs.bytes(), pflat)
        K, E, S = int(ss.size), int(poffs.size - 1), int(offs.size - 1)
        out_bytes = int(pflat.size)
        segs.free()
        plan.free()
        del sb, se, pflat, poffs
        copy = d2d(hip, int(flat.size), args.steps, args.warmup)

        def host_front():
            so, b, e, s = _lib.split_specials_flat(flat, offs, specials)
            pf, po = _lib.pack_segments(flat, b, e, s, crlf)
            tgx.NativeCorpus(pf, po).free()   # the upload (synchronous)
        host_ms = host_clock(host_front, args.e2e_steps)
        kernels = sum(stage_ms.values())
        rec = {"plan": plan_name, "corpus_mib": args.size, "bytes": int(flat.size), "samples": S, "segments": K, "encoded_segments": E,
               "specials": K - E, "crlf": crlf, "packed_bytes": out_bytes, "steps": args.steps,
               "stage_ms": stage_ms, "stages_ms": round(kernels, 4), "split_call_ms": call["ms"], "split_call_ms_min": call["ms_min"],
               "stages_gb_s": round(flat.size / kernels / 1e6, 1), "split_call_gb_s": round(flat.size / call["ms"] / 1e6, 1),
               "d2d_copy_ms": copy["ms"], "d2d_copy_ms_min": copy["ms_min"], "stages_over_copy": round(kernels / copy["ms"], 2),
               "call_over_copy": round(call["ms"] / copy["ms"], 2),
               "host_front_ms": host_ms, "host_front_gb_s": round(flat.size / host_ms / 1e6, 2), "host_over_call": round(host_ms / call["ms"], 2)}
        if not args.no_e2e:
            a, b = tk.encode_corpus_result(corpus), tk.encode_batch_result_flat(flat, offs)
            assert np.array_equal(a.offsets(), b.offsets()) and np.array_equal(a.ids(), b.ids())
            rec["ids_out"] = int(a.num_tokens)
            a.free()
            b.free()
            dev = host_clock(lambda: tk.encode_corpus_result(corpus).free(), args.e2e_steps)
            host = host_clock(lambda: tk.encode_batch_result_flat(flat, offs).free(), args.e2e_steps)
            rec.update({"e2e_encode_corpus_result_ms": dev, "e2e_encode_batch_result_flat_ms": host, "e2e_flat_over_corpus": round(host / dev, 2)})
        print(json.dumps(rec), flush=True)
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
