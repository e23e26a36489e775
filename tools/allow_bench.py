"""The document-frequency pass with the allow pattern on the device (tgx_substring_df_allow: csrc/allow.hip) beside the
parent path (tgx_substring_df_top and the allow regex on the host) on bench.py's mixed corpus, every sample one part, the
reference's allow regex as the 37-state automaton of tests/allow_cases.py.  Per max_token_length: the kept windows and the
distinct substrings with and without the filter; the wall time of either call (both synchronous, both with the same upload
of the text) with top_k = --top-k and, unless --no-all, with top_k = 0; the new call's device time per stage
(tgx_allow_last_times); and the host regex filter's wall time over the first --host-rows substrings the parent returns.

Wall times are the median of --steps calls after --warmup, smallest and largest beside it.  One JSON line per length.
usage: allow_bench.py [--size 64] [--mtl 16 24] [--steps 3] [--warmup 1] [--top-k 100000] [--host-rows 1000000] [--no-all]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth

import allow_cases as ac


def timed(call, args):
    out, ms = None, []
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        out = call()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="corpus size in MiB")
    ap.add_argument("--mtl", type=int, nargs="+", default=[16, 24])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--top-k", type=int, default=100000)
    ap.add_argument("--host-rows", type=int, default=1000000)
    ap.add_argument("--no-all", action="store_true", help="skip the top_k = 0 calls (every distinct substring comes back)")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("allow_bench.py needs a GPU")
    flat, offs = synth.make_corpus(args.size << 20, "mixed", seed_offset=1000)  # bench.py's corpus of rank 0
    keep = np.flatnonzero(offs[1:] > offs[:-1])
    pb, pe, ps = offs[:-1][keep], offs[1:][keep], keep.astype(np.uint32)
    pat, exact = ac.automaton("B"), re.compile(ac.exact_source())
    for mtl in args.mtl:
        rec = {"corpus_mib": args.size, "bytes": int(flat.size), "parts": int(pb.size), "max_token_length": mtl, "n_states": pat.n_states, "steps": args.steps}
        for label, top_k in [("top", args.top_k)] + ([] if args.no_all else [("all", 0)]):
            stages = []

            def new():
                out = _lib.substring_df_allow(flat, pb, pe, ps, mtl, top_k, pat)
                stages.append(_lib.allow_last_times())
                return out

            got, t_new = timed(new, args)
            parent, t_parent = timed(lambda: _lib.substring_df_top(flat, pb, pe, ps, mtl, top_k), args)
            rec[f"allow_{label}"], rec[f"parent_{label}"] = t_new, t_parent
            rec[f"parent_x_allow_{label}"] = round(t_parent["ms"] / t_new["ms"], 3)
            rec[f"allow_{label}_stages_ms"] = {k: round(statistics.median(s[k] for s in stages[args.warmup:]), 3) for k in stages[-1]}
            rec["n_windows_allow"], rec["n_distinct_allow"], rec["n_windows_parent"], rec["n_distinct_parent"] = got[3], got[4], parent[3], parent[4]
            rec[f"cutoff_df_{label}"] = {"allow": got[5], "parent": parent[5]}
            if label == "all":  # what the parent path then does on the host, over the first rows
                raw, rows = flat.tobytes(), min(args.host_rows, len(parent[0]))
                t0 = time.perf_counter()
                kept = sum(1 for p, l in zip(parent[0][:rows].tolist(), parent[1][:rows].tolist()) if exact.fullmatch(raw[p:p + l]))
                rec["host_filter"] = {"rows": rows, "kept": kept, "s": round(time.perf_counter() - t0, 3)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
