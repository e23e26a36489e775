"""Row selection on the device (csrc/select.hip) on a resident encode of bench.py's mixed corpus with the spec 32 000
vocabulary: time of NativeResult.select and NativeCorpus.select with identity rows and with the seeded permutation
(shuffled_rows), through the host-index and the device-index path — the whole call, and the stages alone
(tgx_select_last_times) — and of tgx_shuffled_rows_device alone, beside two things measured in the same run and process:

  (a) NativeResult.fim at rate 0 over the same result: the project's existing copy through the same per-tile search
      (fim_fill_kernel, tgx_fim_last_times);
  (b) hipMemcpyAsync device-to-device of the output's bytes: the floor of a kernel that reads and writes that much.

Times are device events on torch's current stream around the call (which returns once the stream has reached its end), the
median of --steps calls after --warmup, with the smallest and the largest beside it.  One JSON line per corpus size.
usage: select_bench.py [--sizes 256,1024] [--steps 10] [--warmup 3]"""
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


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def timed(fn, steps, warmup):
    """median / min / max ms of fn() between two events on the current stream"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms)


def d2d(hip, nbytes, steps, warmup):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream)  # hipMemcpyDeviceToDevice
        assert rc == 0, rc
        torch.cuda.current_stream().synchronize()   # as the select calls do
    return timed(fn, steps, warmup)


def select_run(obj, rows, what, order, path, unit, n_rows, steps, warmup, stream):
    """one timed select -> its record; unit: bytes per element (4: ids, 1: text)"""
    stages = {"select_check": [], "select_offsets_scan": [], "select_fill_kernel": []}
    n_out = [0]

    def call():
        out = obj.select(rows, stream=stream)
        for k, v in _lib.select_last_times().items():
            stages[k].append(v)
        n_out[0] = out.num_tokens if unit == 4 else out.num_bytes
        out.free()
    whole = timed(call, steps, warmup)
    fill = spread(stages["select_fill_kernel"][-steps:])
    moved = 2 * unit * n_out[0] + 8 * n_rows + 16 * (n_rows + 1)   # elements read and written, the index, both offsets per row
    return {"what": what, "rows": order, "index_path": path, "out_elements": n_out[0], "call_ms": whole["ms"], "call_ms_min": whole["ms_min"],
            "call_ms_max": whole["ms_max"], "fill_kernel_ms": fill["ms"], "fill_kernel_ms_min": fill["ms_min"], "fill_kernel_ms_max": fill["ms_max"],
            "offsets_scan_ms": round(statistics.median(stages["select_offsets_scan"][-steps:]), 4),
            "check_ms": round(statistics.median(stages["select_check"][-steps:]), 4), "moved_bytes": moved, "fill_gb_s": rate(moved, fill["ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024", help="corpus sizes in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("select_bench.py needs a GPU")
    hip = _hip()
    toks, scores, _ = synth.load_spec_vocab(32000)
    model = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
    V = model.vocab_size
    stream = torch.cuda.current_stream().cuda_stream
    for mib in [int(x) for x in args.sizes.split(",")]:
        flat, offs = synth.make_corpus(mib << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
        corpus = tgx.NativeCorpus(flat, offs)
        res = model.encode_corpus(corpus)
        S, T, N = res.num_samples, res.num_tokens, int(flat.size)
        rec = {"corpus_mib": mib, "bytes": N, "samples": S, "tokens": T, "mean_row": round(T / S, 1), "steps": args.steps, "runs": []}
        # the permutation alone
        d_shuffled = tgx.shuffled_rows(S, 1, res.device)
        t = timed(lambda: tgx.shuffled_rows(S, 1, res.device), args.steps, args.warmup)
        rec["runs"].append({"what": "shuffled_rows_device (call)", "n": S, **t})
        d_identity = torch.arange(S, dtype=torch.int64, device="cuda")
        orders = {"identity": (np.arange(S, dtype=np.int64), d_identity), "shuffled": (d_shuffled.cpu().numpy(), d_shuffled)}
        for what, obj, unit in (("result_select", res, 4), ("corpus_select", corpus, 1)):
            for order, (h_rows, d_rows) in orders.items():
                for path, rows in (("host", h_rows), ("device", d_rows)):
                    rec["runs"].append(select_run(obj, rows, what, order, path, unit, S, args.steps, args.warmup, stream))
        # (a) fim at rate 0 over the same result: a copy through the same per-tile search
        fill = []

        def fim_call():
            out = res.fim(V, V + 1, V + 2, rate=0.0, seed=1, stream=stream)
            fill.append(_lib.fim_last_times()["fim_fill_kernel"])
            out.free()
        whole = timed(fim_call, args.steps, args.warmup)
        f = spread(fill[-args.steps:])
        moved = 8 * T + 16 * (S + 1)
        rec["runs"].append({"what": "fim rate 0", "call_ms": whole["ms"], "call_ms_min": whole["ms_min"], "call_ms_max": whole["ms_max"],
                            "fill_kernel_ms": f["ms"], "fill_kernel_ms_min": f["ms_min"], "fill_kernel_ms_max": f["ms_max"], "moved_bytes": moved,
                            "fill_gb_s": rate(moved, f["ms"])})
        # (b) the floor: device-to-device copies of the outputs' bytes
        c_ids, c_text = d2d(hip, 4 * T, args.steps, args.warmup), d2d(hip, N, args.steps, args.warmup)
        rec["runs"].append({"what": "d2d ids", "bytes": 4 * T, **c_ids, "gb_s": rate(8 * T, c_ids["ms"])})
        rec["runs"].append({"what": "d2d text", "bytes": N, **c_text, "gb_s": rate(2 * N, c_text["ms"])})
        for run in rec["runs"]:
            if run["what"] == "result_select":
                run["fill_x_fim_fill"] = round(run["fill_kernel_ms"] / f["ms"], 2)
                run["fill_x_d2d"] = round(run["fill_kernel_ms"] / c_ids["ms"], 2)
            elif run["what"] == "corpus_select":
                run["fill_x_d2d"] = round(run["fill_kernel_ms"] / c_text["ms"], 2)
        print(json.dumps(rec), flush=True)
        del d_shuffled, d_identity, orders
        res.free()
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
