"""Unicode normalisation on the device (csrc/norm.hip: NativeCorpus.normalize) on bench.py's mixed corpus.  Three inputs, in
one run:

  plain     the corpus as it is under NFC: no piece, so the call is the mark pass and a device-to-device copy;
  accents   the same with 1 % of its identifiers rewritten to first letter + U+0301 + rest, under NFC: the slow path at work;
  nfkc      the corpus as it is under NFKC: its fullwidth punctuation changes.

Per input: the stages of the call (the library's events around each stage's kernels and scans: mark, pieces, length,
places, write) and the whole call; beside it a device-to-device hipMemcpyAsync of the same text, and the host route's wall
time: normalize_flat (host threads) + the upload of what it returns.  The device figures are device events on torch's
current stream around calls that return once their stream has reached its end, the median of --steps calls after --warmup,
as tools/front_bench.py; the host route is the median of --host-steps calls after one.  One JSON line per input.
usage: norm_bench.py [--size 256] [--steps 10] [--warmup 3] [--host-steps 3] [--inputs plain,accents,nfkc]"""
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
from assemble_bench import host_clock
from layout_bench import _hip, d2d, timed


def with_accents(flat: np.ndarray, offs: np.ndarray, every: int = 100):
    """U+0301 behind the first letter of every `every`-th identifier (a run of ASCII letters, digits and '_' that starts
    with a letter)"""
    word = np.zeros(256, bool)
    for lo, hi in ((0x30, 0x3A), (0x41, 0x5B), (0x61, 0x7B)):
        word[lo:hi] = True
    word[0x5F] = True
    letter = word.copy()
    letter[0x30:0x3A] = letter[0x5F] = False
    starts = np.nonzero(letter[flat] & ~np.concatenate(([False], word[flat[:-1]])))[0]
    starts = starts[~np.isin(starts, offs[:-1].astype(np.int64))][::every]   # (a row's first byte has no byte in front of it to ask)
    at = np.repeat(starts + 1, 2)
    out = np.insert(flat, at, np.tile(np.array([0xCC, 0x81], np.uint8), starts.size))
    new_offs = offs + 2 * np.searchsorted(starts, offs.astype(np.int64), side="left").astype(np.uint64)
    return np.ascontiguousarray(out), new_offs, int(starts.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="corpus size in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--inputs", default="plain,accents,nfkc")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("norm_bench.py needs a GPU")
    hip = _hip()
    flat0, offs0 = synth.make_corpus(args.size << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
    flat0 = np.ascontiguousarray(flat0)
    for name in args.inputs.split(","):
        form = "nfkc" if name == "nfkc" else "nfc"
        flat, offs, rewritten = with_accents(flat0, offs0) if name == "accents" else (flat0, offs0, 0)
        corpus = tgx.NativeCorpus(flat, offs)
        stages = []

        def normalize():
            out = corpus.normalize(form)
            stages.append(_lib.norm_last_times())
            return out
        call = timed(lambda: normalize().free(), args.steps, args.warmup)
        last = stages[-args.steps:]
        stage_ms = {k: round(statistics.median(s[k] for s in last), 4) for k in last[0]}
        # the device route against the host route, once
        out = normalize()
        want_f, want_o = _lib.normalize_flat(form, flat, offs)
        assert np.array_equal(out.offsets(), want_o) and np.array_equal(out.bytes(), want_f)
        pieces, out_bytes = int(out.n_pieces), int(want_f.size)
        out.free()
        del want_f, want_o
        copy = d2d(hip, int(flat.size), args.steps, args.warmup)

        def host_route():
            f, o = _lib.normalize_flat(form, flat, offs)
            tgx.NativeCorpus(f, o).free()   # the upload (synchronous)
        host_ms = host_clock(host_route, args.host_steps)
        host_norm_ms = host_clock(lambda: _lib.normalize_flat(form, flat, offs), args.host_steps)
        kernels = sum(stage_ms.values())
        rec = {"input": name, "form": form, "corpus_mib": args.size, "bytes": int(flat.size), "rows": int(offs.size - 1),
               "non_ascii_bytes": int((flat >= 0x80).sum()), "identifiers_rewritten": rewritten, "pieces": pieces, "out_bytes": out_bytes,
               "steps": args.steps, "stage_ms": stage_ms, "stages_ms": round(kernels, 4), "call_ms": call["ms"], "call_ms_min": call["ms_min"],
               "call_gb_s": round(flat.size / call["ms"] / 1e6, 1), "d2d_copy_ms": copy["ms"], "d2d_copy_ms_min": copy["ms_min"],
               "call_over_copy": round(call["ms"] / copy["ms"], 2), "host_normalize_flat_ms": host_norm_ms, "host_route_ms": host_ms,
               "host_over_call": round(host_ms / call["ms"], 2)}
        print(json.dumps(rec), flush=True)
        corpus.free()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
