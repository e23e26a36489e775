"""The device assembly of special-token ids (csrc/assemble.hip) on bench.py's mixed corpus with the spec 32 000 vocabulary
and special tokens written into the text under two plans:

  fim   four specials per sample: <fim_prefix> at its start, <fim_suffix> and <fim_middle> at one and two thirds, <|endoftext|> at its end;
  chat  a role marker (<|user|> / <|asst|>) at the start of every sample and then every 64 bytes.

Per plan, in one run:
  (a) assemble_fill_kernel (the library's events around the launch) and the whole NativeModel.assemble call;
  (b) layout_pack_kernel int32 over the same number of output ids (tensors.pack_into on the assembled result, no bos / eos):
      the yardstick, a per-tile search plus a 4-byte gather of the same shape;
  (c) the encode pass over the plan's non-special segments (sum of its kernels), so the share of assembly is visible;
  (d) end to end on the host clock: Tokenizer.encode_batch_packed_flat(block_len=4096) against the route without the device
      assembly: encode_batch_flat -> layout_pack_host -> torch.from_numpy().cuda().

(a) and (b) are device events on torch's current stream around calls that return once their stream has reached its end,
the median of --steps calls after --warmup, as tools/layout_bench.py; (d) is the median of --e2e-steps calls after one.
One JSON line per plan.   usage: assemble_bench.py [--size 256] [--steps 10] [--warmup 3] [--e2e-steps 3] [--no-e2e]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import tokengeex_amd as tgx
from tokengeex_amd import _lib, synth, tensors
from layout_bench import timed

FIM = ["<fim_prefix>", "<fim_suffix>", "<fim_middle>"]   # of one length: written in one pass
EOT = "<|endoftext|>"
ROLES = ["<|user|>", "<|asst|>"]
SPECIALS = FIM + [EOT] + ROLES + ["<pad>"]


def _to_char_start(flat, pos, end):
    """positions moved forward off UTF-8 continuation bytes (a special token is not written into a character)"""
    pos = pos.copy()
    for _ in range(3):
        inside = pos < end
        cont = np.zeros(pos.shape, bool)
        cont[inside] = (flat[pos[inside]] & 0xC0) == 0x80
        pos[cont] += 1
    return pos


def _insert(flat, offs, pos, sample, words):
    """words[k] (all of one length) written before byte pos[k] of the text, for sample[k] -> (flat, offs)"""
    m = len(words[0])
    assert all(len(w) == m for w in words) and np.all(np.diff(pos) >= 0)
    table = np.frombuffer("".join(words).encode(), np.uint8).reshape(len(words), m)
    values = table[np.arange(pos.size) % len(words)].reshape(-1)
    out = np.insert(flat, np.repeat(pos, m), values)
    grown = np.zeros(offs.size, np.int64)
    np.cumsum(np.bincount(sample, minlength=offs.size - 1) * m, out=grown[1:])
    return out, (offs.astype(np.int64) + grown).astype(np.uint64)


def with_specials(flat, offs, plan):
    o = offs.astype(np.int64)
    b, e = o[:-1], o[1:]
    n = e - b
    S = n.size
    if plan == "fim":
        pos = np.stack([b, b + n // 3, b + 2 * n // 3], axis=1).reshape(-1)
        pos = np.maximum.accumulate(_to_char_start(flat, pos, np.repeat(e, 3)))
        flat, offs = _insert(flat, offs, pos, np.repeat(np.arange(S), 3), FIM)
        ends = offs.astype(np.int64)[1:]
        return _insert(flat, offs, ends, np.arange(S), [EOT])
    k = np.where(n > 0, -(-n // 64), 0)
    sample = np.repeat(np.arange(S), k)
    j = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)
    pos = np.maximum.accumulate(_to_char_start(flat, b[sample] + 64 * j, e[sample]))
    return _insert(flat, offs, pos, sample, ROLES)


def host_route(tk, flat, offs, block_len, pad):
    ids, o = tk.encode_batch_flat(flat, offs)
    h = _lib.layout_pack_host(ids, o, block_len, pad, dtype=np.int64)
    t = torch.from_numpy(h["input_ids"]).cuda()
    torch.cuda.synchronize()
    return t


def device_route(tk, flat, offs, block_len, pad):
    t = tk.encode_batch_packed_flat(flat, offs, block_len, pad_id=pad)["input_ids"]
    torch.cuda.synchronize()
    return t


def host_clock(fn, steps):
    fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="corpus size in MiB")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-steps", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true", help="skip (d)")
    ap.add_argument("--plans", default="fim,chat")
    args = ap.parse_args()
    if tgx.device_count() < 1:
        raise SystemExit("assemble_bench.py needs a GPU")
    toks, scores, _ = synth.load_spec_vocab(32000)
    tk = tgx.Tokenizer([(t, float(s), False) for t, s in zip(toks, scores)], [], SPECIALS)
    model = tk._model()
    pad = tk.special_token_to_id("<pad>")
    flat0, offs0 = synth.make_corpus(args.size << 20, "mixed", seed_offset=1000)   # bench.py's corpus of rank 0
    for plan in args.plans.split(","):
        flat, offs = with_specials(flat0, offs0, plan)
        seg_offs, ss, pflat, poffs = tk._split_segments(flat, offs)
        K, E, S = int(ss.size), int(poffs.size - 1), int(offs.size - 1)
        segs = model.encode_batch_flat(pflat, poffs)
        encode = model.last_kernel_times()
        fill_ms, scan_ms, starts_ms = [], [], []

        def assemble():
            r = model.assemble(segs, seg_offs, ss, len(SPECIALS))
            kt = model.last_kernel_times()
            fill_ms.append(kt["assemble_fill_kernel"])
            scan_ms.append(kt["assemble_ranks_scan"])
            starts_ms.append(kt["assemble_starts_kernel"])
            return r
        call = timed(lambda: assemble().free(), args.steps, args.warmup)
        res = assemble()
        n_out = res.num_tokens
        # the assembled ids against the host loop, once
        want_ids, want_offs = _lib.assemble_ids(seg_offs, ss, segs.ids(), segs.offsets(), tk.base_vocab_size())
        assert np.array_equal(res.ids(), want_ids) and np.array_equal(res.offsets(), want_offs)
        del want_ids, want_offs
        L = 4096
        B = -(-n_out // L)
        out = torch.empty((B, L), dtype=torch.int32, device="cuda")
        pack = timed(lambda: tensors.pack_into(res, out, block_len=L, pad_id=pad), args.steps, args.warmup)
        del out
        last = args.steps   # the timed calls (the warm-up ones come first)
        fill = round(statistics.median(fill_ms[-last - 1:-1]), 4)
        rec = {"plan": plan, "corpus_mib": args.size, "bytes": int(flat.size), "samples": S, "segments": K, "encoded_segments": E,
               "specials": K - E, "ids_out": int(n_out), "steps": args.steps,
               "assemble_fill_kernel_ms": fill, "assemble_fill_kernel_ms_min": round(min(fill_ms[-last - 1:-1]), 4),
               "assemble_ranks_scan_ms": round(statistics.median(scan_ms[-last - 1:-1]), 4),
               "assemble_starts_kernel_ms": round(statistics.median(starts_ms[-last - 1:-1]), 4),
               "assemble_call_ms": call["ms"], "assemble_call_ms_min": call["ms_min"], "plan_upload_bytes": 8 * (S + 1) + 4 * K,
               "fill_gb_s": round(8 * n_out / fill / 1e6, 1),
               "layout_pack_i32_call_ms": pack["ms"], "layout_pack_i32_call_ms_min": pack["ms_min"],
               "fill_over_pack": round(fill / pack["ms"], 2),
               "encode_ms": round(sum(encode.values()), 3), "encode_kernels": {k: round(v, 3) for k, v in encode.items()}}
        res.free()
        segs.free()
        if not args.no_e2e:
            a, b = device_route(tk, flat, offs, L, pad), host_route(tk, flat, offs, L, pad)
            assert torch.equal(a, b)
            del a, b
            dev = host_clock(lambda: device_route(tk, flat, offs, L, pad), args.e2e_steps)
            host = host_clock(lambda: host_route(tk, flat, offs, L, pad), args.e2e_steps)
            rec.update({"e2e_block_len": L, "e2e_device_route_ms": dev, "e2e_host_route_ms": host, "e2e_host_over_device": round(host / dev, 2)})
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
