"""SHA-256 digests of what the transforms of a resident result or corpus write, over the raw bytes of every output array
(not part of the pytest suite: run it on the GPU box).  It is the bit-for-bit comparison of two builds of the library: run
it once per build and compare the lines,

    python tests/measure/transform_digest.py [--root TREE] [--size-mb 8]

where TREE is the checkout whose tokengeex_amd is loaded (this one by default; the cases and the corpus always come from this
one's tests/ and synth).  One line per workload and array, `<workload> <array> <sha256>`; an array's digest runs over all
cases of its workload in order, and a call that raises contributes its message.

  * fim: tests/fim_cases.py's batches and its long row: ids, offsets, mode and cuts;
  * select ids / select bytes: tests/select_cases.py's batches and long rows, a result's and a corpus's rows;
  * front: tests/front_cases.py's fixed cases with the CRLF pass on and off: the segments' text and offsets, the plan, and
    the plan assembled over the segments' encode (the front end and the assembly);
  * norm: tests/norm_cases.py's edge batch in the four forms: bytes and offsets;
  * scan: tests/scan_cases.py's edge corpora of the first three vocabularies, encoded, through every layout below;
  * result: the corpus of test_assemble_gpu.py and test_decode_gpu.py (96 KiB of mixed text, empty rows, a 70 000-byte row)
    under the 32 000-token vocabulary, encoded, through every layout below, and assembled over test_assemble_gpu.py's
    first plan;
  * corpus: --size-mb MiB of synth's mixed corpus under the same vocabulary, encoded, through every layout below.

The layouts of a result: pad (ids, mask, lengths), pack (ids, doc, pos), windows (ids, mask, lengths, row, first), the flat,
padded and windowed spans in bytes and in characters as i32 and as i64, fim and select of the result, and the decode of the
result and of its padded tensor (bytes, offsets)."""
import argparse
import hashlib
import os
import sys
import traceback

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--size-mb", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.root))  # tokengeex_amd (and its libtgx.so) from TREE

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tokengeex_amd as tgx  # noqa: E402
from tokengeex_amd import _lib, synth, tensors  # noqa: E402

sys.path.insert(0, HERE)  # everything else, the case modules among it, from this checkout
import fim_cases  # noqa: E402
import front_cases  # noqa: E402
import norm_cases  # noqa: E402
import scan_cases  # noqa: E402
import select_cases  # noqa: E402

digests = {}
PAD, BOS, EOS = 3, 1, 2


def add(workload, name, value):
    h = digests.setdefault((workload, name), hashlib.sha256())
    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    h.update(value.encode() if isinstance(value, str) else np.ascontiguousarray(value).tobytes())


def guarded(workload, name, fn):
    """a call that raises contributes its message (and says so on stderr: stdout is for diff)"""
    try:
        fn()
    except Exception as ex:  # noqa: BLE001
        add(workload, name, type(ex).__name__ + ": " + str(ex))
        print(workload, name, "raised:", file=sys.stderr)
        traceback.print_exc(file=sys.stderr)


def add_result(workload, prefix, res):
    add(workload, prefix + ".ids", res.ids())
    add(workload, prefix + ".offsets", res.offsets())
    res.free()


def add_text(workload, prefix, text):
    add(workload, prefix + ".bytes", text.bytes())
    add(workload, prefix + ".offsets", text.offsets())
    text.free()


def fim_of(workload, res, pre, suf, mid, **kw):
    out, mode, cuts = res.fim(pre, suf, mid, return_info=True, **kw)
    add_result(workload, "fim", out)
    add(workload, "fim.mode", np.asarray(mode))
    add(workload, "fim.cuts", np.asarray(cuts))


def layouts(workload, res, model, specials):
    """every layout of a result whose ids are the model's (specials: the special tokens' bytes behind the vocabulary)"""
    S, V = res.num_samples, res.vocab_size
    L = 48
    for dt in (torch.int32, torch.int64):
        name = "i64" if dt == torch.int64 else "i32"

        def pad():
            p = tensors.to_padded(res, max_length=L, pad_id=PAD, bos_id=BOS, eos_id=EOS, dtype=dt, return_lengths=True)
            for k in sorted(p):
                add(workload, f"pad.{name}.{k}", p[k])
            if dt == torch.int32:
                add_text(workload, "decode_padded", tensors.decode_padded(model, p["input_ids"], attention_mask=p["attention_mask"],
                                                                         special_flat=specials[0], special_offs=specials[1]))

        def pack():
            p = tensors.to_packed(res, 512, pad_id=PAD, eos_id=EOS, dtype=dt, return_doc=True)
            for k in sorted(p):
                add(workload, f"pack.{name}.{k}", p[k])

        def windows():
            w = tensors.to_windows(res, max_length=L, stride=8, pad_id=PAD, bos_id=BOS, eos_id=EOS, dtype=dt, return_lengths=True)
            for k in sorted(w):
                add(workload, f"windows.{name}.{k}", w[k])

        guarded(workload, f"pad.{name}", pad)
        guarded(workload, f"pack.{name}", pack)
        guarded(workload, f"windows.{name}", windows)
        for unit in ("byte", "char"):
            sp = tuple(np.asarray(a) for a in specials)
            guarded(workload, f"spans.flat.{unit}.{name}", lambda: add(workload, f"spans.flat.{unit}.{name}", tensors.to_spans(res, model, sp, unit=unit, dtype=dt)))
            guarded(workload, f"spans.pad.{unit}.{name}", lambda: add(workload, f"spans.pad.{unit}.{name}", tensors.to_padded_spans(
                res, model, sp, unit=unit, dtype=dt, max_length=L, bos_id=BOS, eos_id=EOS)))
            guarded(workload, f"spans.windows.{unit}.{name}", lambda: add(workload, f"spans.windows.{unit}.{name}", tensors.to_window_spans(
                res, model, sp, unit=unit, dtype=dt, max_length=L, stride=8, bos_id=BOS, eos_id=EOS)))
    guarded(workload, "fim", lambda: fim_of(workload, res, V, V + 1, V + 2, rate=0.5, spm_rate=0.5, seed=3))
    rows = _lib.shuffled_rows_host(S, 5)[: max(1, S - S // 4)] if S else np.zeros(0, np.int64)
    guarded(workload, "select", lambda: add_result(workload, "select", res.select(rows)))
    guarded(workload, "decode", lambda: add_text(workload, "decode", model.decode_result(res, specials[0], specials[1], True)))


print("tokengeex_amd from", os.path.dirname(os.path.abspath(tgx.__file__)), file=sys.stderr, flush=True)  # (stdout is for diff)
if tgx.device_count() < 1:
    raise SystemExit("transform_digest needs a GPU: no usable HIP device")

# ---- the cases of the suite ------------------------------------------------------------------------------------------
for case in [fim_cases.batch(k) for k in range(fim_cases.N_BATCHES)] + [fim_cases.long_row()]:
    src = _lib.NativeResult.from_ids(case["ids"], case["offs"], case["vocab_size"])
    guarded("fim", "fim", lambda: fim_of("fim", src, case["pre"], case["suf"], case["mid"], **fim_cases.args(case)))
    src.free()

for kind in ("ids", "bytes"):
    for case in [select_cases.batch(k, kind) for k in range(select_cases.N_BATCHES)] + [select_cases.long_row(kind)]:
        if kind == "ids":
            src = _lib.NativeResult.from_ids(case["data"], case["offs"], case["vocab_size"])
            guarded("select ids", "select", lambda: add_result("select ids", "select", src.select(case["rows"])))
        else:
            src = _lib.NativeCorpus(case["data"], case["offs"])
            guarded("select bytes", "select", lambda: add_text("select bytes", "select", src.select(case["rows"])))
        src.free()

toks, scores, _ = synth.load_spec_vocab(32000)
spec = tgx.NativeModel(list(toks), np.asarray(scores, np.float64))
no_specials = (np.zeros(0, np.uint8), np.zeros(1, np.uint64))


def front(samples, specials, crlf):
    corpus = tgx.NativeCorpus(*tgx.pack(samples))
    segs, plan = corpus.split_specials(specials, crlf)
    add("front", "segments.bytes", segs.bytes())
    add("front", "segments.offsets", segs.offsets())
    add("front", "plan.seg_offs", plan.seg_offs())
    add("front", "plan.seg_special", plan.seg_special())
    enc = spec.encode_corpus(segs) if plan.num_encoded else None
    add_result("front", "assembled", spec.assemble_plan(enc, plan, len(specials)))
    for h in (enc, segs, plan, corpus):
        if h is not None:
            h.free()


for name, samples, specials in front_cases.fixed_cases():
    for crlf in (False, True):
        guarded("front", name, lambda: front(samples, specials, crlf))

edge = tgx.NativeCorpus(*tgx.pack(list(norm_cases.edge_batch())))
for form in norm_cases.FORMS:
    guarded("norm", form, lambda: add_text("norm", form, edge.normalize(form)))
edge.free()

for vname in scan_cases.VOCABS[:3]:
    vt, vs = scan_cases.vocab(vname)[:2]
    model = tgx.NativeModel(list(vt), np.asarray(vs, np.float64))
    for tail in scan_cases.TAILS:
        def scan_case():
            flat, offs = scan_cases.corpus(vname, "edges", tail)[:2]
            res = model.encode_batch_flat(np.asarray(flat, np.uint8), np.asarray(offs, np.uint64))
            layouts("scan", res, model, no_specials)
            res.free()
        guarded("scan", "encode", scan_case)
    model.free()

# ---- the corpus of the assemble and decode GPU tests ---------------------------------------------------------------------
flat, offs = synth.make_corpus(96 << 10, "mixed", max_len=4096, seed_offset=3)
big, _ = synth.make_corpus(80_000, "mixed", min_len=70_000, max_len=70_000, seed_offset=4)
rows = [bytes(flat[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
half = len(rows) // 2
texts = [b"", b""] + rows[:half] + [b"", b"", b""] + [bytes(big[:70_000])] + rows[half:] + [b""]
SPECIALS = [s.encode() for s in ["<|endoftext|>", "<|fim", "<|fim|>", "<pad>", "<s>", "</s>"]]
sp_arrays = _lib.pack(SPECIALS)
res = spec.encode_batch_flat(*tgx.pack(texts))
layouts("result", res, spec, no_specials)
# test_assemble_gpu.py's shape of plan: a special token in front of every second segment, three segments to a sample
E = res.num_samples
items = []
for e in range(E):
    if e % 2 == 0:
        items.append(e % len(SPECIALS))
    items.append(-1)
seg_offs = np.unique(np.append(np.arange(0, len(items), 3), len(items))).astype(np.uint64)
asm = spec.assemble(res, seg_offs, np.asarray(items, np.int32), len(SPECIALS))
add("result", "assembled.ids", asm.ids())
add("result", "assembled.offsets", asm.offsets())
layouts("assembled", asm, spec, sp_arrays)
asm.free()
res.free()

# ---- the mixed corpus ------------------------------------------------------------------------------------------------------
flat, offs = synth.make_corpus(args.size_mb << 20, "mixed", max_len=65536, seed_offset=1000)
corpus = tgx.NativeCorpus(flat, offs)
res = spec.encode_corpus(corpus)
layouts("corpus", res, spec, no_specials)
rows = _lib.shuffled_rows_host(corpus.num_samples, 9)
guarded("corpus", "select bytes", lambda: add_text("corpus", "select bytes", corpus.select(rows)))
res.free()

for (workload, name), h in digests.items():
    print(workload, name, h.hexdigest(), flush=True)
