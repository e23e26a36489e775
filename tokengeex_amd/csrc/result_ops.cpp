// The C ABI's transforms of a resident result (include/tgx.h): layouts and windows, assembly, fill-in-the-middle, row
// selection and the seeded permutation, decode and the text handle, spans.  They run on the caller's stream under a StreamGuard (assembly: on the model's,
// under a Pass) and share device_internal.h with the passes (tgx_api.cpp, encode_pass.cpp, estep_pass.cpp, lattice_pass.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "assemble.h"
#include "decode.h"
#include "dedup.h"
#include "fim.h"
#include "kernels.h"
#include "layout.h"
#include "pass_internal.h"  // (the knobs: TGX_DEDUP_HASH_BITS)
#include "select.h"
#include "spans.h"

using namespace tgx::host;
using namespace tgx::dev;

// ---- layouts: padded rows / packed blocks of a result, in caller-owned device memory (layout.hip) ----------------

tgx_status tgx_result_layout_info(const tgx_result* r, uint32_t bos_id, uint32_t eos_id, uint64_t* max_row_len, uint64_t* n_stream) {
    if (!r) return fail(TGX_ERR_INVALID, "tgx_result_layout_info: result is NULL");
    const uint64_t A = (bos_id != TGX_NO_ID ? 1 : 0) + (eos_id != TGX_NO_ID ? 1 : 0);
    if (n_stream) *n_stream = r->n_tokens + r->n_samples * A;
    if (!max_row_len) return TGX_OK;
    *max_row_len = A;
    if (r->n_samples == 0 || r->n_tokens == 0) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    hipStream_t st = stream_or_default(nullptr, r->device);
    unsigned long long h_max = 0, *d_max = nullptr;
    StreamGuard guard(r->device, st);
    HIP_TRY(guard.alloc(sizeof(unsigned long long), &d_max));
    HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(unsigned long long), st));
    HIP_TRY(tgx::launch_layout_max_row(r->d_offs, r->n_samples, d_max, st));
    const tgx_status rst = read_u64(st, d_max, &h_max);
    if (rst != TGX_OK) return rst;
    guard.done();
    *max_row_len = h_max + A;
    return TGX_OK;
}

tgx_status tgx_result_pad_device(const tgx_result* r, uint32_t row_len, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id,
                                 uint32_t flags, void* stream, void* d_ids, uint8_t* d_mask, int32_t* d_lengths,
                                 uint64_t* n_truncated) {
    const char* who = "tgx_result_pad_device";
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if (!d_ids && r->n_samples) return fail(TGX_ERR_INVALID, "%s: d_ids is NULL", who);
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT | TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    if (r->vocab_size > 0x80000000u) return fail(TGX_ERR_INVALID, "%s: the model's ids are not all below 2^31", who);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    if ((st = layout_check_row_len(who, row_len, seq.extra)) != TGX_OK) return st;
    if (n_truncated) *n_truncated = 0;
    if (r->n_samples == 0) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    if ((st = check_device_ptr(who, "d_ids", d_ids, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_mask", d_mask, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_lengths", d_lengths, r->device, "result")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, r->device);
    unsigned long long h_count = 0, *d_count = nullptr;
    StreamGuard guard(r->device, hs);
    if (n_truncated) HIP_TRY(guard.alloc(sizeof(unsigned long long), &d_count));
    tgx::LayoutParams p = {};
    p.ids = r->d_ids;
    p.offs = r->d_offs;
    p.n_rows = r->n_samples;
    p.len = row_len;
    p.pad = pad_id;
    p.bos = bos_id;
    p.eos = eos_id;
    p.flags = flags;
    p.out = d_ids;
    p.mask = d_mask;
    p.lengths = d_lengths;
    p.counter = d_count;
    if (n_truncated) HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), hs));
    HIP_TRY(tgx::launch_layout_pad(p, hs));
    if (n_truncated) HIP_TRY(hipMemcpyAsync(&h_count, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, hs));
    // the stream has reached its end before the result or the destination can change hands (the guard: also after a failure)
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    if (n_truncated) *n_truncated = h_count;
    return TGX_OK;
}

tgx_status tgx_result_pack_device(const tgx_result* r, uint32_t block_len, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id,
                                  uint32_t flags, void* stream, void* d_ids, int32_t* d_doc, int32_t* d_pos, uint64_t* n_blocks) {
    const char* who = "tgx_result_pack_device";
    if (!r || !n_blocks) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    if (r->vocab_size > 0x80000000u) return fail(TGX_ERR_INVALID, "%s: the model's ids are not all below 2^31", who);
    if (block_len < 1) return fail(TGX_ERR_INVALID, "%s: block_len is 0", who);
    if (r->n_samples >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^31 rows or more", who);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    const uint64_t n_stream = r->n_tokens + r->n_samples * seq.extra;
    const uint64_t nb = (n_stream + block_len - 1) / block_len;
    *n_blocks = nb;
    if (nb == 0) return TGX_OK;
    if (!d_ids) return fail(TGX_ERR_INVALID, "%s: d_ids is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    if ((st = check_device_ptr(who, "d_ids", d_ids, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_doc", d_doc, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_pos", d_pos, r->device, "result")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, r->device);
    tgx::LayoutParams p = {};
    p.ids = r->d_ids;
    p.offs = r->d_offs;
    p.n_rows = r->n_samples;
    p.len = block_len;
    p.pad = pad_id;
    p.bos = bos_id;
    p.eos = eos_id;
    p.flags = flags;
    p.out = d_ids;
    p.doc = d_doc;
    p.pos = d_pos;
    StreamGuard guard(r->device, hs);
    HIP_TRY(tgx::launch_layout_pack(p, n_stream, nb * block_len, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

// ---- overflow windows: long rows as overlapping [W, L] windows (layout.hip; layout.h has the window mapping) ---------

namespace {

// Wo = the rows' first windows, in pooled scratch of the guard (u64[S+1]), and *n_windows = W = Wo[S], for a result with
// S >= 1 rows: the count kernel, the scan, and one read-back of W and the longest row, which are checked against 2^31.
// The stream has reached its end when this returns TGX_OK.
tgx_status window_offsets_device(const char* who, const tgx_result* r, uint32_t room, uint32_t step, hipStream_t hs, StreamGuard& guard,
                                 const uint64_t** d_wo, uint64_t* n_windows) {
    const uint64_t S = r->n_samples;
    size_t scan_bytes = 0;
    if (tgx::scan_temp_bytes(S, &scan_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan temp-size query failed");
    uint32_t* counts = nullptr;
    uint64_t* wo = nullptr;  // Wo[0 .. S], then the longest row
    void* scan = nullptr;
    HIP_TRY(guard.alloc((size_t)(S + 1) * 4, &counts));
    HIP_TRY(guard.alloc((size_t)(S + 2) * 8, &wo));
    if (scan_bytes) HIP_TRY(guard.alloc(scan_bytes, &scan));
    HIP_TRY(hipMemsetAsync(wo + S + 1, 0, 8, hs));
    HIP_TRY(tgx::launch_layout_window_count(r->d_offs, S, room, step, counts, reinterpret_cast<unsigned long long*>(wo + S + 1), hs));
    HIP_TRY(tgx::launch_scan(counts, wo, S, scan, scan_bytes, hs));
    uint64_t h[2] = {0, 0};
    tgx_status st = read_u64(hs, wo + S, h, 2);
    if (st == TGX_OK) st = window_check_totals(who, h[1], h[0], nullptr);
    if (st != TGX_OK) return st;
    *d_wo = wo;
    *n_windows = h[0];
    return TGX_OK;
}

}  // namespace

tgx_status tgx_result_window_info(const tgx_result* r, uint32_t row_len, uint32_t stride, uint32_t bos_id, uint32_t eos_id, uint32_t flags,
                                  uint64_t* n_windows) {
    const char* who = "tgx_result_window_info";
    if (!r || !n_windows) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT | TGX_LAYOUT_I64 | TGX_SPAN_CHARS);
    if (st == TGX_OK) st = layout_check_ids(who, 0, bos_id, eos_id);
    if (st != TGX_OK) return st;
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, 0);
    if ((st = window_check_args(who, row_len, stride, seq.extra)) != TGX_OK) return st;
    *n_windows = 0;
    if (r->n_samples == 0) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    hipStream_t hs = stream_or_default(nullptr, r->device);
    StreamGuard guard(r->device, hs);
    const uint64_t* d_wo = nullptr;
    st = window_offsets_device(who, r, row_len - seq.extra, row_len - seq.extra - stride, hs, guard, &d_wo, n_windows);
    if (st == TGX_OK) guard.done();
    return st;
}

tgx_status tgx_result_window_pad_device(const tgx_result* r, uint32_t row_len, uint32_t stride, uint32_t pad_id, uint32_t bos_id, uint32_t eos_id,
                                        uint32_t flags, void* stream, uint64_t n_windows, void* d_ids, uint8_t* d_mask, int32_t* d_lengths,
                                        int32_t* d_window_row, int32_t* d_window_first) {
    const char* who = "tgx_result_window_pad_device";
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if (!d_ids && r->n_samples) return fail(TGX_ERR_INVALID, "%s: d_ids is NULL", who);
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_PAD_LEFT | TGX_LAYOUT_TRUNC_LEFT | TGX_LAYOUT_I64);
    if (st == TGX_OK) st = layout_check_ids(who, pad_id, bos_id, eos_id);
    if (st != TGX_OK) return st;
    if (r->vocab_size > 0x80000000u) return fail(TGX_ERR_INVALID, "%s: the model's ids are not all below 2^31", who);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, pad_id);
    if ((st = window_check_args(who, row_len, stride, seq.extra)) != TGX_OK) return st;
    if (r->n_samples == 0) return window_check_totals(who, 0, 0, &n_windows);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    if ((st = check_device_ptr(who, "d_ids", d_ids, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_mask", d_mask, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_lengths", d_lengths, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_window_row", d_window_row, r->device, "result")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_window_first", d_window_first, r->device, "result")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, r->device);
    StreamGuard guard(r->device, hs);
    const uint64_t* d_wo = nullptr;
    uint64_t W = 0;
    st = window_offsets_device(who, r, row_len - seq.extra, row_len - seq.extra - stride, hs, guard, &d_wo, &W);
    if (st == TGX_OK) st = window_check_totals(who, 0, W, &n_windows);
    if (st != TGX_OK) return st;
    tgx::WindowParams q = {};
    q.base.ids = r->d_ids;
    q.base.offs = r->d_offs;
    q.base.n_rows = r->n_samples;
    q.base.len = row_len;
    q.base.pad = pad_id;
    q.base.bos = bos_id;
    q.base.eos = eos_id;
    q.base.flags = flags;
    q.base.out = d_ids;
    q.base.mask = d_mask;
    q.base.lengths = d_lengths;
    q.wo = d_wo;
    q.stride = stride;
    q.window_row = d_window_row;
    q.window_first = d_window_first;
    HIP_TRY(tgx::launch_layout_windows(q, W, hs));
    // the stream has reached its end before the result or the destination can change hands (the guard: also after a failure)
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

// ---- assembly: a sample-level result with the special tokens' ids, from the segment-level result (assemble.hip) ----

namespace {

// What tgx_assemble_result and tgx_assemble_result_plan share: everything after the checks of the plan itself.  The plan
// is K segments of S samples, E of them encoded, in host arrays that are uploaded (h_*) or in device memory (d_*: d_special
// with room for K + 1 entries).
tgx_status assemble_device(const char* who, tgx_model* m, const tgx_result* segs, const uint64_t* h_seg_offs, const int32_t* h_special,
                           const uint64_t* d_plan_offs, int32_t* d_plan_special, uint64_t S, uint64_t K, uint32_t n_specials, tgx_result** out) {
    if (segs && segs->device != m->device)
        return fail(TGX_ERR_INVALID, "%s: the result is on device %d, the model on device %d", who, segs->device, m->device);
    if (segs && segs->vocab_size != m->vocab_size)
        return fail(TGX_ERR_INVALID, "%s: the result was written for %u tokens, the model has %u", who, segs->vocab_size, m->vocab_size);
    const uint64_t E = segs ? segs->n_samples : 0;
    const uint64_t n_out = (segs ? segs->n_tokens : 0) + (K - E);

    std::lock_guard<std::mutex> lk(m->mu);
    HIP_TRY(hipSetDevice(m->device));
    m->n_timed = 0;
    Pass pass(m);
    tgx_result* r = pass.new_result(S);
    r->vocab_size = m->vocab_size + n_specials;
    r->n_tokens = n_out;
    uint64_t *d_seg_offs = nullptr, *d_rank = nullptr, *d_starts = nullptr, *d_zero = nullptr;
    int32_t* d_special = d_plan_special;
    ScanScratch scan;
    if (r->d_offs.alloc(m->device, (size_t)(S + 1) * 8) != hipSuccess || r->d_ids.alloc(m->device, (size_t)n_out * 4 + 256) != hipSuccess ||
        (!d_plan_offs && pass.alloc((size_t)(S + 1) * 8, &d_seg_offs) != hipSuccess) ||
        (!d_plan_special && pass.alloc((size_t)(K + 1) * 4, &d_special) != hipSuccess) ||
        pass.alloc((size_t)(K + 1) * 8, &d_rank) != hipSuccess || pass.alloc((size_t)(K + 1) * 8, &d_starts) != hipSuccess ||
        (E == 0 && pass.alloc(8, &d_zero) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "out of device memory (assembly)");
    const tgx_status scan_st = scan_room(&scan, pass, tgx::assemble_scan_temp_bytes, K, "out of device memory (assembly)");
    if (scan_st != TGX_OK) return scan_st;
    if ((!d_plan_offs && hipMemcpyAsync(d_seg_offs, h_seg_offs, (size_t)(S + 1) * 8, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
        (!d_plan_special && K && hipMemcpyAsync(d_special, h_special, (size_t)K * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
        (d_zero && hipMemsetAsync(d_zero, 0, 8, m->stream) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "upload of the split plan failed: %s", hipGetErrorString(hipGetLastError()));

    tgx::AssembleParams p = {};
    p.ids = E ? segs->d_ids.get() : nullptr;
    p.offs = E ? segs->d_offs.get() : d_zero;
    p.seg_offs = d_plan_offs ? d_plan_offs : d_seg_offs;
    p.seg_special = d_special;
    p.rank = d_rank;
    p.starts = d_starts;
    p.n_segs = K;
    p.n_samples = S;
    p.n_out = n_out;
    p.vocab_size = m->vocab_size;
    p.out_ids = r->d_ids;
    p.out_offs = r->d_offs;
    time_begin(m, "assemble_ranks_scan");
    if (tgx::launch_assemble_ranks(d_special, d_rank, K, scan.ptr, scan.bytes, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "scan launch failed");
    time_end(m);
    time_begin(m, "assemble_starts_kernel");
    if (tgx::launch_assemble_starts(p, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "assemble_starts_kernel launch failed");
    time_end(m);
    time_begin(m, "assemble_fill_kernel");
    if (tgx::launch_assemble_fill(p, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "assemble_fill_kernel launch failed");
    time_end(m);
    if (hipStreamSynchronize(m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "assembly failed: %s", hipGetErrorString(hipGetLastError()));
    *out = pass.release_result();
    return pass.done();
}

}  // namespace

tgx_status tgx_assemble_result(tgx_model* m, const tgx_result* segs, const uint64_t* seg_offs, const int32_t* seg_special,
                               uint64_t n_samples, uint32_t n_specials, tgx_result** out) {
    const char* who = "tgx_assemble_result";
    const tgx_status dst = require_device();
    if (dst != TGX_OK) return dst;
    if (!m || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    uint64_t K = 0;
    const tgx_status cst = assemble_check(who, seg_offs, seg_special, n_samples, m->vocab_size, n_specials, segs != nullptr, segs ? segs->n_samples : 0, &K);
    if (cst != TGX_OK) return cst;
    return assemble_device(who, m, segs, seg_offs, seg_special, nullptr, nullptr, n_samples, K, n_specials, out);
}

tgx_status tgx_assemble_result_plan(tgx_model* m, const tgx_result* segs, const tgx_plan* plan, uint32_t n_specials, tgx_result** out) {
    const char* who = "tgx_assemble_result_plan";
    const tgx_status dst = require_device();
    if (dst != TGX_OK) return dst;
    if (!m || !plan || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    // what assemble_check asks of host arrays, of a plan whose arrays the split wrote
    if ((uint64_t)m->vocab_size + n_specials > 0xFFFFFFFEull)
        return fail(TGX_ERR_INVALID, "%s: %u tokens and %u special tokens leave no room for their ids", who, m->vocab_size, n_specials);
    if (n_specials != plan->n_specials)
        return fail(TGX_ERR_INVALID, "%s: %u special tokens, the plan was made with %u", who, n_specials, plan->n_specials);
    if (plan->n_enc && !segs) return fail(TGX_ERR_INVALID, "%s: %llu encoded segments and no result over them", who, (unsigned long long)plan->n_enc);
    if (plan->n_enc != (segs ? segs->n_samples : 0))
        return fail(TGX_ERR_INVALID, "%s: %llu encoded segments, the result over them has %llu rows", who, (unsigned long long)plan->n_enc,
                    (unsigned long long)(segs ? segs->n_samples : 0));
    if (plan->device != m->device) return fail(TGX_ERR_INVALID, "%s: the plan is on device %d, the model on device %d", who, plan->device, m->device);
    return assemble_device(who, m, segs, nullptr, nullptr, plan->d_seg_offs, plan->d_special, plan->n_samples, plan->n_segs, n_specials, out);
}

// ---- decode: ids in HBM to UTF-8 text in HBM (decode.hip; decode.h has the index arithmetic) ----------------------

namespace {

uint64_t decode_elem_bytes(uint32_t kind) { return kind == tgx::kDecodeI64 ? 8 : 4; }

// the model's token tables on its device, once (under m->mu)
tgx_status ensure_decode_tables(tgx_model* m) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->decode_tables_ready) return TGX_OK;
    const uint32_t V = m->vocab_size;
    std::vector<uint8_t> len;
    std::vector<tgx::DecodeSlot> slots;
    const tgx_status st = decode_build_tables("decode", m->vocab_bytes.data(), m->vocab_offs.data(), V, &len, &slots);
    if (st != TGX_OK) return st;
    const size_t nb = m->vocab_bytes.size();
    if (!m->d_dec_len) HIP_TRY(hipMalloc((void**)&m->d_dec_len, (size_t)V + 16));
    if (!m->d_dec_slots) HIP_TRY(hipMalloc(&m->d_dec_slots, ((size_t)V + 1) * sizeof(tgx::DecodeSlot)));
    if (!m->d_dec_bytes) HIP_TRY(hipMalloc((void**)&m->d_dec_bytes, nb + 16));
    if (!m->d_dec_offs) HIP_TRY(hipMalloc((void**)&m->d_dec_offs, ((size_t)V + 1) * 8));
    if (V) HIP_TRY(hipMemcpy(m->d_dec_len, len.data(), V, hipMemcpyHostToDevice));
    if (V) HIP_TRY(hipMemcpy(m->d_dec_slots, slots.data(), (size_t)V * sizeof(tgx::DecodeSlot), hipMemcpyHostToDevice));
    if (nb) HIP_TRY(hipMemcpy(m->d_dec_bytes, m->vocab_bytes.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_dec_offs, m->vocab_offs.data(), ((size_t)V + 1) * 8, hipMemcpyHostToDevice));
    m->decode_tables_ready = true;
    return TGX_OK;
}

// The decode of src (device pointers) on stream hs of the model's device, which is current.  row_offs_dev: the offsets
// form's offsets, read back only to name the row of an out-of-bounds id.
tgx_status decode_device(tgx_model* m, tgx::DecodeSrc src, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials,
                         int include_special, hipStream_t hs, tgx_text** out, uint64_t* bad_sample, uint64_t* bad_id) {
    const int dev = m->device;
    const uint64_t S = src.n_rows, N = src.n;
    std::unique_ptr<tgx_text> text(new tgx_text());
    PoolBuf<uint8_t> raw;          // the raw bytes: the text's own when nothing is replaced
    std::vector<uint64_t> h_offs;  // the offsets form's offsets, read back to name the row of an out-of-bounds id
    StreamGuard guard(dev, hs);    // destroyed before them: a failed call's queued work is over before they go
    uint32_t *meta = nullptr, *flags = nullptr, *codes = nullptr;
    uint64_t *starts = nullptr, *specials = nullptr, *gpos = nullptr, *sp_offs = nullptr;
    uint8_t* sp_bytes = nullptr;
    ScanScratch scan, scan2;
    unsigned long long* ctrl = nullptr;  // [0]: lowest out-of-bounds position, [1]: replacement characters, [2]: live specials
    tgx_text* t = text.get();
    t->device = dev;
    t->n_rows = S;
    HIP_TRY(t->d_offs.alloc(dev, (size_t)(S + 1) * 8));
    if (S == 0 || N == 0) {
        HIP_TRY(t->d_bytes.alloc(dev, 0));
        HIP_TRY(hipMemsetAsync(t->d_offs, 0, (size_t)(S + 1) * 8, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        guard.done();
        *out = text.release();
        return TGX_OK;
    }
    tgx_status st = ensure_decode_tables(m);
    if (st != TGX_OK) return st;

    const uint64_t sp_total = n_specials ? special_offs[n_specials] - special_offs[0] : 0;
    HIP_TRY(guard.alloc((size_t)(N + 1) * 4, &meta));
    HIP_TRY(guard.alloc((size_t)(N + 1) * 8, &starts));
    if ((st = scan_room(&scan, guard, tgx::decode_scan_temp_bytes, N)) != TGX_OK) return st;
    HIP_TRY(guard.alloc(24, &ctrl));
    HIP_TRY(guard.alloc(((size_t)n_specials + 1) * 8, &sp_offs));
    HIP_TRY(guard.alloc((size_t)sp_total + 16, &sp_bytes));
    std::vector<uint64_t> sp_offs0((size_t)n_specials + 1, 0);  // from 0
    for (uint32_t k = 0; k <= n_specials && n_specials; k++) sp_offs0[k] = special_offs[k] - special_offs[0];
    HIP_TRY(guard.upload(sp_offs, std::move(sp_offs0)));
    if (sp_total) HIP_TRY(hipMemcpyAsync(sp_bytes, special_bytes + special_offs[0], sp_total, hipMemcpyHostToDevice, hs));
    HIP_TRY(hipMemsetAsync(ctrl, 0xFF, 8, hs));
    HIP_TRY(hipMemsetAsync(ctrl + 1, 0, 16, hs));

    tgx::DecodeParams p = {};
    p.tab.tok_len = m->d_dec_len;
    p.tab.slots = static_cast<const tgx::DecodeSlot*>(m->d_dec_slots);
    p.tab.bytes = m->d_dec_bytes;
    p.tab.offs = m->d_dec_offs;
    p.tab.sp_bytes = sp_bytes;
    p.tab.sp_offs = sp_offs;
    p.tab.vocab_size = m->vocab_size;
    p.tab.n_specials = n_specials;
    p.tab.include_special = include_special ? 1 : 0;
    p.src = src;
    p.meta = meta;
    p.starts = starts;
    p.bad_pos = ctrl;
    p.n_replaced = ctrl + 1;
    p.n_specials_live = ctrl + 2;
    p.row_offs = t->d_offs;
    HIP_TRY(tgx::launch_decode_meta(p, scan.ptr, scan.bytes, hs));
    unsigned long long h_bad = ~0ull, h_raw = 0, h_replaced = 0, h_final = 0, h_specials = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, ctrl, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipMemcpyAsync(&h_specials, ctrl + 2, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipMemcpyAsync(&h_raw, starts + N, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    if (h_bad != ~0ull) {
        int64_t x = 0;
        union { int64_t i64; int32_t i32; uint32_t u32; } v = {};
        HIP_TRY(hipMemcpyAsync(&v, static_cast<const char*>(src.ids) + h_bad * decode_elem_bytes(src.kind), decode_elem_bytes(src.kind), hipMemcpyDeviceToHost, hs));
        if (src.offs) {
            h_offs.resize(S + 1);
            HIP_TRY(hipMemcpyAsync(h_offs.data(), src.offs, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, hs));
        }
        HIP_TRY(hipStreamSynchronize(hs));
        x = src.kind == tgx::kDecodeI64 ? v.i64 : src.kind == tgx::kDecodeI32 ? (int64_t)v.i32 : (int64_t)v.u32;
        const uint64_t row = src.offs ? (uint64_t)(std::upper_bound(h_offs.begin(), h_offs.end(), (uint64_t)h_bad) - h_offs.begin()) - 1 : h_bad / src.row_len;
        guard.done();
        return decode_oob(src.kind, x, row, bad_sample, bad_id);
    }
    const uint64_t T = h_raw;
    if (T == 0) {
        HIP_TRY(t->d_bytes.alloc(dev, 0));
        HIP_TRY(hipMemsetAsync(t->d_offs, 0, (size_t)(S + 1) * 8, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        guard.done();
        *out = text.release();
        return TGX_OK;
    }
    const uint64_t G = (T + tgx::kDecodeGroup - 1) / tgx::kDecodeGroup;
    HIP_TRY(raw.alloc(dev, (size_t)G * tgx::kDecodeGroup + 16));
    HIP_TRY(guard.alloc((size_t)G * 4, &flags));
    HIP_TRY(guard.alloc((size_t)(G + 1) * 4, &codes));
    p.n_raw = T;
    p.raw = raw;
    p.flags = flags;
    p.codes = codes;
    if (h_specials) {  // only then can a run end inside a row
        HIP_TRY(guard.alloc((size_t)(N + 1) * 8, &specials));
        p.specials = specials;
        HIP_TRY(tgx::launch_decode_specials(p, scan.ptr, scan.bytes, hs));
    }
    HIP_TRY(tgx::launch_decode_fill(p, hs));
    HIP_TRY(tgx::launch_decode_rows(p, hs));
    HIP_TRY(tgx::launch_decode_utf8(p, hs));
    HIP_TRY(hipMemcpyAsync(&h_replaced, ctrl + 1, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    t->n_replaced = h_replaced;
    if (h_replaced == 0) {  // the raw bytes are the text and the rows' raw starts its offsets
        t->d_bytes = std::move(raw);
        t->n_bytes = T;
        guard.done();
        *out = text.release();
        return TGX_OK;
    }
    HIP_TRY(guard.alloc((size_t)(G + 1) * 8, &gpos));
    if ((st = scan_room(&scan2, guard, tgx::decode_expand_temp_bytes, G)) != TGX_OK) return st;
    p.gpos = gpos;
    HIP_TRY(tgx::launch_decode_positions(p, scan2.ptr, scan2.bytes, hs));
    HIP_TRY(hipMemcpyAsync(&h_final, gpos + G, 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    HIP_TRY(t->d_bytes.alloc(dev, (size_t)h_final + 16));
    p.out = t->d_bytes;
    HIP_TRY(tgx::launch_decode_expand(p, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    t->n_bytes = h_final;
    guard.done();
    *out = text.release();
    return TGX_OK;
}

}  // namespace

tgx_status tgx_decode_result(tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials,
                             int include_special, void* stream, tgx_text** out, uint64_t* bad_sample, uint64_t* bad_id) {
    const char* who = "tgx_decode_result";
    if (!m || !r || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    tgx_status st = decode_check_specials(who, m->vocab_size, special_bytes, special_offs, n_specials);
    if (st != TGX_OK) return st;
    if ((st = require_device()) != TGX_OK) return st;
    if (r->device != m->device) return fail(TGX_ERR_INVALID, "%s: the result is on device %d, the model on device %d", who, r->device, m->device);
    if ((uint64_t)r->vocab_size > (uint64_t)m->vocab_size + n_specials)
        return fail(TGX_ERR_INVALID, "%s: the result was written for %u ids, the model has %u tokens and %u special tokens", who, r->vocab_size,
                    m->vocab_size, n_specials);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t hs = stream_or_default(stream, m->device);
    tgx::DecodeSrc src = {};
    src.ids = r->d_ids.get();
    src.offs = r->d_offs.get();
    src.n_rows = r->n_samples;
    src.n = r->n_tokens;
    src.kind = tgx::kDecodeU32;
    src.skip_id = TGX_NO_ID;
    return decode_device(m, src, special_bytes, special_offs, n_specials, include_special, hs, out, bad_sample, bad_id);
}

tgx_status tgx_decode_padded(tgx_model* m, const void* d_ids, uint64_t n_rows, uint64_t row_len, uint32_t flags, const uint8_t* d_mask,
                             const int32_t* d_lengths, uint32_t skip_id, const uint8_t* special_bytes, const uint64_t* special_offs,
                             uint32_t n_specials, int include_special, void* stream, tgx_text** out, uint64_t* bad_sample, uint64_t* bad_id) {
    const char* who = "tgx_decode_padded";
    if (!m || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    tgx_status st = layout_check_flags(who, flags, TGX_LAYOUT_I64);
    if (st == TGX_OK) st = decode_check_specials(who, m->vocab_size, special_bytes, special_offs, n_specials);
    if (st != TGX_OK) return st;
    if (n_rows && row_len && n_rows > 0xFFFFFFFFFFFFFFFFull / 16 / row_len) return fail(TGX_ERR_UNSUPPORTED, "%s: %llu rows of %llu elements", who, (unsigned long long)n_rows, (unsigned long long)row_len);
    const uint64_t N = n_rows * row_len;
    if (N && !d_ids) return fail(TGX_ERR_INVALID, "%s: d_ids is NULL", who);
    if ((st = require_device()) != TGX_OK) return st;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(m->device));
    if (N) {
        if ((st = check_device_ptr(who, "d_ids", d_ids, m->device, "model")) != TGX_OK) return st;
        if ((st = check_device_ptr(who, "d_mask", d_mask, m->device, "model")) != TGX_OK) return st;
        if ((st = check_device_ptr(who, "d_lengths", d_lengths, m->device, "model")) != TGX_OK) return st;
    }
    hipStream_t hs = stream_or_default(stream, m->device);
    tgx::DecodeSrc src = {};
    src.ids = d_ids;
    src.mask = d_mask;
    src.lengths = d_lengths;
    src.n_rows = n_rows;
    src.row_len = row_len;
    src.n = N;
    src.kind = (flags & TGX_LAYOUT_I64) ? tgx::kDecodeI64 : tgx::kDecodeI32;
    src.skip_id = skip_id;
    return decode_device(m, src, special_bytes, special_offs, n_specials, include_special, hs, out, bad_sample, bad_id);
}

uint64_t tgx_text_num_rows(const tgx_text* t) { return t ? t->n_rows : 0; }
uint64_t tgx_text_num_bytes(const tgx_text* t) { return t ? t->n_bytes : 0; }
uint64_t tgx_text_num_replaced(const tgx_text* t) { return t ? t->n_replaced : 0; }
int tgx_text_device(const tgx_text* t) { return t ? t->device : -1; }
const void* tgx_text_bytes_device(const tgx_text* t) { return t ? t->d_bytes.get() : nullptr; }
const void* tgx_text_offsets_device(const tgx_text* t) { return t ? t->d_offs.get() : nullptr; }
// (the call that made it returned after its stream had reached its end: the buffers go straight back to the pool)
void tgx_text_free(tgx_text* t) { delete t; }

tgx_status tgx_text_copy_bytes(const tgx_text* t, uint8_t* dst, uint64_t cap) {
    if (!t || (!dst && t->n_bytes)) return fail(TGX_ERR_INVALID, "tgx_text_copy_bytes: NULL argument");
    if (cap < t->n_bytes) return fail(TGX_ERR_INVALID, "tgx_text_copy_bytes: %llu bytes, room for %llu", (unsigned long long)t->n_bytes, (unsigned long long)cap);
    if (!t->n_bytes) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(copy_sync(dst, t->d_bytes, t->n_bytes, hipMemcpyDeviceToHost, t->device));
    return TGX_OK;
}

tgx_status tgx_text_copy_offsets(const tgx_text* t, uint64_t* dst, uint64_t cap) {
    if (!t || !dst) return fail(TGX_ERR_INVALID, "tgx_text_copy_offsets: NULL argument");
    if (cap < t->n_rows + 1) return fail(TGX_ERR_INVALID, "tgx_text_copy_offsets: %llu offsets, room for %llu", (unsigned long long)(t->n_rows + 1), (unsigned long long)cap);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(copy_sync(dst, t->d_offs, (t->n_rows + 1) * 8, hipMemcpyDeviceToHost, t->device));
    return TGX_OK;
}

// ---- fill-in-the-middle: a result's rows rearranged behind three sentinels (fim.hip; fim.h has the index arithmetic) ----

namespace {

// device time of the last tgx_result_fim of this thread, per stage (tgx_fim_last_times)
constexpr int kFimStages = 3;
const char* const kFimStageNames[kFimStages] = {"fim_offsets_scan", "fim_fill_kernel", "fim_info_kernel"};
thread_local float g_fim_ms[kFimStages] = {0, 0, 0};

}  // namespace

int tgx_fim_last_times(const char** names, float* ms, int cap) { return stage_times(kFimStageNames, g_fim_ms, kFimStages, names, ms, cap); }

tgx_status tgx_result_from_ids(int device, const uint32_t* ids, const uint64_t* offs, uint64_t n_rows, uint32_t vocab_size, tgx_result** out) {
    const char* who = "tgx_result_from_ids";
    if (!out) return fail(TGX_ERR_INVALID, "%s: out is NULL", who);
    *out = nullptr;
    tgx_status st = result_check_host(who, ids, offs, n_rows, vocab_size);
    if (st != TGX_OK) return st;
    int n_devices = 0;
    if ((st = require_device(&n_devices)) != TGX_OK) return st;
    if (device < 0 || device >= n_devices) return fail(TGX_ERR_INVALID, "%s: device %d of %d", who, device, n_devices);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<tgx_result> r(new tgx_result());
    r->device = device;
    r->vocab_size = vocab_size;
    r->n_samples = n_rows;
    r->n_tokens = offs[n_rows];
    if (r->d_offs.alloc(device, (size_t)(n_rows + 1) * 8) != hipSuccess || r->d_ids.alloc(device, (size_t)r->n_tokens * 4 + 256) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (result from ids)");
    HIP_TRY(copy_sync(r->d_offs, offs, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, device));
    if (r->n_tokens) HIP_TRY(copy_sync(r->d_ids, ids, (size_t)r->n_tokens * 4, hipMemcpyHostToDevice, device));
    *out = r.release();
    return TGX_OK;
}

tgx_status tgx_result_fim(const tgx_result* r, uint32_t prefix_id, uint32_t suffix_id, uint32_t middle_id, double rate, double spm_rate,
                          uint64_t seed, uint64_t first_row, void* stream, uint8_t* mode, uint64_t* cuts, uint64_t* n_applied, tgx_result** out) {
    const char* who = "tgx_result_fim";
    if (!r || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    tgx_status st = fim_check(who, prefix_id, suffix_id, middle_id, rate, spm_rate);
    if (st != TGX_OK) return st;
    const uint64_t S = r->n_samples;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    hipStream_t hs = stream_or_default(stream, r->device);
    std::unique_ptr<tgx_result> res(new tgx_result());  // before the guard: its buffers go back after the stream's end
    uint64_t h_total = 0;
    StageTimer<kFimStages> timer(hs, g_fim_ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(r->device, hs);
    res->device = r->device;
    res->vocab_size = fim_vocab_size(r->vocab_size, prefix_id, suffix_id, middle_id);
    res->n_samples = S;
    ScanScratch scan;
    if (res->d_offs.alloc(r->device, (size_t)(S + 1) * 8) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (fill-in-the-middle)");
    if ((st = scan_room(&scan, guard, tgx::fim_scan_temp_bytes, S, "out of device memory (fill-in-the-middle)")) != TGX_OK) return st;
    tgx::FimParams p = {};
    p.ids = r->d_ids;
    p.offs = r->d_offs;
    p.n_rows = S;
    p.f = tgx::FimArgs{seed, first_row, rate, spm_rate, prefix_id, suffix_id, middle_id};
    p.out_offs = res->d_offs;
    timer.begin(0);
    if (tgx::launch_fim_offsets(p, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan launch failed");
    timer.end(0);
    // the one word that visits the host: T' sizes the id buffer
    if ((st = read_u64(hs, res->d_offs.get() + S, &h_total)) != TGX_OK) return st;
    if (h_total < r->n_tokens || (h_total - r->n_tokens) % 3 || (h_total - r->n_tokens) / 3 > S)
        return fail(TGX_ERR_DEVICE, "%s: %llu ids from %llu over %llu rows", who, (unsigned long long)h_total, (unsigned long long)r->n_tokens,
                    (unsigned long long)S);
    res->n_tokens = h_total;
    if (res->d_ids.alloc(r->device, (size_t)h_total * 4 + 256) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (fill-in-the-middle)");
    p.n_out = h_total;
    p.out_ids = res->d_ids;
    timer.begin(1);
    if (tgx::launch_fim_fill(p, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "fim_fill_kernel launch failed");
    timer.end(1);
    if (S && (mode || cuts)) {
        uint8_t* d_mode = nullptr;
        uint64_t* d_cuts = nullptr;
        if (mode) HIP_TRY(guard.alloc((size_t)S, &d_mode));
        if (cuts) HIP_TRY(guard.alloc((size_t)S * 16, &d_cuts));
        timer.begin(2);
        if (tgx::launch_fim_info(p, d_mode, d_cuts, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "fim_info_kernel launch failed");
        timer.end(2);
        if (mode) HIP_TRY(hipMemcpyAsync(mode, d_mode, (size_t)S, hipMemcpyDeviceToHost, hs));
        if (cuts) HIP_TRY(hipMemcpyAsync(cuts, d_cuts, (size_t)S * 16, hipMemcpyDeviceToHost, hs));
    }
    // the stream has reached its end before either result can change hands (the guard: also after a failure)
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    if (n_applied) *n_applied = (h_total - r->n_tokens) / 3;
    *out = res.release();
    return TGX_OK;
}

// ---- row selection: rows of a result through an index, the rows' lengths, the seeded permutation (select.hip; select.h) ----

namespace {

const char* const kSelectStageNames[kSelectStages] = {"select_check", "select_offsets_scan", "select_fill_kernel"};
thread_local float g_select_ms[kSelectStages] = {0, 0, 0};

}  // namespace

namespace tgx::dev {

float* select_stage_ms() { return g_select_ms; }

tgx_status select_rows_device(const char* who, const int64_t* rows, uint64_t n_select, uint32_t flags, int device, StreamGuard& guard,
                              const int64_t** d_rows) {
    *d_rows = nullptr;
    if (n_select == 0) return TGX_OK;
    if (flags & TGX_SELECT_ROWS_DEVICE) {
        *d_rows = rows;
        return check_device_ptr(who, "rows", rows, device, "source");
    }
    uint64_t* up = nullptr;
    HIP_TRY(guard.alloc((size_t)n_select * 8, &up));
    HIP_TRY(guard.upload(up, std::vector<uint64_t>(reinterpret_cast<const uint64_t*>(rows), reinterpret_cast<const uint64_t*>(rows) + n_select)));
    *d_rows = reinterpret_cast<const int64_t*>(up);
    return TGX_OK;
}

tgx_status select_bad_index(const char* who, uint64_t bad_k, const int64_t* d_rows, uint64_t n_src, hipStream_t hs) {
    if (bad_k == tgx::kSelectNoBad) return TGX_OK;
    int64_t value = 0;
    const tgx_status st = read_u64(hs, d_rows + bad_k, &value);
    if (st != TGX_OK) return st;
    return select_index_error(who, bad_k, value, n_src);
}

}  // namespace tgx::dev

int tgx_select_last_times(const char** names, float* ms, int cap) { return stage_times(kSelectStageNames, g_select_ms, kSelectStages, names, ms, cap); }

tgx_status tgx_result_select(const tgx_result* r, const int64_t* rows, uint64_t n_select, uint32_t flags, void* stream, tgx_result** out) {
    const char* who = "tgx_result_select";
    if (!r || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (n_select && !rows) return fail(TGX_ERR_INVALID, "%s: rows is NULL", who);
    tgx_status st = layout_check_flags(who, flags, TGX_SELECT_ROWS_DEVICE);
    if (st != TGX_OK) return st;
    const bool on_device = (flags & TGX_SELECT_ROWS_DEVICE) != 0;
    if (!on_device && (st = select_check_rows(who, rows, n_select, r->n_samples)) != TGX_OK) return st;  // before any device call
    const uint64_t S = r->n_samples, M = n_select;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    hipStream_t hs = stream_or_default(stream, r->device);
    std::unique_ptr<tgx_result> res(new tgx_result());  // before the guard: its buffers go back after the stream's end
    unsigned long long h_words[2] = {0, tgx::kSelectNoBad};  // T' and the bad-index word
    StageTimer<kSelectStages> timer(hs, g_select_ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(r->device, hs);
    res->device = r->device;
    res->vocab_size = r->vocab_size;
    res->n_samples = M;
    tgx::SelectParams p = {};
    if ((st = select_rows_device(who, rows, M, flags, r->device, guard, &p.rows)) != TGX_OK) return st;
    ScanScratch scan;
    unsigned long long* d_bad = nullptr;
    if (res->d_offs.alloc(r->device, (size_t)(M + 1) * 8) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (select)");
    if ((st = scan_room(&scan, guard, tgx::select_scan_temp_bytes, M, "out of device memory (select)")) != TGX_OK) return st;
    if (guard.alloc(sizeof(unsigned long long), &d_bad) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (select)");
    p.data = r->d_ids;
    p.offs = r->d_offs;
    p.n_src = S;
    p.n_rows = M;
    p.out_offs = res->d_offs;
    if (on_device && M) {
        HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), hs));
        timer.begin(0);
        if (tgx::launch_select_check(p, d_bad, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "select_check_kernel launch failed");
        timer.end(0);
        HIP_TRY(hipMemcpyAsync(&h_words[1], d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, hs));
    }
    timer.begin(1);
    if (tgx::launch_select_offsets(p, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan launch failed");
    timer.end(1);
    // the one host visit: T' sizes the id buffer, and the bad-index word comes with it
    if ((st = read_u64(hs, res->d_offs.get() + M, &h_words[0])) != TGX_OK) return st;
    if ((st = select_bad_index(who, h_words[1], p.rows, S, hs)) != TGX_OK) {
        guard.done();  // (the stream has reached its end)
        return st;
    }
    const uint64_t h_total = h_words[0];
    res->n_tokens = h_total;
    if (res->d_ids.alloc(r->device, (size_t)h_total * 4 + 256) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (select)");
    p.n_out = h_total;
    p.out = res->d_ids;
    timer.begin(2);
    if (tgx::launch_select_fill_ids(p, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "select_fill_kernel launch failed");
    timer.end(2);
    // the stream has reached its end before either result can change hands (the guard: also after a failure)
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    *out = res.release();
    return TGX_OK;
}

tgx_status tgx_result_lengths_device(const tgx_result* r, void* stream, int64_t* d_lengths) {
    const char* who = "tgx_result_lengths_device";
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if (r->n_samples == 0) return TGX_OK;
    if (!d_lengths) return fail(TGX_ERR_INVALID, "%s: d_lengths is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(r->device));
    const tgx_status st = check_device_ptr(who, "d_lengths", d_lengths, r->device, "result");
    if (st != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, r->device);
    StreamGuard guard(r->device, hs);
    HIP_TRY(tgx::launch_select_lengths(r->d_offs, r->n_samples, d_lengths, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

tgx_status tgx_shuffled_rows_device(int device, uint64_t n, uint64_t seed, void* stream, int64_t* d_rows) {
    const char* who = "tgx_shuffled_rows_device";
    if (n >= 0x80000000ull) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^31 rows or more", who);
    int n_devices = 0;
    tgx_status st = require_device(&n_devices);
    if (st != TGX_OK) return st;
    if (device < 0 || device >= n_devices) return fail(TGX_ERR_INVALID, "%s: device %d of %d", who, device, n_devices);
    if (n == 0) return TGX_OK;
    if (!d_rows) return fail(TGX_ERR_INVALID, "%s: d_rows is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_rows", d_rows, device, "call")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    StreamGuard guard(device, hs);
    size_t sort_bytes = 0;
    if (tgx::shuffle_sort_temp_bytes(n, &sort_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "sort temp-size query failed");
    uint64_t *keys_in = nullptr, *keys_out = nullptr;
    int64_t* vals_in = nullptr;
    void* d_sort = nullptr;
    HIP_TRY(guard.alloc((size_t)n * 8, &keys_in));
    HIP_TRY(guard.alloc((size_t)n * 8, &keys_out));
    HIP_TRY(guard.alloc((size_t)n * 8, &vals_in));
    HIP_TRY(guard.alloc(sort_bytes + 8, &d_sort));  // (never NULL: that asks the sort for its size)
    HIP_TRY(tgx::launch_shuffled_rows(n, seed, keys_in, keys_out, vals_in, d_rows, d_sort, sort_bytes, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

// ---- exact row deduplication: the first row with the same content (dedup.hip; dedup.h has the hash and the rules) ----

namespace {

const char* const kDedupStageNames[tgx::kDedupStages] = {"dedup_hash_kernel", "dedup_sort", "dedup_compare_kernel", "dedup_resolve"};
thread_local float g_dedup_ms[tgx::kDedupStages] = {0, 0, 0, 0};
thread_local uint32_t g_dedup_rounds = 0;

// bits of the hash that make the sort key: 64, or the test knob's (a small number makes rows collide)
uint32_t dedup_hash_bits() {
    int bits = 64;
    knob_int("TGX_DEDUP_HASH_BITS", 0, 64, &bits);
    return (uint32_t)bits;
}

// what the calls on rows share before anything is queued: the limit on S, the destination
tgx_status dedup_check_dest(const char* who, const char* what, const tgx::DedupRows& rows, const void* dest, int device) {
    if (rows.n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (!dest) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, what);
    return check_device_ptr(who, what, dest, device, "source");
}

}  // namespace

namespace tgx::dev {

// The rounds.  The scratch is the guard's, allocated once and used by every round; a round ends in the one host visit
// that reads how many rows are left (and the heads so far), after which the stages' times of that round are added up.
tgx_status dedup_first_equal(const char* who, const tgx::DedupRows& rows, int device, void* stream, int64_t* d_first, uint64_t* n_unique) {
    const uint64_t S = rows.n_rows;
    if (n_unique) *n_unique = 0;
    if (S == 0) {
        g_dedup_rounds = 0;
        std::fill(g_dedup_ms, g_dedup_ms + tgx::kDedupStages, 0.f);
        return TGX_OK;
    }
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    tgx_status st = dedup_check_dest(who, "d_first", rows, d_first, device);
    if (st != TGX_OK) return st;
    const uint32_t bits = dedup_hash_bits();
    hipStream_t hs = stream_or_default(stream, device);
    unsigned long long h_words[2] = {0, 0};  // rows left, heads so far (before the guard: a copy writes them)
    float round_ms[tgx::kDedupStages] = {0, 0, 0, 0}, total_ms[tgx::kDedupStages] = {0, 0, 0, 0};
    StageTimer<tgx::kDedupStages> timer(hs, round_ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    tgx::DedupScratch s = {};
    if (tgx::dedup_temp_bytes(S, &s.scan_bytes, &s.sort_bytes, &s.select_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    const bool got = guard.alloc((size_t)S * 8, &s.keys_a) == hipSuccess && guard.alloc((size_t)S * 8, &s.keys_b) == hipSuccess &&
                     guard.alloc((size_t)S * 4, &s.rows_a) == hipSuccess && guard.alloc((size_t)S * 4, &s.rows_b) == hipSuccess &&
                     guard.alloc((size_t)(S + 1) * 8, &s.offs_tmp) == hipSuccess && guard.alloc((size_t)S * 4, &s.head_row) == hipSuccess &&
                     guard.alloc((size_t)S, &s.flag) == hipSuccess && guard.alloc((size_t)S, &s.mark) == hipSuccess &&
                     guard.alloc((size_t)S * 4, &s.list[0]) == hipSuccess && guard.alloc((size_t)S * 4, &s.list[1]) == hipSuccess &&
                     guard.alloc(2 * sizeof(unsigned long long), &s.words) == hipSuccess &&
                     guard.alloc(s.scan_bytes + 8, &s.scan_tmp) == hipSuccess &&  // (never NULL: that asks for the size)
                     guard.alloc(s.sort_bytes + 8, &s.sort_tmp) == hipSuccess && guard.alloc(s.select_bytes + 8, &s.select_tmp) == hipSuccess;
    if (!got) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (dedup)");
    }
    HIP_TRY(hipMemsetAsync(s.words, 0, 2 * sizeof(unsigned long long), hs));
    const uint32_t* list = nullptr;  // round 0: every row
    uint64_t n_list = S;
    uint32_t round = 0;
    while (n_list) {
        uint32_t* next = s.list[round & 1];
        timer.begin(0);
        if (tgx::launch_dedup_hash(rows, list, n_list, round, bits, s.offs_tmp, s.scan_tmp, s.scan_bytes, s.keys_a, s.keys_a, s.rows_a, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "dedup_hash_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_dedup_sort(s, n_list, bits, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dedup sort launch failed");
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_dedup_compare(rows, s, n_list, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dedup_compare_kernel launch failed");
        timer.end(2);
        timer.begin(3);
        if (tgx::launch_dedup_resolve(s, list, n_list, next, d_first, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dedup resolve launch failed");
        timer.end(3);
        if ((st = read_u64(hs, s.words, h_words, 2)) != TGX_OK) return st;  // the round's host visit
        timer.read();
        for (int k = 0; k < tgx::kDedupStages; k++) total_ms[k] += round_ms[k];
        round++;
        if (h_words[0] >= n_list) {  // (every round resolves its heads)
            guard.done();
            return fail(TGX_ERR_DEVICE, "%s: round %u resolved no row", who, round);
        }
        n_list = h_words[0];
        list = next;
    }
    guard.done();  // (the stream has reached its end)
    std::copy(total_ms, total_ms + tgx::kDedupStages, g_dedup_ms);
    g_dedup_rounds = round;
    if (n_unique) *n_unique = h_words[1];
    return TGX_OK;
}

tgx_status dedup_row_hashes(const char* who, const tgx::DedupRows& rows, int device, uint64_t seed, void* stream, uint64_t* d_hashes) {
    const uint64_t S = rows.n_rows;
    if (S == 0) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    tgx_status st = dedup_check_dest(who, "d_hashes", rows, d_hashes, device);
    if (st != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    StreamGuard guard(device, hs);
    size_t scan_bytes = 0, sort_bytes = 0, select_bytes = 0;
    if (tgx::dedup_temp_bytes(S, &scan_bytes, &sort_bytes, &select_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    uint64_t *pad_offs = nullptr, *sums = nullptr;
    void* scan_tmp = nullptr;
    if (guard.alloc((size_t)(S + 1) * 8, &pad_offs) != hipSuccess || guard.alloc((size_t)S * 8, &sums) != hipSuccess ||
        guard.alloc(scan_bytes + 8, &scan_tmp) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (dedup)");
    }
    if (tgx::launch_dedup_hash(rows, nullptr, S, seed, 64, pad_offs, scan_tmp, scan_bytes, sums, d_hashes, nullptr, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "dedup_hash_kernel launch failed");
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

}  // namespace tgx::dev

int tgx_dedup_last_times(const char** names, float* ms, int cap) { return stage_times(kDedupStageNames, g_dedup_ms, tgx::kDedupStages, names, ms, cap); }
uint32_t tgx_dedup_last_rounds(void) { return g_dedup_rounds; }

namespace {
tgx::DedupRows dedup_rows_of(const tgx_result* r) { return tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}; }
}  // namespace

tgx_status tgx_result_first_equal_device(const tgx_result* r, uint32_t flags, void* stream, int64_t* d_first, uint64_t* n_unique) {
    const char* who = "tgx_result_first_equal_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return dedup_first_equal(who, dedup_rows_of(r), r->device, stream, d_first, n_unique);
}

tgx_status tgx_result_row_hashes_device(const tgx_result* r, uint64_t seed, void* stream, uint64_t* d_hashes) {
    const char* who = "tgx_result_row_hashes_device";
    const tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    return dedup_row_hashes(who, dedup_rows_of(r), r->device, seed, stream, d_hashes);
}

// ---- spans: the part of its row's text that every token covers (spans.hip; spans.h has the index arithmetic) ------

namespace {

// the model's token words on its device, once (under m->mu)
tgx_status ensure_span_words(tgx_model* m) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->span_words_ready) return TGX_OK;
    const uint32_t V = m->vocab_size;
    std::vector<uint16_t> words;
    const tgx_status st = span_build_words("spans", m->vocab_bytes.data(), m->vocab_offs.data(), V, &words);
    if (st != TGX_OK) return st;
    if (!m->d_span_words) HIP_TRY(hipMalloc((void**)&m->d_span_words, ((size_t)V + 8) * 2));
    if (V) HIP_TRY(hipMemcpy(m->d_span_words, words.data(), (size_t)V * 2, hipMemcpyHostToDevice));
    m->span_words_ready = true;
    return TGX_OK;
}

// The first half of a spans call over a result with T >= 1 tokens: the model's words, the specials' words, the value
// words and their prefix sums in pooled scratch of the guard, and for int32 spans the check of the rows' totals (one
// word is read back; nothing has been written to the destination when a row does not fit).  Fills p's tables, source
// and scratch; p->flags is set by the caller.
tgx_status span_sums_device(const char* who, tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs,
                            uint32_t n_specials, hipStream_t hs, StreamGuard& guard, tgx::SpanParams* p) {
    const bool chars = (p->flags & TGX_SPAN_CHARS) != 0, i64 = (p->flags & TGX_LAYOUT_I64) != 0;
    const uint64_t T = r->n_tokens;
    const tgx_status st = ensure_span_words(m);
    if (st != TGX_OK) return st;
    std::vector<uint64_t> sp_words;
    span_special_words(special_bytes, special_offs, n_specials, chars, &sp_words);
    uint32_t* vals = nullptr;
    uint64_t *sums = nullptr, *d_sp_words = nullptr;
    ScanScratch scan;
    HIP_TRY(guard.alloc((size_t)(T + 1) * 4, &vals));
    HIP_TRY(guard.alloc((size_t)(T + 1) * 8, &sums));
    const tgx_status scan_st = scan_room(&scan, guard, tgx::span_scan_temp_bytes, T);
    if (scan_st != TGX_OK) return scan_st;
    HIP_TRY(guard.alloc(sp_words.size() * 8, &d_sp_words));
    HIP_TRY(guard.upload(d_sp_words, std::move(sp_words)));
    p->tab.words = m->d_span_words;
    p->tab.sp_words = d_sp_words;
    p->tab.vocab_size = m->vocab_size;
    p->tab.n_specials = n_specials;
    p->ids = r->d_ids;
    p->offs = r->d_offs;
    p->n_rows = r->n_samples;
    p->n = T;
    p->vals = vals;
    p->sums = sums;
    HIP_TRY(tgx::launch_span_sums(*p, scan.ptr, scan.bytes, hs));
    if (!i64) {  // nothing is written when a row does not fit: the one word that is read back
        unsigned long long h_max = 0, *row_max = nullptr;
        HIP_TRY(guard.alloc(sizeof(unsigned long long), &row_max));
        p->row_max = row_max;
        HIP_TRY(hipMemsetAsync(row_max, 0, sizeof(unsigned long long), hs));
        HIP_TRY(tgx::launch_span_row_max(*p, hs));
        HIP_TRY(hipMemcpyAsync(&h_max, row_max, sizeof(unsigned long long), hipMemcpyDeviceToHost, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        if (h_max >= 0x80000000ull) return span_too_long(who, h_max, chars);
    }
    return TGX_OK;
}

// row_len = 0: the flat form
tgx_status spans_device(const char* who, tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs,
                        uint32_t n_specials, uint32_t row_len, uint32_t bos_id, uint32_t eos_id, uint32_t flags, void* stream, void* d_spans) {
    if (!m || !r) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    const bool padded = row_len != 0;
    const tgx_status st0 = span_check_args(who, m->vocab_size, special_bytes, special_offs, n_specials, padded, row_len, bos_id, eos_id, flags);
    if (st0 != TGX_OK) return st0;
    const uint64_t S = r->n_samples, T = r->n_tokens;
    const uint64_t n_pairs = padded ? S * (uint64_t)row_len : (S ? T : 0);
    if (!d_spans && n_pairs) return fail(TGX_ERR_INVALID, "%s: d_spans is NULL", who);
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (r->device != m->device) return fail(TGX_ERR_INVALID, "%s: the result is on device %d, the model on device %d", who, r->device, m->device);
    if ((uint64_t)r->vocab_size > (uint64_t)m->vocab_size + n_specials)
        return fail(TGX_ERR_INVALID, "%s: the result was written for %u ids, the model has %u tokens and %u special tokens", who, r->vocab_size,
                    m->vocab_size, n_specials);
    if (n_pairs == 0) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(m->device));
    if ((st = check_device_ptr(who, "d_spans", d_spans, m->device, "result")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, m->device);
    const int dev = m->device;
    const bool i64 = (flags & TGX_LAYOUT_I64) != 0;
    if (T == 0) {  // the padded form of rows without tokens
        StreamGuard guard(dev, hs);
        HIP_TRY(hipMemsetAsync(d_spans, 0, (size_t)n_pairs * 2 * (i64 ? 8 : 4), hs));
        HIP_TRY(hipStreamSynchronize(hs));
        guard.done();
        return TGX_OK;
    }
    StreamGuard guard(dev, hs);
    tgx::SpanParams p = {};
    p.len = row_len;
    p.bos = bos_id;
    p.eos = eos_id;
    p.flags = flags;
    p.out = d_spans;
    if ((st = span_sums_device(who, m, r, special_bytes, special_offs, n_specials, hs, guard, &p)) != TGX_OK) return st;
    HIP_TRY(padded ? tgx::launch_span_pad(p, hs) : tgx::launch_span_flat(p, hs));
    // the stream has reached its end before the result or the destination can change hands
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}

}  // namespace

tgx_status tgx_result_spans_device(tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs,
                                   uint32_t n_specials, uint32_t flags, void* stream, void* d_spans) {
    return spans_device("tgx_result_spans_device", m, r, special_bytes, special_offs, n_specials, 0, TGX_NO_ID, TGX_NO_ID, flags, stream, d_spans);
}

tgx_status tgx_result_pad_spans_device(tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs,
                                       uint32_t n_specials, uint32_t row_len, uint32_t bos_id, uint32_t eos_id, uint32_t flags, void* stream,
                                       void* d_spans) {
    const char* who = "tgx_result_pad_spans_device";
    if (row_len == 0) return fail(TGX_ERR_INVALID, "%s: row_len 0 (needs >= 1)", who);
    return spans_device(who, m, r, special_bytes, special_offs, n_specials, row_len, bos_id, eos_id, flags, stream, d_spans);
}

tgx_status tgx_result_window_spans_device(tgx_model* m, const tgx_result* r, const uint8_t* special_bytes, const uint64_t* special_offs,
                                          uint32_t n_specials, uint32_t row_len, uint32_t stride, uint32_t bos_id, uint32_t eos_id, uint32_t flags,
                                          void* stream, uint64_t n_windows, void* d_spans) {
    const char* who = "tgx_result_window_spans_device";
    if (!m || !r) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    if (row_len == 0) return fail(TGX_ERR_INVALID, "%s: row_len 0 (needs >= 1)", who);
    tgx_status st = span_check_args(who, m->vocab_size, special_bytes, special_offs, n_specials, true, row_len, bos_id, eos_id, flags);
    const tgx::LayoutSeq seq = tgx::layout_seq(bos_id, eos_id, 0);
    if (st == TGX_OK) st = window_check_args(who, row_len, stride, seq.extra);
    if (st != TGX_OK) return st;
    const uint64_t S = r->n_samples, T = r->n_tokens;
    if (!d_spans && S) return fail(TGX_ERR_INVALID, "%s: d_spans is NULL", who);
    if ((st = require_device()) != TGX_OK) return st;
    if (r->device != m->device) return fail(TGX_ERR_INVALID, "%s: the result is on device %d, the model on device %d", who, r->device, m->device);
    if ((uint64_t)r->vocab_size > (uint64_t)m->vocab_size + n_specials)
        return fail(TGX_ERR_INVALID, "%s: the result was written for %u ids, the model has %u tokens and %u special tokens", who, r->vocab_size,
                    m->vocab_size, n_specials);
    if (S == 0) return window_check_totals(who, 0, 0, &n_windows);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(m->device));
    if ((st = check_device_ptr(who, "d_spans", d_spans, m->device, "result")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, m->device);
    StreamGuard guard(m->device, hs);
    const uint64_t* d_wo = nullptr;
    uint64_t W = 0;
    st = window_offsets_device(who, r, row_len - seq.extra, row_len - seq.extra - stride, hs, guard, &d_wo, &W);
    if (st == TGX_OK) st = window_check_totals(who, 0, W, &n_windows);
    if (st != TGX_OK) return st;
    if (T == 0) {  // rows without tokens: W = S windows of padding
        HIP_TRY(hipMemsetAsync(d_spans, 0, (size_t)W * row_len * 2 * ((flags & TGX_LAYOUT_I64) ? 8 : 4), hs));
    } else {
        tgx::SpanParams p = {};
        p.len = row_len;
        p.bos = bos_id;
        p.eos = eos_id;
        p.flags = flags;
        p.out = d_spans;
        if ((st = span_sums_device(who, m, r, special_bytes, special_offs, n_specials, hs, guard, &p)) != TGX_OK) return st;
        HIP_TRY(tgx::launch_span_windows(p, d_wo, stride, W, hs));
    }
    // the stream has reached its end before the result or the destination can change hands
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    return TGX_OK;
}
