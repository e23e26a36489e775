// The C ABI's hashed n-gram features (include/tgx_hashed.h: tgx_result_hashed_counts_device,
// tgx_corpus_hashed_counts_device, tgx_result_hashed_scores_device, tgx_corpus_hashed_scores_device, tgx_hashed_info,
// tgx_hashed_last_times): the argument checks, the scratch for the transposed weights and the stages' times around the
// launchers of hashed.hip.  The calls run on the caller's stream under a StreamGuard, as the shared n-gram calls of
// gram_ops.cpp do, and share device_internal.h with them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "../../include/tgx_hashed.h"
#include "api_internal.h"
#include "device_internal.h"
#include "hashed.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_HASHED_MAX_WIDTHS == tgx::kHashedMaxWidths && TGX_HASHED_MAX_VECTORS == tgx::kHashedMaxVectors &&
                  TGX_HASHED_MAX_ENTRIES == tgx::kHashedMaxEntries,
              "include/tgx_hashed.h and hashed.h name the same limits");

namespace {

const char* const kHashedStageNames[tgx::kHashedStages] = {"hashed_counts_kernel", "hashed_scores_kernel"};
thread_local float g_hashed_ms[tgx::kHashedStages] = {0, 0};

// Counts (d_q == NULL and n_vectors == 1) or scores of the rows of a result or of a corpus.  The handle, the flags and a
// device have been checked.
tgx_status hashed_call(const char* who, const tgx::DedupRows& rows, int device, bool scores, const uint32_t* widths, uint32_t n_widths, uint64_t buckets,
                       uint32_t n_vectors, uint64_t seed, const int32_t* d_q, void* stream, int64_t* d_out) {
    tgx::HashedWidths ws;
    tgx_status st = tgx::hashed_check(who, widths, n_widths, rows.elem_bytes, buckets, n_vectors, &ws);
    if (st != TGX_OK) return st;
    const char* out_name = scores ? "d_scores" : "d_counts";
    if (!d_out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, out_name);
    if (scores && !d_q) return fail(TGX_ERR_INVALID, "%s: d_q is NULL", who);
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    const int stage = scores ? 1 : 0;
    if (S == 0) {
        g_hashed_ms[stage] = 0;
        return TGX_OK;
    }
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, out_name, d_out, device, "source")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_q", d_q, device, "source")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[1] = {0};
    StageTimer<1> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    int32_t* d_table = nullptr;  // the weights as [B][KP]: every entry is written by hashed_table_kernel, whatever the pool held
    if (scores && rows.n_elems && guard.alloc((size_t)buckets * tgx::hashed_padded(n_vectors) * 4, &d_table) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (hashed features)");
    }
    timer.begin(0);
    if (scores ? tgx::launch_hashed_scores(rows, ws, buckets, n_vectors, seed, d_q, d_table, d_out, hs) != hipSuccess
               : tgx::launch_hashed_counts(rows, ws, buckets, seed, d_out, nullptr, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "%s launch failed", kHashedStageNames[stage]);
    timer.end(0);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    g_hashed_ms[stage] = ms[0];
    return TGX_OK;
}

tgx_status hashed_result(const char* who, const tgx_result* r, bool scores, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors,
                         uint64_t seed, const int32_t* d_q, uint32_t flags, void* stream, int64_t* d_out) {
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return hashed_call(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, scores, widths, n_widths, buckets,
                       n_vectors, seed, d_q, stream, d_out);
}

tgx_status hashed_corpus(const char* who, tgx_corpus* c, bool scores, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors,
                         uint64_t seed, const int32_t* d_q, uint32_t flags, void* stream, int64_t* d_out) {
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return hashed_call(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, scores, widths, n_widths, buckets, n_vectors,
                       seed, d_q, stream, d_out);
}

}  // namespace

int tgx_hashed_last_times(const char** names, float* ms, int cap) { return stage_times(kHashedStageNames, g_hashed_ms, tgx::kHashedStages, names, ms, cap); }

tgx_status tgx_result_hashed_counts_device(const tgx_result* r, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint64_t seed, uint32_t flags,
                                           void* stream, int64_t* d_counts) {
    return hashed_result("tgx_result_hashed_counts_device", r, false, widths, n_widths, buckets, 1, seed, nullptr, flags, stream, d_counts);
}

tgx_status tgx_corpus_hashed_counts_device(tgx_corpus* c, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint64_t seed, uint32_t flags,
                                           void* stream, int64_t* d_counts) {
    return hashed_corpus("tgx_corpus_hashed_counts_device", c, false, widths, n_widths, buckets, 1, seed, nullptr, flags, stream, d_counts);
}

tgx_status tgx_result_hashed_scores_device(const tgx_result* r, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors,
                                           uint64_t seed, const int32_t* d_q, uint32_t flags, void* stream, int64_t* d_scores) {
    return hashed_result("tgx_result_hashed_scores_device", r, true, widths, n_widths, buckets, n_vectors, seed, d_q, flags, stream, d_scores);
}

tgx_status tgx_corpus_hashed_scores_device(tgx_corpus* c, const uint32_t* widths, uint32_t n_widths, uint64_t buckets, uint32_t n_vectors, uint64_t seed,
                                           const int32_t* d_q, uint32_t flags, void* stream, int64_t* d_scores) {
    return hashed_corpus("tgx_corpus_hashed_scores_device", c, true, widths, n_widths, buckets, n_vectors, seed, d_q, flags, stream, d_scores);
}
