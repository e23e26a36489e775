// The C ABI's repetition statistics of a result or a resident corpus (include/tgx.h: tgx_result_repeat_stats_device,
// tgx_corpus_repeat_stats_device, tgx_repeat_last_times): the argument checks, the scratch and the stages' times around
// the launchers of repeat.hip.  They run on the caller's stream under a StreamGuard, as the gram calls of gram_ops.cpp
// do, and share device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "repeat.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_REPEAT_N == tgx::kRepeatN && TGX_REPEAT_MASK_REPEAT == tgx::kRepeatBitRepeat && TGX_REPEAT_MASK_MULTI == tgx::kRepeatBitMulti,
              "include/tgx.h and repeat.h name the same table and mask bits");

namespace {

const char* const kRepeatStageNames[tgx::kRepeatStages] = {"repeat_keys_kernel", "repeat_sort", "repeat_runs_kernel", "repeat_cover_kernel"};
thread_local float g_repeat_ms[tgx::kRepeatStages] = {0, 0, 0, 0};

// table and mask of the rows of a result or of a corpus.  The handle, the flags and a device have been checked.
tgx_status repeat_stats(const char* who, const tgx::DedupRows& rows, int device, uint32_t width, uint64_t seed, void* stream, int64_t* d_stats,
                        uint8_t* d_mask) {
    if (rows.elem_bytes != 1 && rows.elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, rows.elem_bytes);
    if (width == 0 || (uint64_t)width * rows.elem_bytes > tgx::kMinhashMaxBytes)
        return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, width, rows.elem_bytes,
                    tgx::kMinhashMaxBytes / rows.elem_bytes);
    if (!d_stats && !d_mask) return fail(TGX_ERR_INVALID, "%s: d_stats and d_mask are both NULL", who);
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (N > tgx::kRepeatMaxElems) return fail(TGX_ERR_UNSUPPORTED, "%s: 2^32-1 elements or more", who);
    if (S == 0) {
        std::fill(g_repeat_ms, g_repeat_ms + tgx::kRepeatStages, 0.0f);
        return TGX_OK;
    }
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    tgx_status st;
    if ((st = check_device_ptr(who, "d_stats", d_stats, device, "source")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_mask", d_mask, device, "source")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    unsigned long long h_word = 0;  // (before the guard: a queued copy writes it)
    float ms[tgx::kRepeatStages] = {0, 0, 0, 0};
    StageTimer<tgx::kRepeatStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    const char* oom = "out of device memory (repetition statistics)";
    size_t scan_bytes = 0;
    if (tgx::gram_scan_bytes(S, &scan_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    uint64_t* g_offs = nullptr;
    void* scan_tmp = nullptr;
    uint8_t* flag = d_mask;  // the caller's mask is the flag array itself
    if (guard.alloc((size_t)(S + 1) * 8, &g_offs) != hipSuccess || guard.alloc(scan_bytes + 8, &scan_tmp) != hipSuccess ||
        (!flag && N && guard.alloc((size_t)N, &flag) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, oom);
    }
    timer.begin(0);
    if (tgx::launch_gram_offsets(rows, width, g_offs, scan_tmp, scan_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
    if (tgx::launch_repeat_preset(rows, width, d_stats, flag, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    // the grams' total sizes the sort: a host visit
    if ((st = read_u64(hs, g_offs + S, &h_word)) != TGX_OK) return st;
    const uint64_t G = h_word;
    if (G) {
        size_t sort_bytes = 0;
        if (tgx::repeat_sort_bytes(G, &sort_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
        uint64_t *keys_a = nullptr, *keys_b = nullptr;
        uint32_t *pos_a = nullptr, *pos_b = nullptr;
        void* sort_tmp = nullptr;
        if (guard.alloc((size_t)G * 8, &keys_a) != hipSuccess || guard.alloc((size_t)G * 8, &keys_b) != hipSuccess ||
            guard.alloc((size_t)G * 4, &pos_a) != hipSuccess || guard.alloc((size_t)G * 4, &pos_b) != hipSuccess ||
            guard.alloc(sort_bytes + 8, &sort_tmp) != hipSuccess) {  // (never NULL: that asks for the size)
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, oom);
        }
        if (tgx::launch_repeat_keys(rows, width, seed, g_offs, keys_a, pos_a, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "repeat_keys_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_repeat_sort(keys_a, keys_b, pos_a, pos_b, G, sort_tmp, sort_bytes, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "%s: sort launch failed", who);
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_repeat_runs(rows, keys_b, pos_b, G, flag, d_stats, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "repeat_runs_kernel launch failed");
        timer.end(2);
        if (d_stats) {
            timer.begin(3);
            if (tgx::launch_repeat_cover(rows, width, flag, d_stats, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "repeat_cover_kernel launch failed");
            timer.end(3);
        }
    } else {
        timer.end(0);  // no gram: the pre-set is the answer
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kRepeatStages, g_repeat_ms);
    return TGX_OK;
}

}  // namespace

int tgx_repeat_last_times(const char** names, float* ms, int cap) {
    return stage_times(kRepeatStageNames, g_repeat_ms, tgx::kRepeatStages, names, ms, cap);
}

tgx_status tgx_result_repeat_stats_device(const tgx_result* r, uint32_t width, uint64_t seed, uint32_t flags, void* stream, int64_t* d_stats,
                                          uint8_t* d_mask) {
    const char* who = "tgx_result_repeat_stats_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return repeat_stats(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, width, seed, stream, d_stats,
                        d_mask);
}

tgx_status tgx_corpus_repeat_stats_device(tgx_corpus* c, uint32_t width, uint64_t seed, uint32_t flags, void* stream, int64_t* d_stats,
                                          uint8_t* d_mask) {
    const char* who = "tgx_corpus_repeat_stats_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return repeat_stats(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, width, seed, stream, d_stats, d_mask);
}
