// The C ABI's word statistics of a resident corpus (include/tgx_words.h: tgx_corpus_word_stats_device,
// tgx_wordstat_last_times): the argument checks, the stop table, the scratch and the stages' times around the launchers
// of wordstat.hip.  The call runs on the caller's stream under a StreamGuard, as the text statistics of textstat_ops.cpp
// do, and shares device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx_words.h"
#include "api_internal.h"
#include "device_internal.h"
#include "wordstat.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_WORDSTAT_N == tgx::kWordstatN && TGX_WORDSTAT_CHARS == tgx::kWordstatChars && TGX_WORDSTAT_FOLD == tgx::kWordstatFold,
              "include/tgx_words.h and wordstat.h name the same table and flags");

namespace {

const char* const kWordstatStageNames[tgx::kWordstatStages] = {"wordstat_summary_kernel", "wordstat_scan", "wordstat_kernel"};
thread_local float g_wordstat_ms[tgx::kWordstatStages] = {0, 0, 0};

}  // namespace

int tgx_wordstat_last_times(const char** names, float* ms, int cap) {
    return stage_times(kWordstatStageNames, g_wordstat_ms, tgx::kWordstatStages, names, ms, cap);
}

tgx_status tgx_corpus_word_stats_device(tgx_corpus* c, uint64_t word_limit, const uint8_t* stop_bytes, const uint64_t* stop_offs, uint32_t n_stop,
                                        uint32_t flags, void* stream, int64_t* d_stats, uint8_t* d_marks) {
    const char* who = "tgx_corpus_word_stats_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, TGX_WORDSTAT_CHARS | TGX_WORDSTAT_FOLD)) != TGX_OK) return st;
    std::vector<uint64_t> table(tgx::kWordstatStopWords * std::max<uint32_t>(std::min(n_stop, tgx::kWordstatMaxStop), 1u));
    if (const char* why = tgx::wordstat_pack_table(stop_bytes, stop_offs, n_stop, flags, table.data())) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_stats && !d_marks) return fail(TGX_ERR_INVALID, "%s: d_stats and d_marks are both NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_wordstat_ms, g_wordstat_ms + tgx::kWordstatStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_stats", d_stats, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_marks", d_marks, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kWordstatStages] = {0, 0, 0};
    StageTimer<tgx::kWordstatStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (rows.n_elems) {
        const uint64_t n_chunks = (rows.n_elems + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk;
        ScanScratch scan;
        if ((st = scan_room(&scan, guard, tgx::wordstat_scan_bytes, n_chunks, "out of device memory (word statistics)")) != TGX_OK) return st;
        uint64_t *summary = nullptr, *carry = nullptr, *d_table = nullptr;
        if (guard.alloc((size_t)n_chunks * 8, &summary) != hipSuccess || guard.alloc((size_t)n_chunks * 8, &carry) != hipSuccess ||
            guard.alloc(table.size() * 8, &d_table) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (word statistics)");
        }
        if (n_stop) HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
        timer.begin(0);
        if (tgx::launch_wordstat_summary(rows, flags, summary, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "wordstat_summary_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_wordstat_scan(summary, carry, n_chunks, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_wordstat(rows, word_limit, flags, d_table, n_stop, carry, d_stats, d_marks, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "wordstat_kernel launch failed");
        timer.end(2);
    } else if (tgx::launch_wordstat(rows, word_limit, flags, nullptr, 0, nullptr, d_stats, nullptr, hs) != hipSuccess) {  // only empty rows: the table's zeros
        return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kWordstatStages, g_wordstat_ms);
    return TGX_OK;
}
