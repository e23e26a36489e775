// The C ABI's text statistics and line view of a resident corpus (include/tgx.h: tgx_corpus_text_stats_device,
// tgx_corpus_lines, tgx_textstat_last_times): the argument checks, the scratch and the stages' times around the launchers
// of textstat.hip.  They run on the caller's stream under a StreamGuard, as the gram calls of gram_ops.cpp do, and share
// device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "textstat.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_TEXTSTAT_N == tgx::kTextstatN && TGX_TEXTSTAT_CHARS == tgx::kTextstatChars, "include/tgx.h and textstat.h name the same table and flag");

namespace {

const char* const kTextstatStageNames[tgx::kTextstatStages] = {"textstat_summary_kernel", "textstat_scan", "textstat_kernel", "textstat_lines"};
thread_local float g_textstat_ms[tgx::kTextstatStages] = {0, 0, 0, 0};

// The three stages that both calls share, queued on hs: the summaries, their scan, the kernel.  The corpus has a row and
// a byte.  Stages 0 .. 2 of the timer are set here.
template <int N>
tgx_status textstat_passes(const char* who, const tgx::DedupRows& rows, uint64_t line_limit, uint32_t flags, StreamGuard& guard, StageTimer<N>& timer,
                           hipStream_t hs, int64_t* d_stats, uint8_t* d_line_start) {
    const uint64_t n_chunks = (rows.n_elems + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk;
    ScanScratch scan;
    tgx_status st = scan_room(&scan, guard, tgx::textstat_scan_bytes, n_chunks, "out of device memory (text statistics)");
    if (st != TGX_OK) return st;
    uint64_t *summary = nullptr, *carry = nullptr;
    if (guard.alloc((size_t)n_chunks * 8, &summary) != hipSuccess || guard.alloc((size_t)n_chunks * 8, &carry) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (text statistics)");
    }
    timer.begin(0);
    if (tgx::launch_textstat_summary(rows, flags, summary, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "textstat_summary_kernel launch failed");
    timer.end(0);
    timer.begin(1);
    if (tgx::launch_textstat_scan(summary, carry, n_chunks, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
    timer.end(1);
    timer.begin(2);
    if (tgx::launch_textstat(rows, line_limit, flags, carry, d_stats, d_line_start, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "textstat_kernel launch failed");
    timer.end(2);
    return TGX_OK;
}

}  // namespace

int tgx_textstat_last_times(const char** names, float* ms, int cap) {
    return stage_times(kTextstatStageNames, g_textstat_ms, tgx::kTextstatStages, names, ms, cap);
}

tgx_status tgx_corpus_text_stats_device(tgx_corpus* c, uint64_t line_limit, uint32_t flags, void* stream, int64_t* d_stats, uint8_t* d_line_start) {
    const char* who = "tgx_corpus_text_stats_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, TGX_TEXTSTAT_CHARS)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_stats && !d_line_start) return fail(TGX_ERR_INVALID, "%s: d_stats and d_line_start are both NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_textstat_ms, g_textstat_ms + tgx::kTextstatStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_stats", d_stats, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_line_start", d_line_start, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[3] = {0, 0, 0};
    StageTimer<3> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (rows.n_elems) {
        if ((st = textstat_passes(who, rows, line_limit, flags, guard, timer, hs, d_stats, d_line_start)) != TGX_OK) return st;
    } else if (tgx::launch_textstat(rows, line_limit, flags, nullptr, d_stats, nullptr, hs) != hipSuccess) {  // only empty rows: the table's zeros
        return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + 3, g_textstat_ms);
    g_textstat_ms[3] = 0;
    return TGX_OK;
}

tgx_status tgx_corpus_lines(tgx_corpus* c, uint32_t flags, void* stream, tgx_corpus** out) {
    const char* who = "tgx_corpus_lines";
    if (out) *out = nullptr;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "out" : "corpus");
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    tgx_corpus* made = nullptr;
    if (S == 0 || N == 0) {  // no line: an empty corpus
        if ((st = corpus_create(who, device, nullptr, TextFrom::Caller, nullptr, 0, &made)) != TGX_OK) return st;
        std::fill(g_textstat_ms, g_textstat_ms + tgx::kTextstatStages, 0.0f);
        *out = made;
        return TGX_OK;
    }
    hipStream_t hs = stream_or_default(stream, device);
    std::vector<uint64_t> h_offs;  // the lines' offsets visit the host, which corpus_create needs anyway
    unsigned long long h_count = 0;
    float ms[tgx::kTextstatStages] = {0, 0, 0, 0};
    StageTimer<tgx::kTextstatStages> timer(hs, ms);
    StreamGuard guard(device, hs);  // destroyed before them: a failed call's queued work is over before they go
    uint8_t* marks = nullptr;
    unsigned long long* d_count = nullptr;
    size_t count_bytes = 0, select_bytes = 0;
    if (tgx::textstat_lines_bytes(N, &count_bytes, &select_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    void* tmp = nullptr;
    if (guard.alloc((size_t)N, &marks) != hipSuccess || guard.alloc(sizeof(unsigned long long), &d_count) != hipSuccess ||
        guard.alloc(std::max(count_bytes, select_bytes) + 8, &tmp) != hipSuccess) {  // (never NULL: that asks for the size)
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (lines)");
    }
    if ((st = textstat_passes(who, rows, 0, 0, guard, timer, hs, nullptr, marks)) != TGX_OK) return st;
    // the marks' number sizes the compaction's destination: a host visit of its own
    timer.begin(3);
    if (tgx::launch_textstat_count(marks, N, d_count, tmp, count_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: count launch failed", who);
    if ((st = read_u64(hs, d_count, &h_count)) != TGX_OK) return st;
    const uint64_t n_lines = h_count;
    if (n_lines > tgx::kTextstatMaxLines) {
        guard.done();  // (the stream has reached its end)
        return fail(TGX_ERR_UNSUPPORTED, "%s: 2^32-1 lines or more", who);
    }
    uint64_t* d_starts = nullptr;
    if (guard.alloc((size_t)n_lines * 8, &d_starts) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (lines)");
    }
    if (tgx::launch_textstat_compact(marks, N, d_starts, d_count, tmp, select_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: select launch failed", who);
    timer.end(3);
    h_offs.resize(n_lines + 1);
    if ((st = read_u64(hs, d_starts, h_offs.data(), (size_t)n_lines)) != TGX_OK) return st;
    h_offs[n_lines] = N;
    guard.done();  // (the stream has reached its end; the text's copy is corpus_create's own)
    timer.read();
    std::copy(ms, ms + tgx::kTextstatStages, g_textstat_ms);
    if ((st = corpus_create(who, device, c->d_text, TextFrom::Device, h_offs.data(), n_lines, &made)) != TGX_OK) return st;
    *out = made;
    return TGX_OK;
}
