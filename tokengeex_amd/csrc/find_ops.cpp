// The C ABI's leftmost-first matches and idiom mining over a resident corpus (include/tgx_find.h:
// tgx_corpus_find_device, tgx_corpus_mine_device, tgx_find_last_times): the automaton's and the arguments' checks, the
// table's build and upload, the scratch and the stages' times around the launchers of find.hip, the scan of dfa64.hip and
// the compaction of textstat.hip.  Both calls run on the caller's stream under a StreamGuard, as dfa64_ops.cpp's does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx_find.h"
#include "api_internal.h"
#include "device_internal.h"
#include "find.h"
#include "textstat.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_FIND_MAX_LEN == tgx::kFindMaxLen, "include/tgx_find.h and find.h name the same limit");

namespace {

const char* const kFindStageNames[tgx::kFindStages] = {"find_walk_kernel", "find_scan", "find_replay_kernel", "find_keys", "find_sort_runs", "find_order"};
thread_local float g_find_ms[tgx::kFindStages] = {0, 0, 0, 0, 0, 0};

using FindTimer = StageTimer<tgx::kFindStages>;

tgx_status find_check(const char* who, const tgx_corpus* c, const tgx_dfa64* dfa, uint32_t max_len) {
    if (!c || !dfa) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "dfa" : "corpus");
    if (const char* why = tgx::dfa64_check(dfa->n_states, dfa->start, dfa->next, dfa->tag)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    if (const char* why = tgx::find_check_max_len(max_len)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    return TGX_OK;
}

// The three stages of a find over N > 0 bytes: walk u8[N] gets the walk bytes; lens (NULL, or walk itself), count and
// truncated are the replay's.
tgx_status find_stages(const char* who, const tgx::DedupRows& rows, const tgx_dfa64* dfa, uint32_t max_len, StreamGuard& guard, FindTimer& timer, hipStream_t hs,
                       uint8_t* walk, uint8_t* lens, int64_t* count, int64_t* truncated) {
    const uint64_t n_segs = tgx::dfa64_segs(rows.n_elems), n_groups = tgx::dfa64_groups(n_segs);
    uint8_t *srec = nullptr, *grec = nullptr, *gentry = nullptr, *sentry = nullptr;
    uint64_t* d_table = nullptr;
    if (guard.alloc((size_t)n_segs * tgx::kDfa64Map, &srec) != hipSuccess || guard.alloc((size_t)n_groups * tgx::kDfa64Map, &grec) != hipSuccess ||
        guard.alloc((size_t)n_groups, &gentry) != hipSuccess || guard.alloc((size_t)n_segs, &sentry) != hipSuccess ||
        guard.alloc((size_t)tgx::kFindTableBytes, &d_table) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (find)");
    }
    std::vector<uint64_t> table(tgx::kFindTableWords);
    tgx::find_build_table(dfa->n_states, dfa->next, dfa->tag, reinterpret_cast<uint8_t*>(table.data()));
    HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
    timer.begin(0);
    if (tgx::launch_find_walk(rows, dfa->start, max_len, reinterpret_cast<const uint8_t*>(d_table), walk, srec, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "find_walk_kernel launch failed");
    timer.end(0);
    timer.begin(1);
    if (tgx::launch_dfa64_scan(0, srec, n_segs, grec, gentry, sentry, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
    timer.end(1);
    timer.begin(2);
    if (tgx::launch_find_replay(rows, walk, sentry, lens, count, truncated, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "find_replay_kernel launch failed");
    timer.end(2);
    return TGX_OK;
}

hipError_t find_lines_bytes(uint64_t n, size_t* bytes) {
    size_t count_bytes = 0, select_bytes = 0;
    const hipError_t e = tgx::textstat_lines_bytes(n, &count_bytes, &select_bytes);
    *bytes = std::max(count_bytes, select_bytes) + 8;  // (never 0: a NULL room asks for the size)
    return e;
}

}  // namespace

int tgx_find_last_times(const char** names, float* ms, int cap) { return stage_times(kFindStageNames, g_find_ms, tgx::kFindStages, names, ms, cap); }

tgx_status tgx_corpus_find_device(tgx_corpus* c, const tgx_dfa64* dfa, uint32_t max_len, int64_t* d_count, uint8_t* d_lens, int64_t* d_truncated, void* stream) {
    const char* who = "tgx_corpus_find_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if ((st = find_check(who, c, dfa, max_len)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_count && !d_lens && !d_truncated) return fail(TGX_ERR_INVALID, "%s: count, lens and truncated are all NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_find_ms, g_find_ms + tgx::kFindStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "count", d_count, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "lens", d_lens, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "truncated", d_truncated, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kFindStages] = {0, 0, 0, 0, 0, 0};
    FindTimer timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (N) {
        uint8_t* walk = d_lens;
        if (!walk && guard.alloc((size_t)N, &walk) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (find)");
        }
        if ((st = find_stages(who, rows, dfa, max_len, guard, timer, hs, walk, d_lens, d_count, d_truncated)) != TGX_OK) return st;
    } else if (tgx::launch_find_replay(rows, nullptr, nullptr, nullptr, d_count, d_truncated, hs) != hipSuccess) {  // (empty rows alone: the counts' zeros)
        return fail(TGX_ERR_DEVICE, "%s: pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kFindStages, g_find_ms);
    return TGX_OK;
}

tgx_status tgx_corpus_mine_device(tgx_corpus* c, const tgx_dfa64* dfa, uint32_t max_len, uint64_t top, uint64_t seed, uint64_t* out_pos, uint32_t* out_len,
                                  uint64_t* out_count, uint64_t* n_out, uint64_t* n_distinct, uint64_t* n_matches, void* stream) {
    const char* who = "tgx_corpus_mine_device";
    if (n_out) *n_out = 0;
    if (n_distinct) *n_distinct = 0;
    if (n_matches) *n_matches = 0;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if ((st = find_check(who, c, dfa, max_len)) != TGX_OK) return st;
    if (top == 0) return fail(TGX_ERR_INVALID, "%s: top is 0", who);
    if (!out_pos || !out_len || !out_count || !n_out) return fail(TGX_ERR_INVALID, "%s: an output is NULL", who);
    std::lock_guard<std::mutex> lkc(c->mu);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0 || N == 0) {
        std::fill(g_find_ms, g_find_ms + tgx::kFindStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kFindStages] = {0, 0, 0, 0, 0, 0};
    unsigned long long h_n = 0, h_runs = 0;  // (before the guard: a failed copy may still write them)
    std::vector<uint64_t> h_top;
    FindTimer timer(hs, ms);
    StreamGuard guard(device, hs);
    uint8_t* lens = nullptr;
    unsigned long long* d_n = nullptr;
    void* lines_tmp = nullptr;
    size_t lines_bytes = 0;
    if (find_lines_bytes(N, &lines_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    if (guard.alloc((size_t)N, &lens) != hipSuccess || guard.alloc(sizeof(unsigned long long), &d_n) != hipSuccess ||
        guard.alloc(lines_bytes, &lines_tmp) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (mine)");
    }
    if ((st = find_stages(who, rows, dfa, max_len, guard, timer, hs, lens, lens, nullptr, nullptr)) != TGX_OK) return st;
    // the matches' number sizes what follows: a host visit of its own, as the line view's
    timer.begin(3);
    if (tgx::launch_textstat_count(lens, N, d_n, lines_tmp, lines_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: count launch failed", who);
    if ((st = read_u64(hs, d_n, &h_n)) != TGX_OK) return st;
    const uint64_t n = h_n;
    uint64_t n_top = 0;
    if (n) {
        uint64_t *pos = nullptr, *keys = nullptr, *pos2 = nullptr, *keys2 = nullptr;
        uint8_t* heads = nullptr;
        void* sort_tmp = nullptr;
        size_t sort_bytes = 0;
        if (tgx::find_sort_bytes(n, &sort_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
        if (guard.alloc((size_t)n * 8, &pos) != hipSuccess || guard.alloc((size_t)n * 8, &keys) != hipSuccess || guard.alloc((size_t)n * 8, &pos2) != hipSuccess ||
            guard.alloc((size_t)n * 8, &keys2) != hipSuccess || guard.alloc((size_t)n, &heads) != hipSuccess || guard.alloc(sort_bytes + 8, &sort_tmp) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (mine)");
        }
        if (tgx::launch_textstat_compact(lens, N, pos, d_n, lines_tmp, lines_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: select launch failed", who);
        if (tgx::launch_find_keys(c->d_text, lens, pos, n, seed, keys, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "find_key_kernel launch failed");
        timer.end(3);
        timer.begin(4);
        if (tgx::launch_find_sort(keys, keys2, pos, pos2, n, sort_tmp, sort_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: sort launch failed", who);
        if (tgx::launch_find_heads(keys2, n, heads, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "find_head_kernel launch failed");
        if (tgx::launch_textstat_count(heads, n, d_n, lines_tmp, lines_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: count launch failed", who);
        if ((st = read_u64(hs, d_n, &h_runs)) != TGX_OK) return st;
        const uint64_t n_runs = h_runs;  // >= 1
        n_top = std::min(top, n_runs);
        // keys and pos are free again: the runs' heads, first positions and counts, and the room of the two sorts
        uint64_t *head = keys, *run_pos = pos, *run_count = nullptr, *pos_tmp = nullptr, *count_tmp = nullptr, *d_top = nullptr;
        if (guard.alloc((size_t)n_runs * 8, &run_count) != hipSuccess || guard.alloc((size_t)n_runs * 8, &pos_tmp) != hipSuccess ||
            guard.alloc((size_t)n_runs * 8, &count_tmp) != hipSuccess || guard.alloc((size_t)n_top * 24, &d_top) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (mine)");
        }
        if (tgx::launch_textstat_compact(heads, n, head, d_n, lines_tmp, lines_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: select launch failed", who);
        if (tgx::launch_find_runs(head, n_runs, n, pos2, run_pos, run_count, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "find_run_kernel launch failed");
        timer.end(4);
        timer.begin(5);
        if (tgx::launch_find_order(run_pos, run_count, pos_tmp, count_tmp, n_runs, sort_tmp, sort_bytes, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "%s: sort launch failed", who);
        if (tgx::launch_find_top(run_pos, run_count, lens, n_top, d_top, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "find_top_kernel launch failed");
        timer.end(5);
        h_top.resize(3 * n_top);
        if ((st = read_u64(hs, d_top, h_top.data(), 3 * n_top)) != TGX_OK) return st;
    } else {
        timer.end(3);
    }
    guard.done();  // (the stream has reached its end)
    timer.read();
    std::copy(ms, ms + tgx::kFindStages, g_find_ms);
    for (uint64_t i = 0; i < n_top; i++) {
        out_pos[i] = h_top[3 * i];
        out_len[i] = (uint32_t)h_top[3 * i + 1];
        out_count[i] = h_top[3 * i + 2];
    }
    *n_out = n_top;
    if (n_distinct) *n_distinct = h_runs;
    if (n_matches) *n_matches = n;
    return TGX_OK;
}
