// The C ABI's automaton of up to 64 states over a resident corpus (include/tgx_patterns64.h:
// tgx_corpus_dfa64_hits_device, tgx_dfa64_last_times): the automaton's and the arguments' checks, the table's build and
// upload, the scratch and the stages' times around the launchers of dfa64.hip.  The call runs on the caller's stream
// under a StreamGuard, as the automaton of dfa_ops.cpp does, and shares device_internal.h with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx_patterns64.h"
#include "api_internal.h"
#include "device_internal.h"
#include "dfa64.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_DFA64_MAX_STATES == tgx::kDfa64MaxStates && sizeof(tgx_dfa64) == 8 + tgx::kDfa64TableBytes,
              "include/tgx_patterns64.h and dfa64.h name the same automaton");

namespace {

const char* const kDfa64StageNames[tgx::kDfa64Stages] = {"dfa64_map_kernel", "dfa64_scan", "dfa64_replay_kernel", "dfa64_count_kernel"};
thread_local float g_dfa64_ms[tgx::kDfa64Stages] = {0, 0, 0, 0};

}  // namespace

int tgx_dfa64_last_times(const char** names, float* ms, int cap) { return stage_times(kDfa64StageNames, g_dfa64_ms, tgx::kDfa64Stages, names, ms, cap); }

tgx_status tgx_corpus_dfa64_hits_device(tgx_corpus* c, const tgx_dfa64* dfa, int64_t* d_count, uint8_t* d_ends, void* stream) {
    const char* who = "tgx_corpus_dfa64_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !dfa) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "dfa" : "corpus");
    if (const char* why = tgx::dfa64_check(dfa->n_states, dfa->start, dfa->next, dfa->tag)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    const uint32_t start = dfa->start;
    std::vector<uint64_t> table(tgx::kDfa64TableWords);
    tgx::dfa64_build_table(dfa->n_states, dfa->next, dfa->tag, reinterpret_cast<uint8_t*>(table.data()));
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_count && !d_ends) return fail(TGX_ERR_INVALID, "%s: count and ends are both NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_dfa64_ms, g_dfa64_ms + tgx::kDfa64Stages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "count", d_count, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "ends", d_ends, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kDfa64Stages] = {0, 0, 0, 0};
    StageTimer<tgx::kDfa64Stages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    uint8_t* tags = d_ends;
    if (N) {
        // every chunk of every segment has a map and a mask, the ones past the corpus's end too
        const uint64_t n_segs = tgx::dfa64_segs(N), n_groups = tgx::dfa64_groups(n_segs);
        uint8_t *cmap = nullptr, *srec = nullptr, *grec = nullptr, *gentry = nullptr, *sentry = nullptr;
        uint64_t *cmask = nullptr, *d_table = nullptr;
        if (guard.alloc((size_t)n_segs * tgx::kDfa64Seg, &cmap) != hipSuccess || guard.alloc((size_t)n_segs * tgx::kDfa64SegChunks * 8, &cmask) != hipSuccess ||
            guard.alloc((size_t)n_segs * tgx::kDfa64Map, &srec) != hipSuccess || guard.alloc((size_t)n_groups * tgx::kDfa64Map, &grec) != hipSuccess ||
            guard.alloc((size_t)n_groups, &gentry) != hipSuccess || guard.alloc((size_t)n_segs, &sentry) != hipSuccess ||
            guard.alloc((size_t)tgx::kDfa64TableBytes, &d_table) != hipSuccess || (!tags && guard.alloc((size_t)N, &tags) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (dfa64)");
        }
        HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
        const uint8_t* tab = reinterpret_cast<const uint8_t*>(d_table);
        timer.begin(0);
        if (tgx::launch_dfa64_map(rows, start, tab, cmap, cmask, srec, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dfa64_map_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_dfa64_scan(start, srec, n_segs, grec, gentry, sentry, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_dfa64_replay(rows, start, tab, cmap, cmask, sentry, tags, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dfa64_replay_kernel launch failed");
        timer.end(2);
    }
    if (d_count) {  // (a corpus of empty rows alone: the counts' zeros)
        timer.begin(3);
        if (tgx::launch_dfa64_count(rows, tags, d_count, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dfa64_count_kernel launch failed");
        timer.end(3);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kDfa64Stages, g_dfa64_ms);
    return TGX_OK;
}
