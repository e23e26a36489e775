// The C ABI's automaton over a resident corpus (include/tgx_patterns.h: tgx_corpus_dfa_hits_device, tgx_dfa_last_times):
// the automaton's and the arguments' checks, the table's build and upload, the scratch and the stages' times around the
// launchers of dfa.hip.  The call runs on the caller's stream under a StreamGuard, as the word statistics of
// wordstat_ops.cpp do, and shares device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx_patterns.h"
#include "api_internal.h"
#include "device_internal.h"
#include "dfa.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_DFA_MAX_STATES == tgx::kDfaMaxStates && sizeof(tgx_dfa) == 8 + 256 * 16 + 16, "include/tgx_patterns.h and dfa.h name the same automaton");

namespace {

const char* const kDfaStageNames[tgx::kDfaStages] = {"dfa_summary_kernel", "dfa_scan", "dfa_kernel"};
thread_local float g_dfa_ms[tgx::kDfaStages] = {0, 0, 0};

}  // namespace

int tgx_dfa_last_times(const char** names, float* ms, int cap) { return stage_times(kDfaStageNames, g_dfa_ms, tgx::kDfaStages, names, ms, cap); }

tgx_status tgx_corpus_dfa_hits_device(tgx_corpus* c, const tgx_dfa* dfa, int64_t* d_count, uint8_t* d_ends, void* stream) {
    const char* who = "tgx_corpus_dfa_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !dfa) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "dfa" : "corpus");
    if (const char* why = tgx::dfa_check(dfa->n_states, dfa->start, dfa->next, dfa->tag)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    const uint32_t width = tgx::dfa_width(dfa->n_states), start = dfa->start;
    std::vector<uint64_t> table(width == 8 ? tgx::kDfaTableWords<8> : tgx::kDfaTableWords<16>);
    if (width == 8)
        tgx::dfa_build_table<8>(dfa->n_states, dfa->next, dfa->tag, table.data());
    else
        tgx::dfa_build_table<16>(dfa->n_states, dfa->next, dfa->tag, table.data());
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_count && !d_ends) return fail(TGX_ERR_INVALID, "%s: count and ends are both NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_dfa_ms, g_dfa_ms + tgx::kDfaStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "count", d_count, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "ends", d_ends, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kDfaStages] = {0, 0, 0};
    StageTimer<tgx::kDfaStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (rows.n_elems) {
        const uint64_t n_chunks = (rows.n_elems + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk, n_recs = n_chunks + 1;  // (the identity behind the last)
        const size_t rec_bytes = (size_t)n_recs * (width == 8 ? 4 : 8);
        ScanScratch scan;
        if ((st = scan_room(&scan, guard, width == 8 ? tgx::dfa_scan_bytes8 : tgx::dfa_scan_bytes16, n_recs, "out of device memory (dfa)")) != TGX_OK) return st;
        uint64_t *rec = nullptr, *carry = nullptr, *d_table = nullptr;
        if (guard.alloc(rec_bytes, &rec) != hipSuccess || guard.alloc(rec_bytes, &carry) != hipSuccess || guard.alloc(table.size() * 8, &d_table) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (dfa)");
        }
        HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
        timer.begin(0);
        if (tgx::launch_dfa_summary(rows, width, start, d_table, rec, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dfa_summary_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_dfa_scan(width, rec, carry, n_recs, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_dfa(rows, width, start, d_table, carry, d_count, d_ends, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "dfa_kernel launch failed");
        timer.end(2);
    } else if (tgx::launch_dfa(rows, width, start, nullptr, nullptr, d_count, nullptr, hs) != hipSuccess) {  // only empty rows: the counts' zeros
        return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kDfaStages, g_dfa_ms);
    return TGX_OK;
}
