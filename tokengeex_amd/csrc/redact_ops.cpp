// The C ABI's cover and redaction of a resident corpus (include/tgx_redact.h: tgx_corpus_dfa_cover_device,
// tgx_corpus_redact, tgx_redact_last_times): the checks, the tables' build and upload, the scratch and the stages' times
// around the launchers of cover.hip, dfa.hip (the scans of both sides) and redact.hip.  The calls run on the caller's
// stream under a StreamGuard, as the automaton of dfa_ops.cpp and the line view of textstat_ops.cpp do, and share
// device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/tgx_redact.h"
#include "api_internal.h"
#include "cover.h"
#include "device_internal.h"
#include "dfa.h"
#include "redact.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(sizeof(tgx_dfa_cover) == 2 * sizeof(tgx_dfa) + 256, "include/tgx_redact.h and cover.h name the same tables");
static_assert(TGX_REDACT_MAX_CLASSES == tgx::kRedactMaxClasses && TGX_REDACT_MAX_REPL == tgx::kRedactMaxRepl, "include/tgx_redact.h and redact.h name the same limits");

namespace {

constexpr int kStages = tgx::kCoverStages + tgx::kRedactStages;
const char* const kStageNames[kStages] = {"cover_summary_kernel", "cover_scan",           "cover_kernel",      "redact_length_kernel",
                                          "redact_scan",          "redact_offsets_kernel", "redact_fill_kernel"};
thread_local float g_ms[kStages] = {0, 0, 0, 0, 0, 0, 0};

template <uint32_t NSF, uint32_t NSB>
void build_table(const tgx_dfa_cover* cov, uint64_t* words) {
    tgx::cover_build_table<NSF, NSB>(cov->fwd.n_states, cov->fwd.next, cov->fwd.tag, cov->bwd.n_states, cov->bwd.next, cov->cover, words);
}

}  // namespace

int tgx_redact_last_times(const char** names, float* ms, int cap) { return stage_times(kStageNames, g_ms, kStages, names, ms, cap); }

tgx_status tgx_corpus_dfa_cover_device(tgx_corpus* c, const tgx_dfa_cover* cov, int64_t* d_covered, uint8_t* d_mask, void* stream) {
    const char* who = "tgx_corpus_dfa_cover_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !cov) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "cov" : "corpus");
    if (const char* why = tgx::cover_check(cov->fwd.n_states, cov->fwd.start, cov->fwd.next, cov->fwd.tag, cov->bwd.n_states, cov->bwd.start, cov->bwd.next))
        return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    const uint32_t wf = tgx::dfa_width(cov->fwd.n_states), wb = tgx::dfa_width(cov->bwd.n_states), f_start = cov->fwd.start, b_start = cov->bwd.start;
    std::vector<uint64_t> table(tgx::cover_table_words(wf, wb));
    if (wf == 8)
        wb == 8 ? build_table<8, 8>(cov, table.data()) : build_table<8, 16>(cov, table.data());
    else
        wb == 8 ? build_table<16, 8>(cov, table.data()) : build_table<16, 16>(cov, table.data());
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_covered && !d_mask) return fail(TGX_ERR_INVALID, "%s: covered and mask are both NULL", who);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        std::fill(g_ms, g_ms + tgx::kCoverStages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "covered", d_covered, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "mask", d_mask, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kCoverStages] = {0, 0, 0};
    StageTimer<tgx::kCoverStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (rows.n_elems) {
        const uint64_t n_chunks = (rows.n_elems + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk, n_recs = n_chunks + 1;  // (the identity behind the last)
        const size_t f_bytes = (size_t)n_recs * (wf == 8 ? 4 : 8), b_bytes = (size_t)n_recs * (wb == 8 ? 4 : 8);
        ScanScratch scan_f, scan_b;
        const char* oom = "out of device memory (cover)";
        if ((st = scan_room(&scan_f, guard, wf == 8 ? tgx::dfa_scan_bytes8 : tgx::dfa_scan_bytes16, n_recs, oom)) != TGX_OK) return st;
        if ((st = scan_room(&scan_b, guard, wb == 8 ? tgx::dfa_scan_bytes8 : tgx::dfa_scan_bytes16, n_recs, oom)) != TGX_OK) return st;
        uint64_t *rec_f = nullptr, *carry_f = nullptr, *rec_b = nullptr, *carry_b = nullptr, *d_table = nullptr;
        if (guard.alloc(f_bytes, &rec_f) != hipSuccess || guard.alloc(f_bytes, &carry_f) != hipSuccess || guard.alloc(b_bytes, &rec_b) != hipSuccess ||
            guard.alloc(b_bytes, &carry_b) != hipSuccess || guard.alloc(table.size() * 8, &d_table) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "%s", oom);
        }
        HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
        timer.begin(0);
        if (tgx::launch_cover_summary(rows, wf, wb, f_start, b_start, d_table, rec_f, rec_b, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "cover_summary_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_dfa_scan(wf, rec_f, carry_f, n_recs, scan_f.ptr, scan_f.bytes, hs) != hipSuccess ||
            tgx::launch_dfa_scan(wb, rec_b, carry_b, n_recs, scan_b.ptr, scan_b.bytes, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        timer.end(1);
        timer.begin(2);
        if (tgx::launch_cover(rows, wf, wb, f_start, b_start, d_table, carry_f, carry_b, d_covered, d_mask, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "cover_kernel launch failed");
        timer.end(2);
    } else if (tgx::launch_cover(rows, wf, wb, f_start, b_start, nullptr, nullptr, nullptr, d_covered, nullptr, hs) != hipSuccess) {  // only empty rows: the counts' zeros
        return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kCoverStages, g_ms);
    return TGX_OK;
}

tgx_status tgx_corpus_redact(tgx_corpus* c, const uint8_t* d_mask, const uint8_t* repl_bytes, const uint64_t* repl_offs, uint32_t n_repl, uint32_t flags,
                             void* stream, tgx_corpus** out) {
    const char* who = "tgx_corpus_redact";
    if (out) *out = nullptr;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "out" : "corpus");
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::vector<uint64_t> table(tgx::kRedactTableWords);
    if (const char* why = tgx::redact_pack_table(repl_bytes, repl_offs, n_repl, table.data())) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    std::lock_guard<std::mutex> lkc(c->mu);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (N && !d_mask) return fail(TGX_ERR_INVALID, "%s: mask is NULL", who);
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "mask", d_mask, device, "corpus")) != TGX_OK) return st;
    tgx_corpus* made = nullptr;
    float* const ms_out = g_ms + tgx::kCoverStages;
    if (S == 0 || N == 0) {  // no byte: the same rows, all empty
        if ((st = corpus_create(who, device, nullptr, TextFrom::Caller, S ? c->h_offs.data() : nullptr, S, &made)) != TGX_OK) return st;
        std::fill(ms_out, ms_out + tgx::kRedactStages, 0.0f);
        *out = made;
        return TGX_OK;
    }
    hipStream_t hs = stream_or_default(stream, device);
    std::vector<uint64_t> h_offs(S + 1);  // the new offsets visit the host, which corpus_create needs anyway
    std::unique_ptr<tgx_corpus, void (*)(tgx_corpus*)> made_owner(nullptr, tgx_corpus_free);
    float ms[tgx::kRedactStages] = {0, 0, 0, 0};
    StageTimer<tgx::kRedactStages> timer(hs, ms);
    StreamGuard guard(device, hs);  // destroyed before them: a failed call's queued work is over before they go
    const uint64_t n_chunks = (N + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk, n_recs = n_chunks + 1;
    const char* oom = "out of device memory (redact)";
    ScanScratch scan;
    if ((st = scan_room(&scan, guard, tgx::redact_scan_bytes, n_recs, oom)) != TGX_OK) return st;
    uint64_t *rec = nullptr, *carry = nullptr, *d_table = nullptr, *d_new_offs = nullptr;
    if (guard.alloc((size_t)n_recs * 8, &rec) != hipSuccess || guard.alloc((size_t)n_recs * 8, &carry) != hipSuccess ||
        guard.alloc(table.size() * 8, &d_table) != hipSuccess || guard.alloc((size_t)(S + 1) * 8, &d_new_offs) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "%s", oom);
    }
    HIP_TRY(guard.upload(d_table, std::move(table)));
    timer.begin(0);
    if (tgx::launch_redact_lengths(rows, d_mask, n_repl, d_table, rec, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "redact_length_kernel launch failed");
    timer.end(0);
    timer.begin(1);
    if (tgx::launch_redact_scan(rec, carry, n_recs, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
    timer.end(1);
    timer.begin(2);
    if (tgx::launch_redact_offsets(rows, d_mask, n_repl, d_table, carry, d_new_offs, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "redact_offsets_kernel launch failed");
    timer.end(2);
    // the new offsets, whose last is the new length, size the output: a host visit of its own
    if ((st = read_u64(hs, d_new_offs, h_offs.data(), (size_t)(S + 1))) != TGX_OK) return st;
    if ((st = corpus_create(who, device, nullptr, TextFrom::Caller, h_offs.data(), S, &made)) != TGX_OK) {
        guard.done();  // (the stream has reached its end)
        return st;
    }
    made_owner.reset(made);
    timer.begin(3);
    if (made->n_bytes && tgx::launch_redact_fill(rows, d_mask, n_repl, d_table, carry, made->d_text, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "redact_fill_kernel launch failed");
    timer.end(3);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kRedactStages, ms_out);
    *out = made_owner.release();
    return TGX_OK;
}
