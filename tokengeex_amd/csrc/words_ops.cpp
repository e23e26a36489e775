// The C ABI's word ids of a resident corpus (include/tgx_word_ids.h: tgx_corpus_words, tgx_words_last_times): the argument
// checks, the scratch, the one host visit, the result and the stages' times around the launchers of words.hip.  The call
// runs on the caller's stream under a StreamGuard, as the word statistics of wordstat_ops.cpp do, and builds its result
// from two device buffers as tgx_result_select of result_ops.cpp does; it shares device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>

#include "../../include/tgx_word_ids.h"
#include "api_internal.h"
#include "device_internal.h"
#include "words.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_WORDS_FOLD == tgx::kWordsFold && TGX_WORDS_VOCAB_SIZE == tgx::kWordsVocabSize, "include/tgx_word_ids.h and words.h name the same flag and bound");
static_assert(sizeof(tgx::WordsRec) == 32 && offsetof(tgx::WordsRec, ends) == 16, "the totals' word ends are read as one 8-byte word");

namespace {

const char* const kWordsStageNames[tgx::kWordsStages] = {"words_summary_kernel", "words_scan", "words_kernel", "words_offsets_kernel"};
thread_local float g_words_ms[tgx::kWordsStages] = {0, 0, 0, 0};

}  // namespace

int tgx_words_last_times(const char** names, float* ms, int cap) { return stage_times(kWordsStageNames, g_words_ms, tgx::kWordsStages, names, ms, cap); }

tgx_status tgx_corpus_words(tgx_corpus* c, uint32_t flags, uint64_t seed, void* stream, tgx_result** out) {
    const char* who = "tgx_corpus_words";
    if (out) *out = nullptr;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "out" : "corpus");
    if ((st = layout_check_flags(who, flags, TGX_WORDS_FOLD)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows, N = rows.n_elems;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    hipStream_t hs = stream_or_default(stream, device);
    std::unique_ptr<tgx_result> res(new tgx_result());  // before the guard: its buffers go back after the stream's end
    unsigned long long h_words = 0;
    float ms[tgx::kWordsStages] = {0, 0, 0, 0};
    StageTimer<tgx::kWordsStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    res->device = device;
    res->vocab_size = tgx::kWordsVocabSize;
    res->n_samples = S;
    if (res->d_offs.alloc(device, (size_t)(S + 1) * 8) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (words)");
    tgx::WordsRec* carry = nullptr;
    if (S && N) {
        const uint64_t n_chunks = (N + tgx::kTextstatChunk - 1) / tgx::kTextstatChunk, n_recs = n_chunks + 1;  // (the totals' record)
        ScanScratch scan;
        if ((st = scan_room(&scan, guard, tgx::words_scan_bytes, n_recs, "out of device memory (words)")) != TGX_OK) return st;
        tgx::WordsRec* rec = nullptr;
        if (guard.alloc((size_t)n_recs * sizeof(tgx::WordsRec), &rec) != hipSuccess || guard.alloc((size_t)n_recs * sizeof(tgx::WordsRec), &carry) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (words)");
        }
        timer.begin(0);
        if (tgx::launch_words_summary(rows, flags, rec, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "words_summary_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_words_scan(rec, carry, n_recs, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        timer.end(1);
        // the one word that visits the host: the number of words sizes the ids
        if ((st = read_u64(hs, &carry[n_chunks].ends, &h_words)) != TGX_OK) return st;
        if (h_words > tgx::kWordsMaxWords) {
            guard.done();  // (the stream has reached its end)
            return fail(TGX_ERR_UNSUPPORTED, "%s: 2^32-1 words or more", who);
        }
        if (h_words > N) return fail(TGX_ERR_DEVICE, "%s: %llu words from %llu bytes", who, h_words, (unsigned long long)N);
    }
    res->n_tokens = h_words;
    if (res->d_ids.alloc(device, (size_t)h_words * 4 + 256) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (words)");
    timer.begin(2);
    if (tgx::launch_words_emit(rows, flags, seed, carry, res->d_ids, h_words, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "words_kernel launch failed");
    timer.end(2);
    timer.begin(3);
    if (tgx::launch_words_offsets(rows, carry, res->d_offs, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "words_offsets_kernel launch failed");
    timer.end(3);
    // the stream has reached its end before the result can change hands (the guard: also after a failure)
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kWordsStages, g_words_ms);
    *out = res.release();
    return TGX_OK;
}
