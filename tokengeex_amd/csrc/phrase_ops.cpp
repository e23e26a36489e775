// The C ABI's literal phrase matching (include/tgx_phrases.h: tgx_phraseset_create / _info / _free,
// tgx_corpus_phrase_hits_device, tgx_result_phrase_hits_device, tgx_phrase_last_times): the handle, the argument checks
// and the stage's time around the launcher of phrase.hip.  The hits calls run on the caller's stream under a StreamGuard,
// as the gram calls of gram_ops.cpp do, and share device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>

#include "../../include/tgx_phrases.h"
#include "api_internal.h"
#include "device_internal.h"
#include "phrase.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_PHRASE_FOLD_CASE == tgx::kPhraseFoldCase && TGX_PHRASE_WHOLE_WORD == tgx::kPhraseWholeWord,
              "include/tgx_phrases.h and phrase.h name the same flags");

// A phrase set: the records and the first-level filter, in pooled memory of its device.  Read-only after creation, so
// concurrent hit calls share it without a lock.
struct tgx_phraseset {
    int device = 0;
    uint32_t n_phrases = 0, n_distinct = 0, elem_bytes = 0, flags = 0, max_len = 0, root_base = 0;
    uint64_t table_bytes = 0;
    PoolBuf<tgx::PhraseRec> d_rec;  // PhraseRec[n_slots]
    PoolBuf<uint32_t> d_filter;     // u32[kPhraseFilterWords]
};

namespace {

const char* const kPhraseStageNames[tgx::kPhraseStages] = {"phrase_hits_kernel"};
thread_local float g_phrase_ms[tgx::kPhraseStages] = {0};

// count, longest and per_phrase of the rows of a result or of a corpus against a set.  The handle, the flags and a device
// have been checked.
tgx_status phrase_hits(const char* who, const tgx::DedupRows& rows, int device, const tgx_phraseset* ps, void* stream, int64_t* d_count,
                       uint8_t* d_longest, int64_t* d_per_phrase) {
    if (!ps) return fail(TGX_ERR_INVALID, "%s: phrase set is NULL", who);
    if (ps->elem_bytes != rows.elem_bytes)
        return fail(TGX_ERR_INVALID, "%s: the set holds phrases of %u-byte elements, the source has %u-byte elements", who, ps->elem_bytes, rows.elem_bytes);
    if (ps->device != device) return fail(TGX_ERR_INVALID, "%s: the set is on device %d, the source on device %d", who, ps->device, device);
    if (!d_count && !d_longest && !d_per_phrase) return fail(TGX_ERR_INVALID, "%s: d_count, d_longest and d_per_phrase are all NULL", who);
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    tgx_status st;
    if ((st = check_device_ptr(who, "d_count", d_count, device, "source")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_longest", d_longest, device, "source")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_per_phrase", d_per_phrase, device, "source")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kPhraseStages] = {0};
    StageTimer<tgx::kPhraseStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    timer.begin(0);
    if (tgx::launch_phrase_hits(rows, ps->d_rec.get(), ps->d_filter.get(), ps->root_base, ps->max_len, ps->flags, ps->n_phrases, d_count, d_longest,
                                d_per_phrase, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "phrase_hits_kernel launch failed");
    timer.end(0);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + tgx::kPhraseStages, g_phrase_ms);
    return TGX_OK;
}

}  // namespace

int tgx_phrase_last_times(const char** names, float* ms, int cap) {
    return stage_times(kPhraseStageNames, g_phrase_ms, tgx::kPhraseStages, names, ms, cap);
}

tgx_status tgx_phraseset_create(int device, const void* phrases, const uint64_t* phrase_offs, uint32_t n_phrases, uint32_t elem_bytes, uint32_t flags,
                                tgx_phraseset** out) {
    const char* who = "tgx_phraseset_create";
    if (out) *out = nullptr;
    int n_devices = 0;
    tgx_status st = require_device(&n_devices);
    if (st != TGX_OK) return st;
    if (!out) return fail(TGX_ERR_INVALID, "%s: out is NULL", who);
    if (device < 0 || device >= n_devices) return fail(TGX_ERR_INVALID, "%s: device %d of %d", who, device, n_devices);
    tgx::PhraseTable table;
    const char* why = nullptr;
    const tgx::PhraseBuild built = tgx::phrase_build_table(phrases, phrase_offs, n_phrases, elem_bytes, flags, &table, &why);
    if (built != tgx::kPhraseOk) return fail(built == tgx::kPhraseInvalid ? TGX_ERR_INVALID : TGX_ERR_UNSUPPORTED, "%s: %s", who, why);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<tgx_phraseset> ps(new tgx_phraseset());
    ps->device = device;
    ps->n_phrases = n_phrases;
    ps->n_distinct = table.n_distinct;
    ps->elem_bytes = elem_bytes;
    ps->flags = flags;
    ps->max_len = table.max_len;
    ps->root_base = table.root_base;
    const size_t rec_bytes = table.rec.size() * sizeof(tgx::PhraseRec), filter_bytes = (size_t)tgx::kPhraseFilterWords * 4;
    ps->table_bytes = rec_bytes + filter_bytes;
    if (ps->d_rec.alloc(device, rec_bytes) != hipSuccess || ps->d_filter.alloc(device, filter_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (phrase set)");
    }
    if (copy_sync(ps->d_rec.get(), table.rec.data(), rec_bytes, hipMemcpyHostToDevice, device) != hipSuccess ||
        copy_sync(ps->d_filter.get(), table.filter.data(), filter_bytes, hipMemcpyHostToDevice, device) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "%s: the copy failed", who);
    *out = ps.release();
    return TGX_OK;
}

tgx_status tgx_phraseset_info(const tgx_phraseset* ps, uint32_t* n_phrases, uint32_t* n_distinct, uint32_t* elem_bytes, uint32_t* flags,
                              uint32_t* max_len, int* device, uint64_t* table_bytes) {
    if (!ps) return fail(TGX_ERR_INVALID, "tgx_phraseset_info: phrase set is NULL");
    if (n_phrases) *n_phrases = ps->n_phrases;
    if (n_distinct) *n_distinct = ps->n_distinct;
    if (elem_bytes) *elem_bytes = ps->elem_bytes;
    if (flags) *flags = ps->flags;
    if (max_len) *max_len = ps->max_len;
    if (device) *device = ps->device;
    if (table_bytes) *table_bytes = ps->table_bytes;
    return TGX_OK;
}

void tgx_phraseset_free(tgx_phraseset* ps) { delete ps; }

tgx_status tgx_result_phrase_hits_device(const tgx_result* r, const tgx_phraseset* ps, uint32_t flags, void* stream, int64_t* d_count,
                                         uint8_t* d_longest, int64_t* d_per_phrase) {
    const char* who = "tgx_result_phrase_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return phrase_hits(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, ps, stream, d_count, d_longest,
                       d_per_phrase);
}

tgx_status tgx_corpus_phrase_hits_device(tgx_corpus* c, const tgx_phraseset* ps, uint32_t flags, void* stream, int64_t* d_count, uint8_t* d_longest,
                                         int64_t* d_per_phrase) {
    const char* who = "tgx_corpus_phrase_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return phrase_hits(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, ps, stream, d_count, d_longest,
                       d_per_phrase);
}
