// The C ABI's shared n-gram calls (include/tgx.h: tgx_result_gramset_create, tgx_corpus_gramset_create,
// tgx_gramset_create_from_keys, tgx_gramset_size / _info / _keys / _free, tgx_result_gram_hits_device,
// tgx_corpus_gram_hits_device, tgx_gram_last_times): the handle, the argument checks, the scratch and the stages' times
// around the launchers of gram.hip.  They run on the caller's stream under a StreamGuard, as the near-duplicate calls
// of minhash_ops.cpp do, and share device_internal.h with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "gram.h"

using namespace tgx::host;
using namespace tgx::dev;

// A gram set: the sorted distinct keys and the bucket directory over them, in pooled memory of its device.  Read-only
// after creation, so concurrent hit calls share it without a lock.
struct tgx_gramset {
    int device = 0;
    uint32_t width = 0, elem_bytes = 0, bits = 0;
    uint64_t seed = 0, n_keys = 0;
    PoolBuf<uint64_t> d_keys;  // u64[max(n_keys, 1)]
    PoolBuf<uint32_t> d_dir;   // u32[2^bits + 1]
};

namespace {

const char* const kGramStageNames[tgx::kGramStages] = {"gram_keys_kernel", "gram_sort", "gram_dir", "gram_hits_kernel"};
thread_local float g_gram_ms[tgx::kGramStages] = {0, 0, 0, 0};

tgx_status gram_check_width(const char* who, uint32_t width, uint32_t elem_bytes) {
    if (elem_bytes != 1 && elem_bytes != 4) return fail(TGX_ERR_INVALID, "%s: elem_bytes %u is neither 1 nor 4", who, elem_bytes);
    if (width == 0 || (uint64_t)width * elem_bytes > tgx::kMinhashMaxBytes)
        return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, width, elem_bytes, tgx::kMinhashMaxBytes / elem_bytes);
    return TGX_OK;
}

// From n_raw keys in d_raw (device memory of the guard, any order, duplicates allowed) to a set: the sort, the unique,
// the host visit that reads n_keys, the set's own buffers and the directory.  The timer's stages 1 and 2 are set here.
tgx_status gramset_finish(const char* who, StreamGuard& guard, StageTimer<3>& timer, hipStream_t hs, const uint64_t* d_raw, uint64_t n_raw,
                          unsigned long long* h_word, std::unique_ptr<tgx_gramset>& gs) {
    size_t sort_bytes = 0, unique_bytes = 0;
    if (tgx::gram_sort_bytes(n_raw, &sort_bytes, &unique_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    uint64_t *sorted = nullptr, *uniq = nullptr;
    unsigned long long* d_word = nullptr;
    void *sort_tmp = nullptr, *unique_tmp = nullptr;
    const size_t key_bytes = (size_t)std::max<uint64_t>(n_raw, 1) * 8;
    if (guard.alloc(key_bytes, &sorted) != hipSuccess || guard.alloc(key_bytes, &uniq) != hipSuccess ||
        guard.alloc(sizeof(unsigned long long), &d_word) != hipSuccess || guard.alloc(sort_bytes + 8, &sort_tmp) != hipSuccess ||
        guard.alloc(unique_bytes + 8, &unique_tmp) != hipSuccess) {  // (never NULL: that asks for the size)
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (gram set)");
    }
    timer.begin(1);
    if (tgx::launch_gram_sort_unique(d_raw, sorted, uniq, d_word, n_raw, sort_tmp, sort_bytes, unique_tmp, unique_bytes, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "%s: sort launch failed", who);
    timer.end(1);
    tgx_status st = read_u64(hs, d_word, h_word);  // the host visit for n_keys
    if (st != TGX_OK) return st;
    const uint64_t n_keys = *h_word;
    if (n_keys > tgx::kGramMaxKeys) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-2 keys", who);
    gs->n_keys = n_keys;
    gs->bits = tgx::gram_dir_bits(n_keys);
    if (gs->d_keys.alloc(gs->device, (size_t)std::max<uint64_t>(n_keys, 1) * 8) != hipSuccess ||
        gs->d_dir.alloc(gs->device, (((size_t)1 << gs->bits) + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (gram set)");
    }
    if (n_keys) HIP_TRY(hipMemcpyAsync(gs->d_keys.get(), uniq, (size_t)n_keys * 8, hipMemcpyDeviceToDevice, hs));
    timer.begin(2);
    if (tgx::launch_gram_dir(gs->d_keys.get(), n_keys, gs->bits, gs->d_dir.get(), hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "gram_dir_kernel launch failed");
    timer.end(2);
    HIP_TRY(hipStreamSynchronize(hs));
    return TGX_OK;
}

// The set of the rows of a result or of a corpus.  The handle, the flags and a device have been checked.
tgx_status gramset_of_rows(const char* who, const tgx::DedupRows& rows, int device, uint32_t width, uint64_t seed, void* stream, tgx_gramset** out) {
    tgx_status st = gram_check_width(who, width, rows.elem_bytes);
    if (st != TGX_OK) return st;
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    hipStream_t hs = stream_or_default(stream, device);
    std::unique_ptr<tgx_gramset> gs(new tgx_gramset());  // (before the guard, as the host words: queued work writes them)
    gs->device = device;
    gs->width = width;
    gs->elem_bytes = rows.elem_bytes;
    gs->seed = seed;
    unsigned long long h_word = 0;
    float ms[3] = {0, 0, 0};
    StageTimer<3> timer(hs, ms);
    StreamGuard guard(device, hs);
    uint64_t n_grams = 0;
    uint64_t* raw = nullptr;
    if (S) {
        size_t scan_bytes = 0;
        if (tgx::gram_scan_bytes(S, &scan_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
        uint64_t* g_offs = nullptr;
        void* scan_tmp = nullptr;
        if (guard.alloc((size_t)(S + 1) * 8, &g_offs) != hipSuccess || guard.alloc(scan_bytes + 8, &scan_tmp) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (gram set)");
        }
        timer.begin(0);
        if (tgx::launch_gram_offsets(rows, width, g_offs, scan_tmp, scan_bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: scan launch failed", who);
        // the grams' total sizes the sort: a host visit of its own, before the one for n_keys
        if ((st = read_u64(hs, g_offs + S, &h_word)) != TGX_OK) return st;
        n_grams = h_word;
        if (n_grams) {
            if (guard.alloc((size_t)n_grams * 8, &raw) != hipSuccess) {
                (void)hipGetLastError();
                return fail(TGX_ERR_DEVICE, "out of device memory (gram set)");
            }
            if (tgx::launch_gram_keys(rows, width, seed, g_offs, raw, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "gram_keys_kernel launch failed");
        }
        timer.end(0);
    }
    if ((st = gramset_finish(who, guard, timer, hs, raw, n_grams, &h_word, gs)) != TGX_OK) return st;
    guard.done();
    timer.read();
    std::copy(ms, ms + 3, g_gram_ms);
    *out = gs.release();
    return TGX_OK;
}

// count and mask of the rows of a result or of a corpus against a set.  The handle, the flags and a device have been checked.
tgx_status gram_hits(const char* who, const tgx::DedupRows& rows, int device, const tgx_gramset* gs, void* stream, int64_t* d_count, uint8_t* d_mask) {
    if (!gs) return fail(TGX_ERR_INVALID, "%s: gram set is NULL", who);
    if (gs->elem_bytes != rows.elem_bytes)
        return fail(TGX_ERR_INVALID, "%s: the set holds grams of %u-byte elements, the source has %u-byte elements", who, gs->elem_bytes, rows.elem_bytes);
    if (gs->device != device) return fail(TGX_ERR_INVALID, "%s: the set is on device %d, the source on device %d", who, gs->device, device);
    tgx_status st = gram_check_width(who, gs->width, rows.elem_bytes);
    if (st != TGX_OK) return st;
    if (!d_count && !d_mask) return fail(TGX_ERR_INVALID, "%s: d_count and d_mask are both NULL", who);
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        g_gram_ms[3] = 0;
        return TGX_OK;
    }
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_count", d_count, device, "source")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_mask", d_mask, device, "source")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[1] = {0};
    StageTimer<1> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    timer.begin(0);
    if (tgx::launch_gram_hits(rows, gs->width, gs->seed, gs->d_keys.get(), gs->d_dir.get(), gs->bits, d_count, d_mask, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "gram_hits_kernel launch failed");
    timer.end(0);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    g_gram_ms[3] = ms[0];
    return TGX_OK;
}

}  // namespace

int tgx_gram_last_times(const char** names, float* ms, int cap) { return stage_times(kGramStageNames, g_gram_ms, tgx::kGramStages, names, ms, cap); }

tgx_status tgx_result_gramset_create(const tgx_result* r, uint32_t width, uint64_t seed, uint32_t flags, void* stream, tgx_gramset** out) {
    const char* who = "tgx_result_gramset_create";
    if (out) *out = nullptr;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r || !out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, r ? "out" : "result");
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return gramset_of_rows(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, width, seed, stream, out);
}

tgx_status tgx_corpus_gramset_create(tgx_corpus* c, uint32_t width, uint64_t seed, uint32_t flags, void* stream, tgx_gramset** out) {
    const char* who = "tgx_corpus_gramset_create";
    if (out) *out = nullptr;
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !out) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "out" : "corpus");
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return gramset_of_rows(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, width, seed, stream, out);
}

tgx_status tgx_gramset_create_from_keys(int device, const uint64_t* keys, uint64_t n, uint32_t width, uint32_t elem_bytes, uint64_t seed,
                                        tgx_gramset** out) {
    const char* who = "tgx_gramset_create_from_keys";
    if (out) *out = nullptr;
    int n_devices = 0;
    tgx_status st = require_device(&n_devices);
    if (st != TGX_OK) return st;
    if (!out) return fail(TGX_ERR_INVALID, "%s: out is NULL", who);
    if (device < 0 || device >= n_devices) return fail(TGX_ERR_INVALID, "%s: device %d of %d", who, device, n_devices);
    if ((st = gram_check_width(who, width, elem_bytes)) != TGX_OK) return st;
    if (n && !keys) return fail(TGX_ERR_INVALID, "%s: keys is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    hipStream_t hs = stream_or_default(nullptr, device);
    std::unique_ptr<tgx_gramset> gs(new tgx_gramset());
    gs->device = device;
    gs->width = width;
    gs->elem_bytes = elem_bytes;
    gs->seed = seed;
    unsigned long long h_word = 0;
    float ms[3] = {0, 0, 0};
    StageTimer<3> timer(hs, ms);
    StreamGuard guard(device, hs);
    uint64_t* raw = nullptr;
    if (n) {
        if (guard.alloc((size_t)n * 8, &raw) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (gram set)");
        }
        HIP_TRY(hipMemcpyAsync(raw, keys, (size_t)n * 8, hipMemcpyHostToDevice, hs));  // (the caller's keys live past the call's end)
    }
    if ((st = gramset_finish(who, guard, timer, hs, raw, n, &h_word, gs)) != TGX_OK) return st;
    guard.done();
    timer.read();
    std::copy(ms, ms + 3, g_gram_ms);
    *out = gs.release();
    return TGX_OK;
}

uint64_t tgx_gramset_size(const tgx_gramset* gs) { return gs ? gs->n_keys : 0; }

tgx_status tgx_gramset_info(const tgx_gramset* gs, uint32_t* width, uint32_t* elem_bytes, uint64_t* seed, int* device, uint32_t* dir_bits) {
    if (!gs) return fail(TGX_ERR_INVALID, "tgx_gramset_info: gram set is NULL");
    if (width) *width = gs->width;
    if (elem_bytes) *elem_bytes = gs->elem_bytes;
    if (seed) *seed = gs->seed;
    if (device) *device = gs->device;
    if (dir_bits) *dir_bits = gs->bits;
    return TGX_OK;
}

tgx_status tgx_gramset_keys(const tgx_gramset* gs, uint64_t* keys_out) {
    const char* who = "tgx_gramset_keys";
    if (!gs) return fail(TGX_ERR_INVALID, "%s: gram set is NULL", who);
    if (gs->n_keys == 0) return TGX_OK;
    if (!keys_out) return fail(TGX_ERR_INVALID, "%s: keys_out is NULL", who);
    if (copy_sync(keys_out, gs->d_keys.get(), (size_t)gs->n_keys * 8, hipMemcpyDeviceToHost, gs->device) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "%s: the copy failed", who);
    return TGX_OK;
}

void tgx_gramset_free(tgx_gramset* gs) { delete gs; }

tgx_status tgx_result_gram_hits_device(const tgx_result* r, const tgx_gramset* gs, uint32_t flags, void* stream, int64_t* d_count, uint8_t* d_mask) {
    const char* who = "tgx_result_gram_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return gram_hits(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, gs, stream, d_count, d_mask);
}

tgx_status tgx_corpus_gram_hits_device(tgx_corpus* c, const tgx_gramset* gs, uint32_t flags, void* stream, int64_t* d_count, uint8_t* d_mask) {
    const char* who = "tgx_corpus_gram_hits_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return gram_hits(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, gs, stream, d_count, d_mask);
}
