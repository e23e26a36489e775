// The C ABI's near-duplicate calls (include/tgx.h: tgx_result_minhash_device, tgx_corpus_minhash_device,
// tgx_minhash_bands_device, tgx_minhash_near_first_device, tgx_minhash_last_times): the argument checks, the scratch and
// the stages' times around the launchers of minhash.hip.  They run on the caller's stream under a StreamGuard, as the
// deduplication of result_ops.cpp does, and share device_internal.h with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "minhash.h"

using namespace tgx::host;
using namespace tgx::dev;

namespace {

// stage k of kMinhashStageNames: the signatures write 0, the bands 1 to 3, the clustering 4 and 5
const char* const kMinhashStageNames[tgx::kMinhashStages] = {"minhash_sig_kernel", "minhash_band_keys", "minhash_sort",
                                                            "minhash_heads",      "minhash_verify",    "minhash_roots"};
thread_local float g_minhash_ms[tgx::kMinhashStages] = {0, 0, 0, 0, 0, 0};

// Events at the boundaries of consecutive stretches of a stream's work, each stretch belonging to a stage: the bands'
// loop alternates sort and heads, and a stage's time is the sum of its stretches.  Declared before the guard.
class BoundaryTimer {
public:
    explicit BoundaryTimer(hipStream_t hs) : hs_(hs) {}
    BoundaryTimer(const BoundaryTimer&) = delete;
    BoundaryTimer& operator=(const BoundaryTimer&) = delete;
    ~BoundaryTimer() {
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    }
    // what was queued since the mark before belongs to `stage` (-1: to none)
    void mark(int stage) {
        hipEvent_t e = nullptr;
        if (!ok_ || hipEventCreate(&e) != hipSuccess || hipEventRecord(e, hs_) != hipSuccess) {
            if (e) (void)hipEventDestroy(e);
            ok_ = false;
            return;
        }
        ev_.push_back(e);
        stage_.push_back(stage);
    }
    void add_to(float* ms) const {  // after the stream has reached its end
        for (size_t k = 1; ok_ && k < ev_.size(); k++) {
            float t = 0;
            if (stage_[k] >= 0 && hipEventElapsedTime(&t, ev_[k - 1], ev_[k]) == hipSuccess) ms[stage_[k]] += t;
        }
    }

private:
    hipStream_t hs_;
    std::vector<hipEvent_t> ev_;
    std::vector<int> stage_;
    bool ok_ = true;
};

tgx_status minhash_check_perm(const char* who, uint32_t n_perm) {
    if (n_perm == 0 || n_perm > tgx::kMinhashMaxPerm) return fail(TGX_ERR_INVALID, "%s: n_perm %u is not in 1 .. %u", who, n_perm, tgx::kMinhashMaxPerm);
    return TGX_OK;
}

// The signatures of the rows of a result or of a corpus.  The handle, the flags and a device have been checked.
tgx_status minhash_signatures(const char* who, const tgx::DedupRows& rows, int device, uint32_t width, uint32_t n_perm, uint64_t seed, void* stream,
                              uint32_t* d_sig) {
    if (width == 0 || (uint64_t)width * rows.elem_bytes > tgx::kMinhashMaxBytes)
        return fail(TGX_ERR_INVALID, "%s: width %u of %u-byte elements is not in 1 .. %u", who, width, rows.elem_bytes, tgx::kMinhashMaxBytes / rows.elem_bytes);
    tgx_status st = minhash_check_perm(who, n_perm);
    if (st != TGX_OK) return st;
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (S == 0) {
        g_minhash_ms[0] = 0;
        return TGX_OK;
    }
    if (!d_sig) return fail(TGX_ERR_INVALID, "%s: d_sig is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_sig", d_sig, device, "source")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[1] = {0};
    StageTimer<1> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    size_t scan_bytes = 0;
    if (tgx::minhash_scan_bytes(S, &scan_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
    uint64_t* sh_offs = nullptr;
    void* scan_tmp = nullptr;
    if (guard.alloc((size_t)(S + 1) * 8, &sh_offs) != hipSuccess || guard.alloc(scan_bytes + 8, &scan_tmp) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (minhash)");
    }
    timer.begin(0);
    if (tgx::launch_minhash_sig(rows, width, n_perm, seed, sh_offs, scan_tmp, scan_bytes, d_sig, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "minhash_sig_kernel launch failed");
    timer.end(0);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    g_minhash_ms[0] = ms[0];
    return TGX_OK;
}

// what the two calls on signatures share before anything is queued
tgx_status minhash_check_sig(const char* who, int device, const uint32_t* d_sig, uint64_t n_rows, uint32_t n_perm) {
    int n_devices = 0;
    tgx_status st = require_device(&n_devices);
    if (st != TGX_OK) return st;
    if (device < 0 || device >= n_devices) return fail(TGX_ERR_INVALID, "%s: device %d of %d", who, device, n_devices);
    if ((st = minhash_check_perm(who, n_perm)) != TGX_OK) return st;
    if (n_rows >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    if (n_rows && !d_sig) return fail(TGX_ERR_INVALID, "%s: d_sig is NULL", who);
    return TGX_OK;
}

}  // namespace

int tgx_minhash_last_times(const char** names, float* ms, int cap) { return stage_times(kMinhashStageNames, g_minhash_ms, tgx::kMinhashStages, names, ms, cap); }

tgx_status tgx_result_minhash_device(const tgx_result* r, uint32_t width, uint32_t n_perm, uint64_t seed, uint32_t flags, void* stream, uint32_t* d_sig) {
    const char* who = "tgx_result_minhash_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!r) return fail(TGX_ERR_INVALID, "%s: result is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    return minhash_signatures(who, tgx::DedupRows{r->d_ids.get(), r->d_offs.get(), r->n_samples, r->n_tokens, 4}, r->device, width, n_perm, seed, stream,
                              d_sig);
}

tgx_status tgx_corpus_minhash_device(tgx_corpus* c, uint32_t width, uint32_t n_perm, uint64_t seed, uint32_t flags, void* stream, uint32_t* d_sig) {
    const char* who = "tgx_corpus_minhash_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return minhash_signatures(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, width, n_perm, seed, stream, d_sig);
}

// Keys in one kernel, row-major for the caller and band-major for the sorts; then per band a stable radix sort of
// (key, row) and the run rule, all bands through one scratch set.
tgx_status tgx_minhash_bands_device(int device, const uint32_t* d_sig, uint64_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed, void* stream,
                                    uint64_t* d_keys, int64_t* d_heads) {
    const char* who = "tgx_minhash_bands_device";
    tgx_status st = minhash_check_sig(who, device, d_sig, n_rows, n_perm);
    if (st != TGX_OK) return st;
    if (bands == 0 || n_perm % bands) return fail(TGX_ERR_INVALID, "%s: bands %u does not divide n_perm %u", who, bands, n_perm);
    if (!d_keys && !d_heads) return fail(TGX_ERR_INVALID, "%s: d_keys and d_heads are both NULL", who);
    const uint64_t S = n_rows;
    if (S == 0) {
        std::fill(g_minhash_ms + 1, g_minhash_ms + 4, 0.f);
        return TGX_OK;
    }
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_sig", d_sig, device, "call")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_keys", d_keys, device, "call")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_heads", d_heads, device, "call")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    BoundaryTimer timer(hs);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    tgx::DedupScratch s = {};
    uint64_t* keys_t = nullptr;
    if (d_heads) {
        if (tgx::dedup_temp_bytes(S, &s.scan_bytes, &s.sort_bytes, &s.select_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "%s: temp-size query failed", who);
        const bool got = guard.alloc((size_t)S * bands * 8, &keys_t) == hipSuccess && guard.alloc((size_t)S * 8, &s.keys_b) == hipSuccess &&
                         guard.alloc((size_t)S * 4, &s.rows_a) == hipSuccess && guard.alloc((size_t)S * 4, &s.rows_b) == hipSuccess &&
                         guard.alloc(s.sort_bytes + 8, &s.sort_tmp) == hipSuccess;  // (never NULL: that asks for the size)
        if (!got) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (minhash bands)");
        }
    }
    timer.mark(-1);
    if (tgx::launch_minhash_band_keys(d_sig, S, n_perm, bands, seed, d_keys, keys_t, hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "minhash_band_keys_kernel launch failed");
    timer.mark(1);
    if (d_heads) {
        if (tgx::launch_minhash_iota(s.rows_a, S, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "minhash_iota_kernel launch failed");
        timer.mark(2);
        for (uint32_t b = 0; b < bands; b++) {
            s.keys_a = keys_t + (uint64_t)b * S;  // (the sort reads its input only)
            if (tgx::launch_dedup_sort(s, S, 64, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "minhash sort launch failed");
            timer.mark(2);
            if (tgx::launch_minhash_heads(s.keys_b, s.rows_b, S, bands, b, d_heads, hs) != hipSuccess)
                return fail(TGX_ERR_DEVICE, "minhash_heads_kernel launch failed");
            timer.mark(3);
        }
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    std::fill(g_minhash_ms + 1, g_minhash_ms + 4, 0.f);
    timer.add_to(g_minhash_ms);
    return TGX_OK;
}

// first0 in one kernel, then rounds of pointer doubling between d_first and a scratch of its size; a round ends in the
// one host visit that reads whether anything moved.
tgx_status tgx_minhash_near_first_device(int device, const uint32_t* d_sig, uint64_t n_rows, uint32_t n_perm, const int64_t* d_heads, uint32_t bands,
                                         uint32_t min_agree, void* stream, int64_t* d_first, uint64_t* n_clusters) {
    const char* who = "tgx_minhash_near_first_device";
    if (n_clusters) *n_clusters = 0;
    tgx_status st = minhash_check_sig(who, device, d_sig, n_rows, n_perm);
    if (st != TGX_OK) return st;
    if (bands == 0 || bands > n_perm) return fail(TGX_ERR_INVALID, "%s: bands %u is not in 1 .. n_perm %u", who, bands, n_perm);
    if (min_agree == 0 || min_agree > n_perm) return fail(TGX_ERR_INVALID, "%s: min_agree %u is not in 1 .. n_perm %u", who, min_agree, n_perm);
    const uint64_t S = n_rows;
    if (S == 0) {
        g_minhash_ms[4] = g_minhash_ms[5] = 0;
        return TGX_OK;
    }
    if (!d_heads) return fail(TGX_ERR_INVALID, "%s: d_heads is NULL", who);
    if (!d_first) return fail(TGX_ERR_INVALID, "%s: d_first is NULL", who);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, "d_sig", d_sig, device, "call")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_heads", d_heads, device, "call")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, "d_first", d_first, device, "call")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    unsigned long long h_word = 0;  // (before the guard: a copy writes it)
    float round_ms[2] = {0, 0}, total_ms[2] = {0, 0};
    StageTimer<2> timer(hs, round_ms);
    StreamGuard guard(device, hs);
    int64_t* other = nullptr;
    unsigned long long* d_word = nullptr;
    if (guard.alloc((size_t)S * 8, &other) != hipSuccess || guard.alloc(sizeof(unsigned long long), &d_word) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_DEVICE, "out of device memory (minhash clusters)");
    }
    int64_t* buf[2] = {d_first, other};
    timer.begin(0);
    if (tgx::launch_minhash_verify(d_sig, S, n_perm, d_heads, bands, min_agree, buf[0], hs) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "minhash_verify_kernel launch failed");
    timer.end(0);
    int at = 0;  // the buffer that holds the chains so far
    for (uint32_t round = 0;; round++) {
        if (round > 64) {
            guard.done();
            return fail(TGX_ERR_DEVICE, "%s: the chains did not end", who);
        }
        timer.begin(1);
        if (tgx::launch_minhash_hop(buf[at], buf[at ^ 1], S, d_word, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "minhash_hop_kernel launch failed");
        timer.end(1);
        if ((st = read_u64(hs, d_word, &h_word)) != TGX_OK) return st;  // the round's host visit
        timer.read();
        if (round == 0) total_ms[0] = round_ms[0];  // (the verify ran once; every read gives its time again)
        total_ms[1] += round_ms[1];
        if (!h_word) break;  // nothing moved: buf[at] holds the roots, and so does the other
        at ^= 1;
    }
    timer.begin(1);
    if (buf[at] != d_first) HIP_TRY(hipMemcpyAsync(d_first, buf[at], (size_t)S * 8, hipMemcpyDeviceToDevice, hs));
    if (tgx::launch_minhash_count(d_first, S, d_word, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "minhash_count_kernel launch failed");
    timer.end(1);
    if ((st = read_u64(hs, d_word, &h_word)) != TGX_OK) return st;
    guard.done();
    timer.read();
    g_minhash_ms[4] = total_ms[0];
    g_minhash_ms[5] = total_ms[1] + round_ms[1];
    if (n_clusters) *n_clusters = h_word;
    return TGX_OK;
}
