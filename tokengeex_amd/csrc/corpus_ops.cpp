// The C ABI's transforms of a resident corpus (include/tgx.h): its read-backs, a corpus from decoded text, the front end
// (special-token split and CRLF), Unicode normalisation, row selection, row deduplication, and the split plan's handle.  They run on a stream of their own
// under a StreamGuard and share device_internal.h with the passes (tgx_api.cpp, encode_pass.cpp, estep_pass.cpp, lattice_pass.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "dedup.h"
#include "front.h"
#include "kernels.h"
#include "norm.h"
#include "select.h"

using namespace tgx::host;
using namespace tgx::dev;

// ---- read-backs; a corpus over a decoded text ----------------------------------------------------------------------

tgx_status tgx_corpus_copy_text(const tgx_corpus* c, uint8_t* dst, uint64_t cap) {
    if (!c || (!dst && c->n_bytes)) return fail(TGX_ERR_INVALID, "tgx_corpus_copy_text: NULL argument");
    if (cap < c->n_bytes) return fail(TGX_ERR_INVALID, "tgx_corpus_copy_text: %llu bytes, room for %llu", (unsigned long long)c->n_bytes, (unsigned long long)cap);
    if (!c->n_bytes) return TGX_OK;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(copy_sync(dst, c->d_text, c->n_bytes, hipMemcpyDeviceToHost, c->device));
    return TGX_OK;
}

tgx_status tgx_corpus_copy_offsets(const tgx_corpus* c, uint64_t* dst, uint64_t cap) {
    if (!c || !dst) return fail(TGX_ERR_INVALID, "tgx_corpus_copy_offsets: NULL argument");
    if (cap < c->n_samples + 1) return fail(TGX_ERR_INVALID, "tgx_corpus_copy_offsets: %llu offsets, room for %llu", (unsigned long long)(c->n_samples + 1), (unsigned long long)cap);
    memcpy(dst, c->h_offs.data(), (size_t)(c->n_samples + 1) * 8);  // (the corpus keeps them on the host too)
    return TGX_OK;
}

tgx_status tgx_corpus_from_text(const tgx_text* t, tgx_corpus** out) {
    const char* who = "tgx_corpus_from_text";
    if (!t || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    std::vector<uint64_t> offs(t->n_rows + 1);
    const tgx_status st = tgx_text_copy_offsets(t, offs.data(), offs.size());
    if (st != TGX_OK) return st;
    DeviceScope scope;
    return corpus_create(who, t->device, t->d_bytes, TextFrom::Device, offs.data(), t->n_rows, out);
}

// ---- the front end on the device: a resident corpus split at special tokens, CRLF applied (front.hip; front.h) ----

namespace {

// device time of the last tgx_corpus_split_specials of this thread, per stage (tgx_front_last_times)
constexpr int kFrontStages = 5;
const char* const kFrontStageNames[kFrontStages] = {"front_mark", "front_resolve", "front_segments", "front_keep", "front_pack"};
thread_local float g_front_ms[kFrontStages] = {0, 0, 0, 0, 0};

}  // namespace

int tgx_front_last_times(const char** names, float* ms, int cap) { return stage_times(kFrontStageNames, g_front_ms, kFrontStages, names, ms, cap); }

tgx_status tgx_corpus_split_specials(tgx_corpus* c, const uint8_t* special_bytes, const uint64_t* special_offs, uint32_t n_specials, uint32_t flags,
                                     tgx_corpus** segs, tgx_plan** plan) {
    const char* who = "tgx_corpus_split_specials";
    if (!c || !segs || !plan) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *segs = nullptr;
    *plan = nullptr;
    tgx_status st = layout_check_flags(who, flags, TGX_FRONT_CRLF);
    FrontHostTables ht;
    if (st == TGX_OK) st = front_build_tables(who, special_bytes, special_offs, n_specials, &ht);
    if (st == TGX_OK) st = require_device();
    if (st != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    DeviceScope scope;
    const int dev = c->device;
    HIP_TRY(hipSetDevice(dev));
    hipStream_t hs = stream_or_default(nullptr, dev);
    const uint64_t S = c->n_samples, N = c->n_bytes;
    std::unique_ptr<tgx_plan> pl(new tgx_plan());
    std::unique_ptr<tgx_corpus> out;  // the segments' corpus
    std::vector<uint64_t> h_out_offs(1, 0);
    unsigned long long h_count = 0;
    StreamGuard guard(dev, hs);  // destroyed before them: a failed call's queued work is over before they go
    StageTimer<kFrontStages> timer(hs, g_front_ms);
    pl->device = dev;
    pl->n_samples = S;
    pl->n_specials = n_specials;
    HIP_TRY(pl->d_seg_offs.alloc(dev, (size_t)(S + 1) * 8));
    if (S == 0 || N == 0) {  // no segments
        HIP_TRY(pl->d_special.alloc(dev, 4));
        HIP_TRY(hipMemsetAsync(pl->d_seg_offs, 0, (size_t)(S + 1) * 8, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        tgx_corpus* empty = nullptr;
        if ((st = corpus_create(who, dev, nullptr, TextFrom::Caller, nullptr, 0, &empty)) != TGX_OK) return st;
        guard.done();
        *segs = empty;
        *plan = pl.release();
        return TGX_OK;
    }

    tgx::FrontParams p = {};
    p.text = c->d_text;
    p.offs = c->d_offs;
    p.n_bytes = N;
    p.n_samples = S;
    p.crlf = (flags & TGX_FRONT_CRLF) ? 1u : 0u;
    const uint64_t tiles = (N + tgx::kFrontTile - 1) / tgx::kFrontTile, slots = (N + tgx::kFrontGroup - 1) / tgx::kFrontGroup;
    // the special tokens' tables
    uint32_t *d_mask = nullptr, *d_first = nullptr, *d_by_first = nullptr, *d_sp_offs = nullptr;
    uint8_t* d_sp_bytes = nullptr;
    HIP_TRY(guard.alloc(32, &d_mask));
    HIP_TRY(guard.alloc(257 * 4, &d_first));
    HIP_TRY(guard.alloc((size_t)n_specials * 4 + 4, &d_by_first));
    HIP_TRY(guard.alloc((size_t)n_specials * 4 + 4, &d_sp_offs));
    HIP_TRY(guard.alloc(ht.sp_bytes.size() + 16, &d_sp_bytes));
    HIP_TRY(hipMemcpyAsync(d_mask, ht.first_mask.data(), 32, hipMemcpyHostToDevice, hs));
    HIP_TRY(hipMemcpyAsync(d_first, ht.first_start.data(), 257 * 4, hipMemcpyHostToDevice, hs));
    if (n_specials) HIP_TRY(hipMemcpyAsync(d_by_first, ht.by_first.data(), (size_t)n_specials * 4, hipMemcpyHostToDevice, hs));
    HIP_TRY(hipMemcpyAsync(d_sp_offs, ht.sp_offs.data(), ((size_t)n_specials + 1) * 4, hipMemcpyHostToDevice, hs));
    if (!ht.sp_bytes.empty()) HIP_TRY(hipMemcpyAsync(d_sp_bytes, ht.sp_bytes.data(), ht.sp_bytes.size(), hipMemcpyHostToDevice, hs));
    p.tab = front_tables(ht, d_mask, d_first, d_by_first, d_sp_offs, d_sp_bytes);
    // every scan's scratch, asked for again when a later count is larger than the ones known so far
    ScanScratch scan;

    // mark
    HIP_TRY(guard.alloc((size_t)slots * 2, &p.hit_mask));
    HIP_TRY(guard.alloc((size_t)slots * 2, &p.crlf_mask));
    HIP_TRY(guard.alloc((size_t)slots * 2, &p.keep_mask));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_count));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_base));
    if ((st = scan_room(&scan, guard, tgx::front_scan_temp_bytes, std::max(tiles, S) + 1)) != TGX_OK) return st;
    timer.begin(0);
    HIP_TRY(tgx::launch_front_mark(p, scan.ptr, scan.bytes, hs));
    timer.end(0);
    if ((st = read_u64(hs, p.tile_base + tiles, &h_count)) != TGX_OK) return st;
    const uint64_t C = h_count;
    // candidates, resolve, the samples' segment counts
    p.n_cand = C;
    HIP_TRY(guard.alloc((size_t)C * 8, &p.cand_pos));
    HIP_TRY(guard.alloc((size_t)C * 8, &p.cand_end));
    HIP_TRY(guard.alloc((size_t)C * 8, &p.pm));
    HIP_TRY(guard.alloc((size_t)C * 8, &p.acc_end));
    HIP_TRY(guard.alloc((size_t)C * 8, &p.la));
    HIP_TRY(guard.alloc((size_t)(C + 1) * 8, &p.seg_sum));
    HIP_TRY(guard.alloc((size_t)C * 4, &p.cand_special));
    HIP_TRY(guard.alloc((size_t)C * 4, &p.cand_sample));
    HIP_TRY(guard.alloc((size_t)(C + 1) * 4, &p.cand_segs));
    HIP_TRY(guard.alloc((size_t)(S + 1) * 8, &p.first));
    HIP_TRY(guard.alloc((size_t)(S + 1) * 8, &p.sample_segs));
    p.seg_offs = pl->d_seg_offs;
    if ((st = scan_room(&scan, guard, tgx::front_scan_temp_bytes, C + 1)) != TGX_OK) return st;
    timer.begin(1);
    HIP_TRY(tgx::launch_front_candidates(p, scan.ptr, scan.bytes, hs));
    timer.end(1);
    if ((st = read_u64(hs, p.seg_offs + S, &h_count)) != TGX_OK) return st;
    const uint64_t K = h_count;
    // segments
    p.n_segs = K;
    HIP_TRY(pl->d_special.alloc(dev, (size_t)(K + 1) * 4));
    p.seg_special = pl->d_special;
    HIP_TRY(guard.alloc((size_t)K * 8, &p.seg_begin));
    HIP_TRY(guard.alloc((size_t)K * 8, &p.seg_end));
    HIP_TRY(guard.alloc((size_t)(K + 1) * 8, &p.rank));
    if ((st = scan_room(&scan, guard, tgx::front_scan_temp_bytes, K + 1)) != TGX_OK) return st;
    timer.begin(2);
    HIP_TRY(tgx::launch_front_segments(p, scan.ptr, scan.bytes, hs));
    timer.end(2);
    if ((st = read_u64(hs, p.rank + K, &h_count)) != TGX_OK) return st;
    const uint64_t E = h_count;
    pl->n_segs = K;
    pl->n_enc = E;
    // keep and pack: the E + 1 offsets visit the host for the corpus's longest-first order
    p.n_enc = E;
    tgx_corpus* made = nullptr;
    if (E) {
        HIP_TRY(guard.alloc((size_t)E * 8, &p.enc_begin));
        HIP_TRY(guard.alloc((size_t)E * 8, &p.enc_end));
        HIP_TRY(guard.alloc((size_t)E * 4, &p.enc_local));
        HIP_TRY(guard.alloc((size_t)(E + 1) * 8, &p.out_offs));
        timer.begin(3);
        HIP_TRY(tgx::launch_front_keep(p, scan.ptr, scan.bytes, hs));
        timer.end(3);
        h_out_offs.resize(E + 1);
        HIP_TRY(hipMemcpyAsync(h_out_offs.data(), p.out_offs, (size_t)(E + 1) * 8, hipMemcpyDeviceToHost, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        if ((st = corpus_create(who, dev, nullptr, TextFrom::Caller, h_out_offs.data(), E, &made)) != TGX_OK) return st;
        out.reset(made);
        p.out = out->d_text;
        timer.begin(4);
        if (out->n_bytes) HIP_TRY(tgx::launch_front_pack(p, hs));
        timer.end(4);
    } else {
        if ((st = corpus_create(who, dev, nullptr, TextFrom::Caller, nullptr, 0, &made)) != TGX_OK) return st;
        out.reset(made);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    *segs = out.release();
    *plan = pl.release();
    return TGX_OK;
}

// ---- Unicode normalisation on the device (norm.hip; norm.h) -------------------------------------------------------

namespace {

// device time of the last tgx_corpus_normalize of this thread, per stage (tgx_norm_last_times)
constexpr int kNormStages = 5;
const char* const kNormStageNames[kNormStages] = {"norm_mark", "norm_pieces", "norm_length", "norm_places", "norm_write"};
thread_local float g_norm_ms[kNormStages] = {0, 0, 0, 0, 0};

// the normaliser's tables on a device: uploaded by the first call that needs them there and kept for the process
std::mutex g_norm_mu;
struct NormDeviceTables {
    bool ready = false;
    tgx::NormTables tab = {};
} g_norm_dev[64];

tgx_status norm_device_tables(int dev, tgx::NormTables* out) {
    if (dev < 0 || dev >= 64) return fail(TGX_ERR_INVALID, "device %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_norm_mu);
    NormDeviceTables& d = g_norm_dev[dev];
    if (!d.ready) {
        const NormHostTables& h = norm_host_tables();
        const tgx::NormTables& t = norm_tables_on_host();
        const void* src[15] = {t.stage1,    t.stage2,     t.ccc_cp,     t.ccc_val,    t.canon_cp,   t.canon_off,   t.canon_seq,      t.canon_len,
                               t.compat_cp, t.compat_off, t.compat_seq, t.compat_len, t.pair_first, t.pair_second, t.pair_composite};
        const size_t bytes[15] = {h.stage1.size() * 2, h.stage2.size(),    h.ccc_cp_bytes,    h.ccc_val_bytes,   h.canon_cp_bytes,
                                  h.canon_off_bytes,   h.canon_seq_bytes,  h.canon_len_bytes, h.compat_cp_bytes, h.compat_off_bytes,
                                  h.compat_seq_bytes,  h.compat_len_bytes, h.pair_bytes,      h.pair_bytes,      h.pair_bytes};
        size_t at[15], total = 0;
        for (int k = 0; k < 15; k++) {
            at[k] = total;
            total += (bytes[k] + 255) & ~(size_t)255;
        }
        uint8_t* base = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&base), total));
        for (int k = 0; k < 15; k++) {
            const hipError_t e = hipMemcpy(base + at[k], src[k], bytes[k], hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(base);
                HIP_TRY(e);
            }
        }
        auto u32 = [&](int k) { return reinterpret_cast<const uint32_t*>(base + at[k]); };
        d.tab = t;
        d.tab.stage1 = reinterpret_cast<const uint16_t*>(base + at[0]);
        d.tab.stage2 = base + at[1];
        d.tab.ccc_cp = u32(2);
        d.tab.ccc_val = base + at[3];
        d.tab.canon_cp = u32(4);
        d.tab.canon_off = u32(5);
        d.tab.canon_seq = u32(6);
        d.tab.canon_len = base + at[7];
        d.tab.compat_cp = u32(8);
        d.tab.compat_off = u32(9);
        d.tab.compat_seq = u32(10);
        d.tab.compat_len = base + at[11];
        d.tab.pair_first = u32(12);
        d.tab.pair_second = u32(13);
        d.tab.pair_composite = u32(14);
        d.ready = true;
    }
    *out = d.tab;
    return TGX_OK;
}

}  // namespace

int tgx_norm_last_times(const char** names, float* ms, int cap) { return stage_times(kNormStageNames, g_norm_ms, kNormStages, names, ms, cap); }

tgx_status tgx_corpus_normalize(tgx_corpus* c, uint32_t form, tgx_corpus** out, uint64_t* n_pieces) {
    const char* who = "tgx_corpus_normalize";
    if (!c || !out || !n_pieces) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    *n_pieces = 0;
    if (form > 3) return fail(TGX_ERR_INVALID, "%s: form must be 0 (NFD), 1 (NFC), 2 (NFKD) or 3 (NFKC)", who);
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    DeviceScope scope;
    const int dev = c->device;
    HIP_TRY(hipSetDevice(dev));
    hipStream_t hs = stream_or_default(nullptr, dev);
    const uint64_t S = c->n_samples, N = c->n_bytes;
    std::unique_ptr<tgx_corpus> made_owner;  // the new corpus
    std::vector<uint64_t> h_out_offs;
    unsigned long long h_count = 0;
    StreamGuard guard(dev, hs);  // destroyed before them: a failed call's queued work is over before they go
    StageTimer<kNormStages> timer(hs, g_norm_ms);
    tgx_corpus* made = nullptr;
    auto copy_of_c = [&]() -> tgx_status {  // no piece: the same rows, device to device
        if ((st = corpus_create(who, dev, c->d_text, TextFrom::Device, S ? c->h_offs.data() : nullptr, S, &made)) != TGX_OK) return st;
        guard.done();
        timer.read();
        *out = made;
        return TGX_OK;
    };
    if (S == 0 || N == 0) return copy_of_c();

    tgx::NormParams p = {};
    p.text = c->d_text;
    p.offs = c->d_offs;
    p.n_bytes = N;
    p.n_rows = S;
    p.form = form;
    if ((st = norm_device_tables(dev, &p.tab)) != TGX_OK) return st;
    const uint64_t tiles = (N + tgx::kFrontTile - 1) / tgx::kFrontTile, slots = (N + tgx::kFrontGroup - 1) / tgx::kFrontGroup;
    ScanScratch scan;
    // mark
    HIP_TRY(guard.alloc((size_t)slots * 4, &p.mask));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_count));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_base));
    if ((st = scan_room(&scan, guard, tgx::norm_scan_temp_bytes, tiles + 1)) != TGX_OK) return st;
    timer.begin(0);
    HIP_TRY(tgx::launch_norm_mark(p, scan.ptr, scan.bytes, hs));
    timer.end(0);
    if ((st = read_u64(hs, p.tile_base + tiles, &h_count)) != TGX_OK) return st;
    const uint64_t P = h_count;
    if (P == 0) return copy_of_c();
    // pieces, their lengths
    p.n_pieces = P;
    HIP_TRY(guard.alloc((size_t)P * 8, &p.piece_begin));
    HIP_TRY(guard.alloc((size_t)P * 8, &p.piece_row));
    HIP_TRY(guard.alloc((size_t)(P + 1) * 8, &p.piece_len));
    HIP_TRY(guard.alloc((size_t)(P + 1) * 8, &p.piece_sum));
    HIP_TRY(guard.alloc(8, &p.overflow_row));
    if ((st = scan_room(&scan, guard, tgx::norm_scan_temp_bytes, P + 1)) != TGX_OK) return st;
    timer.begin(1);
    HIP_TRY(tgx::launch_norm_pieces(p, hs));
    timer.end(1);
    timer.begin(2);
    HIP_TRY(tgx::launch_norm_length(p, scan.ptr, scan.bytes, hs));
    timer.end(2);
    if ((st = read_u64(hs, p.overflow_row, &h_count)) != TGX_OK) return st;
    const uint64_t overflow_row = h_count;
    if (overflow_row != tgx::kNormNoRow) {
        guard.done();  // (the stream has reached its end)
        return norm_overflow(who, overflow_row);
    }
    // places: the S + 1 offsets visit the host for the corpus's longest-first order
    HIP_TRY(guard.alloc((size_t)slots * 4, &p.slot_pre));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_bytes));
    HIP_TRY(guard.alloc((size_t)(tiles + 1) * 8, &p.tile_place));
    HIP_TRY(guard.alloc((size_t)(S + 1) * 8, &p.out_offs));
    timer.begin(3);
    HIP_TRY(tgx::launch_norm_places(p, scan.ptr, scan.bytes, hs));
    timer.end(3);
    h_out_offs.resize(S + 1);
    HIP_TRY(hipMemcpyAsync(h_out_offs.data(), p.out_offs, (size_t)(S + 1) * 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    if ((st = corpus_create(who, dev, nullptr, TextFrom::Caller, h_out_offs.data(), S, &made)) != TGX_OK) return st;
    made_owner.reset(made);
    p.out = made->d_text;
    timer.begin(4);
    HIP_TRY(tgx::launch_norm_write(p, hs));
    timer.end(4);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    *out = made_owner.release();
    *n_pieces = P;
    return TGX_OK;
}

// ---- row selection: samples of a corpus through an index (select.hip; select.h; result_ops.cpp has the shared steps) ----

tgx_status tgx_corpus_select(tgx_corpus* c, const int64_t* rows, uint64_t n_select, uint32_t flags, void* stream, tgx_corpus** out) {
    const char* who = "tgx_corpus_select";
    if (!c || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (n_select && !rows) return fail(TGX_ERR_INVALID, "%s: rows is NULL", who);
    tgx_status st = layout_check_flags(who, flags, TGX_SELECT_ROWS_DEVICE);
    if (st != TGX_OK) return st;
    const uint64_t M = n_select;
    if (M >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 samples", who);
    const bool on_device = (flags & TGX_SELECT_ROWS_DEVICE) != 0;
    std::lock_guard<std::mutex> lkc(c->mu);
    const uint64_t S = c->n_samples;
    std::vector<uint64_t> h_out_offs(M + 1, 0);
    if (!on_device) {  // before any device call: the check, and the new offsets from the corpus's host copy
        if ((st = select_check_rows(who, rows, M, S)) != TGX_OK) return st;
        for (uint64_t k = 0; k < M; k++) h_out_offs[k + 1] = h_out_offs[k] + tgx::select_out_len(c->h_offs.data(), S, rows, k);
    }
    if ((st = require_device()) != TGX_OK) return st;
    DeviceScope scope;
    const int dev = c->device;
    HIP_TRY(hipSetDevice(dev));
    hipStream_t hs = stream_or_default(stream, dev);
    std::unique_ptr<tgx_corpus> made_owner;  // the new corpus
    unsigned long long h_bad = tgx::kSelectNoBad;
    StageTimer<kSelectStages> timer(hs, select_stage_ms());  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(dev, hs);  // destroyed before them: a failed call's queued work is over before they go
    tgx::SelectParams p = {};
    if ((st = select_rows_device(who, rows, M, flags, dev, guard, &p.rows)) != TGX_OK) return st;
    p.data = c->d_text;
    p.offs = c->d_offs;
    p.n_src = S;
    p.n_rows = M;
    if (on_device && M) {  // the device's check and scan; the M + 1 offsets visit the host, which corpus_create needs anyway
        ScanScratch scan;
        unsigned long long* d_bad = nullptr;
        if ((st = scan_room(&scan, guard, tgx::select_scan_temp_bytes, M)) != TGX_OK) return st;
        HIP_TRY(guard.alloc(sizeof(unsigned long long), &d_bad));
        HIP_TRY(guard.alloc((size_t)(M + 1) * 8, &p.out_offs));
        HIP_TRY(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), hs));
        timer.begin(0);
        if (tgx::launch_select_check(p, d_bad, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "select_check_kernel launch failed");
        timer.end(0);
        timer.begin(1);
        if (tgx::launch_select_offsets(p, scan.ptr, scan.bytes, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan launch failed");
        timer.end(1);
        HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, hs));
        if ((st = read_u64(hs, p.out_offs, h_out_offs.data(), (size_t)(M + 1))) != TGX_OK) return st;
        if ((st = select_bad_index(who, h_bad, p.rows, S, hs)) != TGX_OK) {
            guard.done();  // (the stream has reached its end)
            return st;
        }
    }
    tgx_corpus* made = nullptr;
    if ((st = corpus_create(who, dev, nullptr, TextFrom::Caller, M ? h_out_offs.data() : nullptr, M, &made)) != TGX_OK) return st;
    made_owner.reset(made);
    p.out_offs = made->d_offs;  // (the same offsets, now the new corpus's own)
    p.n_out = made->n_bytes;
    p.out = made->d_text;
    timer.begin(2);
    if (tgx::launch_select_fill_text(p, hs) != hipSuccess) return fail(TGX_ERR_DEVICE, "select_fill_kernel launch failed");
    timer.end(2);
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    *out = made_owner.release();
    return TGX_OK;
}

// ---- exact row deduplication: samples of a corpus (dedup.hip; dedup.h; result_ops.cpp has the rounds) ------------------

tgx_status tgx_corpus_first_equal_device(tgx_corpus* c, uint32_t flags, void* stream, int64_t* d_first, uint64_t* n_unique) {
    const char* who = "tgx_corpus_first_equal_device";
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    if ((st = layout_check_flags(who, flags, 0)) != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return dedup_first_equal(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, stream, d_first, n_unique);
}

tgx_status tgx_corpus_row_hashes_device(tgx_corpus* c, uint64_t seed, void* stream, uint64_t* d_hashes) {
    const char* who = "tgx_corpus_row_hashes_device";
    const tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c) return fail(TGX_ERR_INVALID, "%s: corpus is NULL", who);
    std::lock_guard<std::mutex> lkc(c->mu);
    return dedup_row_hashes(who, tgx::DedupRows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1}, c->device, seed, stream, d_hashes);
}

// ---- the split plan (tgx_corpus_split_specials makes it, tgx_assemble_result_plan reads it) ------------------------

uint64_t tgx_plan_num_samples(const tgx_plan* p) { return p ? p->n_samples : 0; }
uint64_t tgx_plan_num_segments(const tgx_plan* p) { return p ? p->n_segs : 0; }
uint64_t tgx_plan_num_encoded(const tgx_plan* p) { return p ? p->n_enc : 0; }
int tgx_plan_device(const tgx_plan* p) { return p ? p->device : -1; }
// (the call that made it returned after its stream had reached its end: the buffers go straight back to the pool)
void tgx_plan_free(tgx_plan* p) { delete p; }

tgx_status tgx_plan_copy(const tgx_plan* p, uint64_t* seg_offs, uint64_t offs_cap, int32_t* seg_special, uint64_t special_cap) {
    const char* who = "tgx_plan_copy";
    if (!p || !seg_offs || (!seg_special && p->n_segs)) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    if (offs_cap < p->n_samples + 1) return fail(TGX_ERR_INVALID, "%s: %llu offsets, room for %llu", who, (unsigned long long)(p->n_samples + 1), (unsigned long long)offs_cap);
    if (special_cap < p->n_segs) return fail(TGX_ERR_INVALID, "%s: %llu segments, room for %llu", who, (unsigned long long)p->n_segs, (unsigned long long)special_cap);
    DeviceScope scope;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(copy_sync(seg_offs, p->d_seg_offs, (size_t)(p->n_samples + 1) * 8, hipMemcpyDeviceToHost, p->device));
    if (p->n_segs) HIP_TRY(copy_sync(seg_special, p->d_special, (size_t)p->n_segs * 4, hipMemcpyDeviceToHost, p->device));
    return TGX_OK;
}
