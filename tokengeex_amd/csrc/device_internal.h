// What the device-side host code shares (tgx_api.cpp, encode_pass.cpp, estep_pass.cpp and lattice_pass.cpp: the passes on
// a model's own streams, which share pass_internal.h too; result_ops.cpp and corpus_ops.cpp: the calls on a caller's stream): the
// handle structs, the buffer pool's interface, the guards of a pass and of a call, the stage timer.  api_internal.h
// stays free of HIP for host_twins.cpp; this header is not.
// Everything with state (the pool, the default and copy streams) is DEFINED once, in tgx_api.cpp, and only declared
// here; the types live in tgx::dev, so that a handle struct is the same type in every translation unit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "trie_build.h"

// (expands where tgx::host::fail is visible)
#define HIP_TRY(expr)                                                                   \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(TGX_ERR_DEVICE, "HIP error %d (%s) at %s:%d: %s", (int)_e,        \
                        hipGetErrorString(_e), __FILE__, __LINE__, #expr);                \
    } while (0)

namespace tgx {
struct DedupRows;  // dedup.h
}

namespace tgx::dev {

// ---- device buffer pool (tgx_api.cpp) --------------------------------------------
hipError_t pool_alloc(int device, size_t bytes, void** out);
void pool_free(int device, void* ptr, size_t bytes);
// hipFree of every pooled buffer of `device` (all devices if < 0); the caller's current device is kept
void pool_trim(int device);
size_t rounded(size_t bytes);
// TGX_POOL_FILL (a knob): set the bytes the library is about to hand out, and wait for it; nothing without the knob.
// pool_alloc calls it over the pooled size; an allocator that bypasses the pool (generate.hip) calls it itself.
hipError_t pool_fill(int device, void* p, size_t bytes);

// A pooled device buffer with one owner: (device, ptr, bytes), bytes being the rounded size it was asked with (what the
// pool files it under).  It goes back to the pool exactly once: on reset(), on the next alloc() or with its owner.
template <class T>
class PoolBuf {
public:
    PoolBuf() = default;
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
    PoolBuf(PoolBuf&& o) noexcept : device_(o.device_), ptr_(o.ptr_), bytes_(o.bytes_) { o.ptr_ = nullptr; }
    PoolBuf& operator=(PoolBuf&& o) noexcept {
        if (this != &o) {
            reset();
            device_ = o.device_;
            ptr_ = o.ptr_;
            bytes_ = o.bytes_;
            o.ptr_ = nullptr;
        }
        return *this;
    }
    ~PoolBuf() { reset(); }

    hipError_t alloc(int device, size_t bytes) {
        reset();
        void* p = nullptr;
        const hipError_t e = pool_alloc(device, bytes, &p);
        if (e != hipSuccess) return e;
        device_ = device;
        ptr_ = static_cast<T*>(p);
        bytes_ = rounded(bytes);
        return hipSuccess;
    }
    void reset() {
        if (ptr_) pool_free(device_, ptr_, bytes_);
        ptr_ = nullptr;
    }
    T* get() const { return ptr_; }
    operator T*() const { return ptr_; }

private:
    int device_ = 0;
    T* ptr_ = nullptr;
    size_t bytes_ = 0;
};

struct KernelTime {
    const char* name;
    hipEvent_t start, stop;
    bool used;
};
constexpr int kMaxTimed = 8;

// The model's control words in device memory: the counters and flags its kernels share with the host, one member per
// role (this is the only place that says which kernel uses which).  Kernels take `unsigned long long*` to a member.  A
// pass holds m->mu, so one pass uses them at a time; each pass resets the ones it reads.
struct DeviceCtrl {
    unsigned long long queue;        // work queue of encode4 / encode4l / encode2 / encode5_kernel and the sampling kernels
    unsigned long long err;          // lowest failing sample (encode, sampling, n-best) or snippet (E-step); ~0: none
    unsigned long long queue6;       // encode6_kernel's own work queue when it runs beside encode5_kernel (co-run)
    struct Estep {                   // contiguous: an E-step pass clears these with ONE hipMemsetAsync over `estep`
        unsigned long long queue;       // estep7_kernel, estep7_redo_kernel, the forward kernels of estep4 / estep4l / estep5
        unsigned long long redo_count;  // estep7_kernel: stretches left to estep7_redo_kernel
        unsigned long long queue_bwd;   // the backward kernels of estep4 / estep4l
        unsigned long long range_flag;  // every linear-domain E-step kernel: the pass belongs to the log-domain kernels
    } estep;
    unsigned long long encode_redo;  // encode4l_kernel, the LONG build of encode5_kernel: samples left to encode2_kernel
    unsigned long long longest;      // estep_pieces_build: the longest piece (piece_len_kernel)
    unsigned long long err_piece;    // err_snip of the chained E-step kernels on pieces (z is checked per snippet afterwards)
};
static_assert(offsetof(DeviceCtrl::Estep, redo_count) == 8 && offsetof(DeviceCtrl::Estep, queue_bwd) == 16 &&
                  offsetof(DeviceCtrl::Estep, range_flag) == 24 && sizeof(DeviceCtrl::Estep) == 32,
              "the E-step words are cleared by one memset");
// what a pass reads back into page-locked host memory
struct HostCtrl {
    unsigned long long err;           // DeviceCtrl::err
    unsigned long long total_tokens;  // the last entry of the scanned token counts
};

}  // namespace tgx::dev

// ---- the handles of include/tgx.h -------------------------------------------------
using tgx::dev::DeviceCtrl;
using tgx::dev::HostCtrl;
using tgx::dev::KernelTime;
using tgx::dev::kMaxTimed;
using tgx::dev::PoolBuf;

struct tgx_model {
    int device = 0;
    uint32_t vocab_size = 0;
    uint32_t lm = 0;  // max token length rounded up to a multiple of 4 (>= 4)
    bool scores_finite = true;  // the four-samples-per-wave kernel encodes 'no token' as -inf
    tgx::FlatTrie flat;
    void* d_trie = nullptr;
    uint32_t* d_tokid = nullptr;
    DeviceCtrl* d_ctrl = nullptr;
    HostCtrl* h_ctrl = nullptr;  // page-locked
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;          // encode6_kernel beside encode5_kernel (encode_pass.cpp, encode_rows5: co-run)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned int* h_started = nullptr;      // page-locked, device-visible: blocks of encode5_kernel that are resident (co-run)
    int num_cus = 0;
    int blocks_per_cu = 0;  // encode_kernel (one sample per wave)
    // E-step only (built on first use): trie of the reversed tokens
    std::vector<uint8_t> vocab_bytes;
    std::vector<uint64_t> vocab_offs;
    std::vector<double> vocab_scores;
    tgx::FlatTrie flat_rev;
    void* d_trie_rev = nullptr;
    bool rev_host_built = false;    // flat_rev was built at creation (TGX_MODEL_FOR_ESTEP)
    void* d_trie_w = nullptr;       // forward / reversed tables with w = exp(score) in place of the score
    void* d_trie_rev_w = nullptr;   //   (linear-domain E-step, estep4l.hip)
    uint64_t last_long_samples = 0;    // samples the last pass gave a block of their own (encode6_kernel)
    uint64_t last_estep_pieces = 0;    // pieces the last E-step cut its snippets into (0: uncut)
    uint32_t last_corun_cus = 0;       // CUs the long-sample kernel had to itself beside encode5_kernel in the last pass (0: one after the other)
    double e7_overflow_share = 0.0;    // share of the sample's matches whose token ranks beyond 65 535 (ensure_estep_trie8t; 0 without counts)
    bool values_ranked = false;        // the score values were re-ranked by how often a sample of some corpus reads them (ensure_value_ranks)
    uint32_t corun_wait_timeouts = 0;  // co-run passes whose host wait for encode5_kernel's blocks ran into its 2 ms limit (then: no more co-runs)
    uint64_t last_redo_samples = 0;    // samples the last encode4l pass left to encode2_kernel
    int last_encode_waves_per_cu = 0;  // resident waves per CU of the last rows4 encode launch (self-check)
    bool estep_linear_ok = false;   // tables for the linear-domain E-step kernels exist
    tgx::TokHashTable tokhash;      // token bytes -> id (rows4 trace); ok == false: not usable
    void* d_tokhash = nullptr;
    // encode5_kernel: 8-byte label-checked records + table of distinct score values (trie_build.h: Trie8)
    void* d_trie8 = nullptr;
    void* d_top8 = nullptr;            // the top table over d_trie8 (top_table.h): written and re-ranked with it
    bool last_encode_top = false;      // the last encode5 launch ran a TOP build (no root copy in LDS)
    double* d_values = nullptr;       // f64[n_values + 1]: -inf, then the distinct score values by rank (trie_build.h: Trie8)
    std::vector<double> value_coverage;  // [k]: expected share of the matches whose value has rank <= k
    uint32_t n_values = 0, root_base8 = 0;
    uint32_t last_n_hot = 0;           // values in the LDS copy of the last encode5 launch
    bool lean_scores_ok = false;       // every score passes the gate of the lean relaxation step (lean_gate.h)
    bool last_ids_in_place = false;    // the last encode pass wrote its ids in place (ids_in_place.h): no tmp, no compact_kernel
    uint32_t last_lean_items = 0;      // lean items of the last pass's encode5_kernel (low byte) and encode6_kernel (next byte); 0: the kernels as they were
    bool have_trie8 = false;
    bool encode_tables_ready = false;  // tokhash / trie8 built and uploaded (ensure_encode_tables)
    bool estep_trie8_tried = false;    // ensure_estep_trie8 ran
    uint64_t estep_calls = 0;          // E-step passes this model has run (estep_rows4)
    bool have_wvalues = false;         // d_trie8 / d_wvalues are there for estep5_fwd_kernel
    double* d_wvalues = nullptr;       // f64[n_values + 1]: [0] = 0, [r] = exp(score value of rank r)
    bool tokhash_host_built = false;   // m->tokhash was built beside the forward trie at creation
    // estep7_kernel: token-ranked 8-byte records, w by rank (trie_build.h: Trie8T), built at the first E-step
    void* d_trie8t = nullptr;
    double* d_wtab = nullptr;          // f64[n_tok7 + 1]
    std::vector<uint32_t> id_of_rank;  // [r] = vocabulary id of the token of rank r (1 .. n_tok7)
    uint32_t n_tok7 = 0, root_base7 = 0;
    bool trie8t_tried = false, have_trie8t = false;
    uint64_t last_estep_redo = 0;      // stretches the last fused E-step left to the chained kernels
    // decode (decode.hip): the tokens' lengths, 16-byte slots and packed bytes, uploaded at the first decode (ensure_decode_tables)
    uint8_t* d_dec_len = nullptr;
    void* d_dec_slots = nullptr;
    uint8_t* d_dec_bytes = nullptr;
    uint64_t* d_dec_offs = nullptr;
    bool decode_tables_ready = false;
    // spans (spans.hip): one packed word per token (spans.h), uploaded at the first call (ensure_span_words)
    uint16_t* d_span_words = nullptr;
    bool span_words_ready = false;
    int estep_blocks_per_cu = 0;
    KernelTime timed[kMaxTimed] = {};
    int n_timed = 0;
    uint64_t last_alg_bytes = 0;
    std::mutex mu;  // one pass at a time per handle (its stream, counters and events)
};

struct tgx_corpus {
    int device = 0;
    uint64_t n_samples = 0, n_bytes = 0, max_len = 0;  // max_len: longest sample in bytes
    std::vector<uint64_t> h_offs;
    std::vector<uint32_t> h_sorted_len;  // sample lengths in the order of d_order (longest first) ...
    std::vector<uint64_t> h_sorted_cum;  // ... and their running sum
    PoolBuf<uint8_t> d_text_alloc;
    uint8_t* d_text = nullptr;        // = d_text_alloc + 256 (the backward E-step sweep reads before a position)
    PoolBuf<uint64_t> d_offs;
    PoolBuf<uint32_t> d_order;
    PoolBuf<uint32_t> d_bp, d_tmp, d_counts, d_status;  // scratch, allocated on first pass (ensure_scratch)
    PoolBuf<void> d_scan_tmp;
    size_t scan_tmp_bytes = 0;
    // E-step work list of the corpus (every sample cut at multiples of snippet_len, longest snippet first) and its
    // device copies: built on the first pass with a given snippet length, reused by the following ones (prune
    // runs two E-steps per iteration over the same corpus; building and sorting the list took 5 of 65 ms at 1 GiB)
    struct EstepWork {
        uint64_t snippet_len = 0;
        std::vector<uint64_t> soffs, sbase;
        std::vector<uint32_t> ssample, order;
        PoolBuf<uint64_t> d_soffs, d_sbase;
        PoolBuf<uint32_t> d_order, d_ssample;
        // windows of the snippets (cuts.hip: one boundary is sought per window): built with the work list
        uint32_t window = 0;
        uint64_t n_windows = 0;
        PoolBuf<uint32_t> d_win_snip, d_win_k;
    } es;
    // the scratch above belongs to the corpus, so a pass holds this lock too (always after its model's):
    // two models may work on one resident corpus from two host threads (prune and merge do, src/prune.rs:48)
    std::mutex mu;
};

struct tgx_result {
    int device = 0;
    uint32_t vocab_size = 0;  // of the model that wrote it: every id is below it
    uint64_t n_samples = 0, n_tokens = 0;
    PoolBuf<uint32_t> d_ids;
    PoolBuf<uint64_t> d_offs;
    std::unique_ptr<uint32_t[]> h_ids;  // uninitialised: a vector would zero a GB first
    std::vector<uint64_t> h_offs;
    bool have_ids = false, have_offs = false;
};

struct tgx_plan {
    int device = 0;
    uint64_t n_samples = 0, n_segs = 0, n_enc = 0;  // S, K, E
    uint32_t n_specials = 0;                        // of the list the corpus was split with
    PoolBuf<uint64_t> d_seg_offs;                   // u64[S+1]
    PoolBuf<int32_t> d_special;                     // i32[K+1]: entry K belongs to the assembly's scan
};

struct tgx_text {
    int device = 0;
    uint64_t n_rows = 0, n_bytes = 0, n_replaced = 0;
    PoolBuf<uint8_t> d_bytes;
    PoolBuf<uint64_t> d_offs;
};

namespace tgx::dev {

// TGX_ERR_DEVICE without a usable HIP device; *n_devices: how many there are
tgx_status require_device(int* n_devices = nullptr);
// a model's kernel timer (tgx_last_kernel_times): events on m->stream around what is launched between the two
void time_begin(tgx_model* m, const char* name);
void time_end(tgx_model* m);

// One pass over a corpus (encode, sampling, n-best, a frequency, pair or E-step pass, a re-rank of a model's tables): it
// owns the pass's scratch and the result it builds.  A pass that fails may have queued kernels that still read or write
// those buffers, the corpus's scratch or the result, so the model's streams are synchronised before anything goes back to
// the pool, where another caller could take it.  A pass that succeeds says so with done(): every success path has
// synchronised its stream already (or ended in a synchronous copy), and gains no synchronisation here.
class Pass {
public:
    explicit Pass(tgx_model* m) : m_(m) {}
    Pass(const Pass&) = delete;
    Pass& operator=(const Pass&) = delete;
    ~Pass() {
        if (ok_) return;
        (void)hipStreamSynchronize(m_->stream);
        if (m_->stream2) (void)hipStreamSynchronize(m_->stream2);
    }  // (then the members go: the scratch and an unclaimed result)

    template <class T>
    hipError_t alloc(size_t bytes, T** out) {
        PoolBuf<void> b;
        const hipError_t e = b.alloc(m_->device, bytes);
        *out = static_cast<T*>(b.get());
        if (e == hipSuccess) scratch_.push_back(std::move(b));
        return e;
    }
    tgx_result* new_result(uint64_t n_samples) {
        result_.reset(new tgx_result());
        result_->device = m_->device;
        result_->vocab_size = m_->vocab_size;
        result_->n_samples = n_samples;
        return result_.get();
    }
    tgx_result* release_result() { return result_.release(); }
    void adopt_result(tgx_result* r) { result_.reset(r); }
    tgx_status done() {
        ok_ = true;
        return TGX_OK;
    }

private:
    tgx_model* m_;
    bool ok_ = false;
    std::vector<PoolBuf<void>> scratch_;
    std::unique_ptr<tgx_result> result_;
};

// the calling thread's current device is put back when a layout entry point that had to change it returns
class DeviceScope {
public:
    DeviceScope() { (void)hipGetDevice(&prev_); }
    ~DeviceScope() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;

private:
    int prev_ = -1;
};

// the stream of a caller that passes none: one blocking stream per device
hipStream_t stream_or_default(void* stream, int device);
// p (may be NULL when optional) must be device memory of `device`, which is the current device and that of `owner`
tgx_status check_device_ptr(const char* who, const char* what, const void* p, int device, const char* owner);

// One call's work on a caller's stream (or stream_or_default's).  It owns the call's pooled buffers and the host memory
// its uploads read.  A call that fails may have queued work that still uses them, the result or the caller's
// destination, so the stream is synchronised before anything goes back to the pool or to the caller.  A call that
// succeeds has synchronised the stream itself and says so with done().  What must outlive the stream's work and is not
// the guard's (a tgx_text, a buffer that moves into one, host memory a copy writes) is declared BEFORE the guard.
// (Pass is the same for a model's own streams.)
class StreamGuard {
public:
    StreamGuard(int device, hipStream_t stream) : device_(device), stream_(stream) {}
    StreamGuard(const StreamGuard&) = delete;
    StreamGuard& operator=(const StreamGuard&) = delete;
    ~StreamGuard() {
        if (!ok_) (void)hipStreamSynchronize(stream_);
    }  // (then the members go)

    template <class T>
    hipError_t alloc(size_t bytes, T** out) {
        PoolBuf<void> b;
        const hipError_t e = b.alloc(device_, bytes);
        *out = static_cast<T*>(b.get());
        if (e == hipSuccess) bufs_.push_back(std::move(b));
        return e;
    }
    // src to dst (device memory) on the stream; src lives as long as the guard
    hipError_t upload(uint64_t* dst, std::vector<uint64_t> src) {
        staged_.push_back(std::move(src));
        return hipMemcpyAsync(dst, staged_.back().data(), staged_.back().size() * 8, hipMemcpyHostToDevice, stream_);
    }
    void done() { ok_ = true; }

private:
    int device_;
    hipStream_t stream_;
    bool ok_ = false;
    std::vector<PoolBuf<void>> bufs_;
    std::vector<std::vector<uint64_t>> staged_;
};

// Device time of one call's N stages on its stream: an event pair per stage, read into ms (N entries: a thread-local
// array of the subsystem's) once the stream has reached its end.  A path that returns without read() leaves the
// previous call's times in ms, and the two early returns differ in this: tgx_corpus_split_specials on an empty input
// does not call read(), so the times of the call before it stay; tgx_corpus_normalize's copy of a corpus without pieces
// does, so its times read zero.
template <int N>
class StageTimer {
public:
    StageTimer(hipStream_t hs, float* ms) : hs_(hs), ms_(ms) {
        for (auto& e : ev_) ok_ = ok_ && hipEventCreate(&e) == hipSuccess;
    }
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() {
        for (auto& e : ev_)
            if (e) (void)hipEventDestroy(e);
    }
    void begin(int stage) {
        if (ok_) used_[stage] = hipEventRecord(ev_[2 * stage], hs_) == hipSuccess;
    }
    void end(int stage) {
        if (ok_ && used_[stage]) used_[stage] = hipEventRecord(ev_[2 * stage + 1], hs_) == hipSuccess;
    }
    void read() {  // after the stream has reached its end
        for (int k = 0; k < N; k++) {
            ms_[k] = 0;
            if (ok_ && used_[k]) (void)hipEventElapsedTime(&ms_[k], ev_[2 * k], ev_[2 * k + 1]);
        }
    }

private:
    hipStream_t hs_;
    float* ms_;
    hipEvent_t ev_[2 * N] = {};
    bool used_[N] = {};
    bool ok_ = true;
};
// what the tgx_*_last_times getters share: up to cap of the n stages' names and times -> how many
int stage_times(const char* const* stage_names, const float* stage_ms, int n, const char** names, float* ms, int cap);

// n 8-byte words of device memory to host words on the stream, then the stream's end.  The host words are the caller's
// and declared before its guard: after a failure the copy may still write them until the guard has synchronised.
tgx_status read_u64(hipStream_t hs, const void* d_src, void* host_words, size_t n = 1);

// A call's scratch for scans of up to n elements, in pooled memory of its guard (a StreamGuard or a Pass): asked for again
// only when n exceeds what is known so far.  temp_bytes: the subsystem's size query.  After TGX_OK ptr is never NULL, which
// would ask a scan for its size, whatever n is.  oom: the error's text when the allocation fails, for the calls that
// report "out of device memory (...)" (default: the HIP error's).
struct ScanScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
    uint64_t n = 0;
};
tgx_status scan_room(ScanScratch* s, StreamGuard& guard, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n, const char* oom = nullptr);
tgx_status scan_room(ScanScratch* s, Pass& pass, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n, const char* oom = nullptr);

// ---- row selection (result_ops.cpp; tgx_corpus_select in corpus_ops.cpp shares it) ------------------------------------
// device time of the calling thread's last select per stage (tgx_select_last_times)
constexpr int kSelectStages = 3;
float* select_stage_ms();
// The indices of a select on the device.  Host rows (no TGX_SELECT_ROWS_DEVICE; the caller has checked every index with
// select_check_rows before its first device call) are uploaded on the guard's stream into pooled memory of the guard.
// Device rows: the pointer is checked (the current device is `device`), nothing is queued.  *d_rows: what the kernels
// read (NULL when M = 0).
tgx_status select_rows_device(const char* who, const int64_t* rows, uint64_t n_select, uint32_t flags, int device, StreamGuard& guard,
                              const int64_t** d_rows);
// The bad-index word of device rows: what select_check_kernel left (kSelectNoBad: every index in range) -> TGX_OK, or
// TGX_ERR_INVALID naming k and rows[k], which is read from the device for the message.
tgx_status select_bad_index(const char* who, uint64_t bad_k, const int64_t* d_rows, uint64_t n_src, hipStream_t hs);

// ---- exact row deduplication (result_ops.cpp; the corpus's entry points in corpus_ops.cpp share it) ---------------------
// The rounds of tgx_*_first_equal_device and the hashes of tgx_*_row_hashes_device over the rows of a result or of a
// corpus (dedup.h: DedupRows), on the caller's stream under a StreamGuard of their own.  The handle, the flags and a
// device have been checked; the destination is checked here, before anything is queued.
tgx_status dedup_first_equal(const char* who, const tgx::DedupRows& rows, int device, void* stream, int64_t* d_first, uint64_t* n_unique);
tgx_status dedup_row_hashes(const char* who, const tgx::DedupRows& rows, int device, uint64_t seed, void* stream, uint64_t* d_hashes);

// ---- corpora (tgx_api.cpp) ----------------------------------------------------------
// a copy on the device's copy stream of that direction, and the stream's end
hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, int device);
enum class TextFrom { Host, Device, Caller };
tgx_status corpus_create(const char* who, int device, const uint8_t* text, TextFrom from, const uint64_t* offs, uint64_t n_samples,
                         tgx_corpus** out);

}  // namespace tgx::dev
