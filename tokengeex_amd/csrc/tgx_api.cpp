// C ABI (include/tgx.h) over the HIP kernels: handles, HBM buffers, launch
// sequencing, error reporting.  Host side of the reference's batch loops
// (src/tokenizer.rs:102-123, src/prune.rs:205-244); there is no CPU fallback —
// without a usable gfx950 device every compute entry point returns TGX_ERR_DEVICE.
// Here: the error state, the buffer pool, the knobs, models and corpora, the result accessors and the counting passes.
// The encode pass is in encode_pass.cpp, the E-step in estep_pass.cpp, sampling, lattice statistics and n-best in
// lattice_pass.cpp (pass_internal.h: what they take from here).  The transforms of a resident result or corpus on a
// caller's stream are in result_ops.cpp and corpus_ops.cpp (device_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "kernels.h"
#include "lean_gate.h"
#include "pass_internal.h"
#include "trie_build.h"

using namespace tgx::host;
using namespace tgx::dev;

// shared with prune_host.cpp: records the message tgx_last_error() returns (thread-local)
tgx_status tgx_set_error(tgx_status st, const char* msg) {
    g_err_msg = msg ? msg : "";
    return st;
}
namespace {

// ---- device buffer pool --------------------------------------------------------
// hipMalloc/hipFree cost far more than a kernel launch; scratch and result
// buffers are recycled through a small per-process free list.
struct PoolEntry {
    void* ptr;
    size_t bytes;
    int device;
};
std::mutex g_pool_mu;
std::vector<PoolEntry> g_pool;
size_t g_pool_bytes = 0;
constexpr size_t kPoolMaxBytes = 64ull << 30;
std::atomic<uint64_t> g_pool_filled_bytes{0};  // tgx_pool_filled_bytes

}  // namespace

namespace tgx::dev {

// hipFree of every pooled buffer of `device` (all devices if < 0); the caller's current device is kept
void pool_trim(int device) {
    std::vector<PoolEntry> victims;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool.size();) {
            if (device < 0 || g_pool[i].device == device) {
                victims.push_back(g_pool[i]);
                g_pool_bytes -= g_pool[i].bytes;
                g_pool.erase(g_pool.begin() + (long)i);
            } else {
                i++;
            }
        }
    }
    if (victims.empty()) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (const PoolEntry& e : victims) {
        (void)hipSetDevice(e.device);
        (void)hipFree(e.ptr);
    }
    if (prev >= 0) (void)hipSetDevice(prev);
}

// TGX_POOL_FILL=<0..255> (a knob, read per allocation): the `bytes` at p, device memory of `device` that the library
// is about to hand out, are set to that byte, and the device has finished doing so on return, so that nothing the
// caller queues on any stream can overtake the fill.  Without the knob: nothing, and no HIP call.  The tests' way of
// making the library's own memory hostile: a recycled buffer holds what its previous owner left anyway, this makes it
// one known value over the whole pooled size (tests/test_pool_fill_gpu.py).
hipError_t pool_fill(int device, void* p, size_t bytes) {
    const char* e = knob("TGX_POOL_FILL");
    if (!e || !*e) return hipSuccess;
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (*end || v < 0 || v > 255 || !p || bytes == 0) return hipSuccess;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != device) (void)hipSetDevice(device);
    hipError_t st = hipMemset(p, (int)v, bytes);
    if (st == hipSuccess) st = hipDeviceSynchronize();
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    if (st == hipSuccess) g_pool_filled_bytes.fetch_add(bytes, std::memory_order_relaxed);
    return st;
}

hipError_t pool_alloc(int device, size_t bytes, void** out) {
    if (bytes == 0) bytes = 256;
    bytes = (bytes + 255) & ~size_t(255);
    {
        std::unique_lock<std::mutex> lk(g_pool_mu);
        size_t best = g_pool.size();
        for (size_t i = 0; i < g_pool.size(); i++) {
            const PoolEntry& e = g_pool[i];
            if (e.device != device || e.bytes < bytes || e.bytes > bytes * 2 + (1u << 20)) continue;
            if (best == g_pool.size() || e.bytes < g_pool[best].bytes) best = i;
        }
        if (best != g_pool.size()) {
            *out = g_pool[best].ptr;
            const size_t entry_bytes = g_pool[best].bytes;
            g_pool_bytes -= entry_bytes;
            g_pool.erase(g_pool.begin() + (long)best);
            lk.unlock();
            const hipError_t fe = pool_fill(device, *out, entry_bytes);
            if (fe != hipSuccess) {  // (a caller takes any failure as "nothing allocated")
                pool_free(device, *out, entry_bytes);
                *out = nullptr;
            }
            return fe;
        }
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory) {
        // the pool may be what fills the device (passes of very different sizes, or memory shared with
        // torch / RCCL allocations): give everything back and try once more
        (void)hipGetLastError();
        pool_trim(device);
        e = hipMalloc(out, bytes);
    }
    if (e != hipSuccess) return e;
    e = pool_fill(device, *out, bytes);
    if (e != hipSuccess) {
        (void)hipFree(*out);
        *out = nullptr;
    }
    return e;
}

size_t rounded(size_t bytes) {
    if (bytes == 0) bytes = 256;
    return (bytes + 255) & ~size_t(255);
}

// Pooled bytes per process: at most a quarter of the device's memory (and never more than kPoolMaxBytes).
static size_t pool_cap(int device) {
    static size_t cap[16] = {0};
    if (device < 0 || device >= 16) return kPoolMaxBytes;
    if (cap[device] == 0) {
        size_t free_b = 0, total_b = 0;
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 4 * kPoolMaxBytes;
        if (prev >= 0) (void)hipSetDevice(prev);
        cap[device] = std::min<size_t>(kPoolMaxBytes, total_b / 4);
    }
    return cap[device];
}

void pool_free(int device, void* ptr, size_t bytes) {
    if (!ptr) return;
    bytes = rounded(bytes);
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool_bytes + bytes <= pool_cap(device) && g_pool.size() < 256) {
            g_pool.push_back(PoolEntry{ptr, bytes, device});
            g_pool_bytes += bytes;
            return;
        }
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    (void)hipFree(ptr);
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
}

}  // namespace tgx::dev

namespace {

int usable_device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

}  // namespace

namespace tgx::dev {

// TGX_DEBUG=1: log every launch to stderr and synchronise after it, so that a
// device fault can be attributed to one kernel.
bool debug_on() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("TGX_DEBUG");
        v = (e && *e && *e != '0') ? 1 : 0;
    }
    return v == 1;
}

// Environment switches that choose among the library's (all correct) kernels and geometries exist for the
// parity tests, A/B timing and diagnosis; a process must opt in with TGX_KNOBS=1 (tests/conftest.py does) or
// TGX_DEBUG=1, so that a stray variable in a production environment changes nothing.
const char* knob(const char* name) {
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("TGX_KNOBS");
        on = ((e && *e && *e != '0') || debug_on()) ? 1 : 0;
    }
    return on == 1 ? getenv(name) : nullptr;
}

tgx_status require_device(int* n_devices) {
    const int n = usable_device_count();
    if (n_devices) *n_devices = n;
    if (n <= 0) return fail(TGX_ERR_DEVICE, "no usable HIP device (gfx950 required)");
    return TGX_OK;
}

void time_begin(tgx_model* m, const char* name) {
    if (debug_on()) {
        fprintf(stderr, "[tgx] launch %s\n", name);
        fflush(stderr);
    }
    if (m->n_timed >= kMaxTimed) return;
    KernelTime& t = m->timed[m->n_timed];
    t.name = name;
    t.used = true;
    (void)hipEventRecord(t.start, m->stream);
}
void time_end(tgx_model* m) {
    if (debug_on()) {
        hipError_t e = hipStreamSynchronize(m->stream);
        fprintf(stderr, "[tgx]   done: %s\n", hipGetErrorString(e));
        fflush(stderr);
    }
    if (m->n_timed >= kMaxTimed) return;
    (void)hipEventRecord(m->timed[m->n_timed].stop, m->stream);
    m->n_timed++;
}

// ---- what the passes share (pass_internal.h; encode_pass.cpp, estep_pass.cpp, lattice_pass.cpp) -------------------

// the encode and sampling passes' scratch: back-pointers, ids right-aligned in `tmp` (then compacted), counts, status.
// with_tmp = false: a pass that writes its ids in place (ids_in_place.h) needs no `tmp` — 4 bytes per text byte that a
// corpus which only ever sees such passes never allocates.
tgx_status ensure_scratch(tgx_corpus* c, bool with_tmp) {
    HIP_TRY(hipSetDevice(c->device));
    // u32[N] for the one-sample-per-wave kernel; the rows4 kernels use it as bytes, N + 128 per sample
    if (!c->d_bp) HIP_TRY(c->d_bp.alloc(c->device, std::max((size_t)c->n_bytes * 4 + 256, (size_t)c->n_bytes + 128 * (size_t)c->n_samples + 512)));
    if (!c->d_counts) HIP_TRY(c->d_counts.alloc(c->device, (size_t)c->n_samples * 4 + 256));
    if (!c->d_status) HIP_TRY(c->d_status.alloc(c->device, (size_t)c->n_samples * 4 + 256));
    if (with_tmp && !c->d_tmp) HIP_TRY(c->d_tmp.alloc(c->device, (size_t)c->n_bytes * 4 + 256));
    return TGX_OK;
}

// An integer knob that holds only inside [lo, hi]: any other value is ignored.
void knob_int(const char* name, int lo, int hi, int* x) {
    if (const char* e = knob(name)) {
        const int v = atoi(e);
        if (v >= lo && v <= hi) *x = v;
    }
}
// TGX_E5_HOT / TGX_E7_HOT: a smaller LDS copy than fits (tests of the COLD builds, table-size sweeps)
uint32_t knob_cap_hot(const char* name, uint32_t n_hot) {
    if (const char* e = knob(name)) {
        const int v = atoi(e);
        if (v >= 0) n_hot = std::min(n_hot, (uint32_t)v);
    }
    return n_hot;
}
// TGX_FLAGS: timing experiments (tools/ablate.py) — results are WRONG when set; honoured only with TGX_DEBUG=1
uint32_t debug_flags() {
    const char* f = debug_on() ? getenv("TGX_FLAGS") : nullptr;
    return f ? (uint32_t)atoi(f) : 0u;
}

// blocks of the trace kernels: four samples per block and round, eight blocks per CU
uint32_t trace_blocks(const tgx_model* m, uint64_t n_samples) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_samples + 3) / 4, (uint64_t)m->num_cus * 8));
}
// fewer waves (of four rows) per block when the pass has fewer units than the chip has rows, so that they spread over
// the `n_blocks` resident blocks
int waves_for_units(int waves, uint64_t units, uint64_t n_blocks) {
    const uint64_t rows_wanted = (units + n_blocks - 1) / n_blocks;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)waves, (rows_wanted + 3) / 4));
}
// rows claim several consecutive units of the order per atomic when units are short: one global atomic round trip
// (~1-2 us) per unit is what a corpus of 130-byte samples otherwise waits for
uint32_t claim_chunk_for(uint64_t n_bytes, uint64_t units) {
    const uint64_t avg = units ? n_bytes / units : 0;
    return (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(1, 4096 / std::max<uint64_t>(1, avg)));
}

// (Stamps: pass_internal.h)
Stamps stamps_begin(tgx_model* m, Pass& pass, char which, size_t n_waves) {
    const char* e = debug_on() ? getenv("TGX_STAMPS") : nullptr;
    Stamps st;
    st.n_waves = n_waves;
    if (!e || *e != which || pass.alloc(n_waves * 64, &st.d) != hipSuccess || hipMemsetAsync(st.d, 0, n_waves * 64, m->stream) != hipSuccess)
        st.d = nullptr;
    return st;
}
// ... and after the launch: mean ticks per `unit` and phase over all waves (a wave counts its units in the word after its
// phases).  ppl: positions per lane, named in the line unless 0.
void stamps_report(tgx_model* m, const Stamps& st, int ppl, const char* what, const char* unit, std::initializer_list<const char*> phases) {
    std::vector<unsigned long long> h(st.n_waves * 8);
    if (hipStreamSynchronize(m->stream) != hipSuccess || hipMemcpy(h.data(), st.d, st.n_waves * 64, hipMemcpyDeviceToHost) != hipSuccess) return;
    const size_t np = phases.size();  // (at most 7)
    double sum[7] = {0, 0, 0, 0, 0, 0, 0}, count = 0;
    for (size_t w = 0; w < st.n_waves; w++) {
        for (size_t i = 0; i < np; i++) sum[i] += (double)h[w * 8 + i];
        count += (double)h[w * 8 + np];
    }
    fprintf(stderr, "[tgx] %s (s_memtime ticks per wave-%s, %zu waves", what, unit, st.n_waves);
    if (ppl) fprintf(stderr, " x ppl %d", ppl);
    fprintf(stderr, ", %.0f %ss):", count, unit);
    size_t i = 0;
    for (const char* name : phases) {
        fprintf(stderr, "%s %s %.0f", i ? " " : "", name, sum[i] / count);
        i++;
    }
    fprintf(stderr, "\n");
}

}  // namespace tgx::dev

const char* tgx_last_error(void) { return g_err_msg.c_str(); }

void tgx_last_error_detail(uint64_t* sample, uint64_t* pos, uint64_t* len) {
    if (sample) *sample = g_err_sample;
    if (pos) *pos = g_err_pos;
    if (len) *len = g_err_len;
}

int tgx_abi_version(void) { return TGX_ABI_VERSION; }
int tgx_device_count(void) { return usable_device_count(); }
void tgx_free(void* p) { free(p); }
void tgx_pool_trim(int device) { pool_trim(device); }
uint64_t tgx_pool_filled_bytes(void) { return g_pool_filled_bytes.load(std::memory_order_relaxed); }
void* tgx_host_alloc(uint64_t bytes) {
    if (require_device() != TGX_OK) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? (size_t)bytes : 1, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        fail(TGX_ERR_DEVICE, "out of page-locked host memory (%llu bytes)", (unsigned long long)bytes);
        return nullptr;
    }
    return p;
}
void tgx_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

static tgx_status finish_model_create(tgx_model* m, const uint8_t* bytes, const uint64_t* offs, const double* scores,
                                      uint32_t vocab_size, int device, uint32_t flags, tgx_model** out);

tgx_status tgx_model_create(const uint8_t* bytes, const uint64_t* offs, const double* scores,
                            uint32_t vocab_size, int device, tgx_model** out) {
    return tgx_model_create_ex(bytes, offs, scores, vocab_size, device, 0, out);
}

tgx_status tgx_model_create_ex(const uint8_t* bytes, const uint64_t* offs, const double* scores,
                               uint32_t vocab_size, int device, uint32_t flags, tgx_model** out) {
    if (!out) return fail(TGX_ERR_INVALID, "tgx_model_create: out is NULL");
    *out = nullptr;
    if (vocab_size && (!offs || !scores)) return fail(TGX_ERR_INVALID, "tgx_model_create: NULL vocab");
    if (vocab_size && !bytes && offs[vocab_size] != offs[0]) return fail(TGX_ERR_INVALID, "tgx_model_create: NULL token bytes");
    int ndev = 0;
    if (const tgx_status dst = require_device(&ndev)) return dst;
    if (device < 0 || device >= ndev)
        return fail(TGX_ERR_INVALID, "device %d out of range (have %d)", device, ndev);

    tgx::HostPhases hp("tgx_model_create");
    tgx_model* m = new tgx_model();
    m->device = device;
    m->vocab_size = vocab_size;
    static const uint64_t zero_offs[1] = {0};
    // TGX_MODEL_FOR_ESTEP: the double-array of the REVERSED tokens (backward sweep of the E-step) is built
    // on a second host thread while this one builds the forward table — `prune` makes a new model for every
    // EM sub-iteration (src/prune.rs:48), and at 500 K tokens each table takes ~0.4 s of host time
    // (round 4: not for vocabularies estep7_kernel serves — tokens of at most 16 bytes, scores within +-300: its E-step
    // walks the forward table only; the reversed table is then built if a pass ever falls back to the chained kernels)
    bool fused_estep = vocab_size != 0;
    for (uint32_t i = 0; i < vocab_size && fused_estep; i++)
        fused_estep = offs[i + 1] - offs[i] <= 16 && scores[i] >= -300.0 && scores[i] <= 300.0;
    std::thread rev_builder;
    if ((flags & TGX_MODEL_FOR_ESTEP) && vocab_size && !fused_estep)
        rev_builder = std::thread([m, bytes, offs, scores, vocab_size]() {
            const uint64_t o0 = offs[0];
            std::vector<uint8_t> rev((size_t)(offs[vocab_size] - o0));
            std::vector<uint64_t> ro(vocab_size + 1);
            for (uint32_t i = 0; i <= vocab_size; i++) ro[i] = offs[i] - o0;
            for (uint32_t i = 0; i < vocab_size; i++)
                for (uint64_t k = ro[i]; k < ro[i + 1]; k++) rev[k] = bytes[o0 + ro[i + 1] - 1 - (k - ro[i])];
            tgx::build_flat_trie(rev.data(), ro.data(), scores, vocab_size, &m->flat_rev);
        });
    // a model for encode: the bytes -> id table does not depend on the trie and is built beside it
    std::thread hash_early;
    if (!(flags & TGX_MODEL_FOR_ESTEP) && vocab_size) {
        bool finite = true;
        uint64_t longest = 0;
        for (uint32_t i = 0; i < vocab_size; i++) {
            finite = finite && (scores[i] - scores[i] == 0.0);
            longest = std::max<uint64_t>(longest, offs[i + 1] - offs[i]);
        }
        if (finite && longest <= 32) {
            hash_early = std::thread([m, bytes, offs, vocab_size]() {
                // (same arguments as ensure_encode_tables: token bytes from offs[0] on, offsets rebased to 0)
                std::vector<uint64_t> ro(vocab_size + 1);
                for (uint32_t i = 0; i <= vocab_size; i++) ro[i] = offs[i] - offs[0];
                tgx::build_tok_hash(bytes + offs[0], ro.data(), vocab_size, &m->tokhash);
            });
        }
    }
    hp.mark("scan of the vocabulary");
    tgx::build_flat_trie(bytes, vocab_size ? offs : zero_offs, scores, vocab_size, &m->flat);
    hp.mark("build_flat_trie");
    if (hash_early.joinable()) {
        hash_early.join();
        m->tokhash_host_built = true;
    }
    if (rev_builder.joinable()) {
        rev_builder.join();
        m->rev_host_built = true;
    }
    hp.mark("join hash / reverse builders");
    const tgx_status fst = finish_model_create(m, bytes, offs, scores, vocab_size, device, flags, out);
    hp.mark("finish (device tables)");
    return fst;
}

// the part of model creation after the host tables exist: checks, device tables, uploads
static tgx_status finish_model_create(tgx_model* m, const uint8_t* bytes, const uint64_t* offs, const double* scores,
                                      uint32_t vocab_size, int device, uint32_t flags, tgx_model** out) {
    std::unique_ptr<tgx_model, void (*)(tgx_model*)> owner(m, tgx_model_destroy);  // released on success only
    if (m->flat.max_token_len > TGX_MAX_TOKEN_LEN)
        return fail(TGX_ERR_UNSUPPORTED, "token of %u bytes exceeds TGX_MAX_TOKEN_LEN (%d)", m->flat.max_token_len,
                    TGX_MAX_TOKEN_LEN);
    if (m->flat.table.size() >= (1u << 26)) return fail(TGX_ERR_UNSUPPORTED, "trie needs more than 2^26 slots");
    m->lm = std::max<uint32_t>(4, (m->flat.max_token_len + 3) & ~3u);
    if (vocab_size) {
        m->vocab_bytes.assign(bytes + offs[0], bytes + offs[vocab_size]);
        m->vocab_offs.resize(vocab_size + 1);
        for (uint32_t i = 0; i <= vocab_size; i++) m->vocab_offs[i] = offs[i] - offs[0];
        m->vocab_scores.assign(scores, scores + vocab_size);
        for (uint32_t i = 0; i < vocab_size; i++)
            if (!(scores[i] - scores[i] == 0.0)) m->scores_finite = false;  // inf or NaN
        m->lean_scores_ok = tgx::lean_scores_ok(scores, vocab_size);
    } else {
        m->vocab_offs.assign(1, 0);
    }

    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    m->num_cus = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    size_t tbytes = m->flat.table.size() * sizeof(tgx::TrieRec);
    HIP_TRY(hipMalloc(&m->d_trie, tbytes));
    HIP_TRY(hipMalloc((void**)&m->d_tokid, m->flat.tokid.size() * 4));
    HIP_TRY(hipMalloc((void**)&m->d_ctrl, sizeof(DeviceCtrl)));
    // the tables only encode needs (bytes -> id table of the trace, 8-byte records and score table of
    // encode5_kernel): now, unless the model is created for E-step passes — then at its first encode
    if (!(flags & TGX_MODEL_FOR_ESTEP)) {
        const tgx_status est = ensure_encode_tables(m);
        if (est != TGX_OK) return est;
    }
    HIP_TRY(hipHostMalloc((void**)&m->h_ctrl, sizeof(HostCtrl), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(m->d_trie, m->flat.table.data(), tbytes, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->d_tokid, m->flat.tokid.data(), m->flat.tokid.size() * 4, hipMemcpyHostToDevice, m->stream));
    for (int i = 0; i < kMaxTimed; i++) {
        m->timed[i].used = false;
        m->timed[i].name = "";
        HIP_TRY(hipEventCreate(&m->timed[i].start));
        HIP_TRY(hipEventCreate(&m->timed[i].stop));
    }
    {
        int occ = 0;
        HIP_TRY(tgx::encode_max_blocks_per_cu(m->lm, &occ));
        m->blocks_per_cu = std::max(1, std::min(occ, 16));
    }
    HIP_TRY(hipStreamSynchronize(m->stream));
    *out = owner.release();
    return TGX_OK;
}

// A model for a SUBSET of another model's vocabulary with new scores, on the other model's double-arrays: the tokens that
// are gone lose their terminal mark, the others get their new id and score, and nothing is rebuilt — a trie with dead
// branches gives the same matches.  `prune` makes three models per iteration (two EM sub-iterations and the pruning step,
// src/prune.rs:36-56), each for a subset of the one before; the double-array builds were two thirds of an iteration at
// 500 000 entries.  keep_ids: ascending ids of the parent's vocabulary; new id = position in keep_ids.
// Not for parents with duplicate tokens (only the last duplicate is in the parent's tables): TGX_ERR_UNSUPPORTED, the
// caller builds the model from scratch.
tgx_status tgx_model_create_derived(const tgx_model* parent, const uint32_t* keep_ids, uint32_t n_keep, const double* scores,
                                    uint32_t flags, tgx_model** out) {
    if (!out) return fail(TGX_ERR_INVALID, "tgx_model_create_derived: out is NULL");
    *out = nullptr;
    if (!parent || (n_keep && (!keep_ids || !scores))) return fail(TGX_ERR_INVALID, "tgx_model_create_derived: NULL argument");
    tgx::HostPhases hp("tgx_model_create_derived");
    const uint32_t PV = parent->vocab_size;
    for (uint32_t i = 0; i < n_keep; i++)
        if (keep_ids[i] >= PV || (i && keep_ids[i] <= keep_ids[i - 1])) return fail(TGX_ERR_INVALID, "tgx_model_create_derived: keep_ids must ascend within the parent's vocabulary");
    // A derived model keeps the parent's slot count.  A parent above the 8-byte records' limit would leave the model that
    // `prune` encodes with (its frequency pass) on the 16-byte kernels however small the vocabulary has become: such a
    // model is built from scratch (the caller does that on TGX_ERR_UNSUPPORTED), its own table is within the limit sooner.
    if (!(flags & TGX_MODEL_FOR_ESTEP) && parent->flat.table.size() > tgx::kTrie8MaxSlots && (uint64_t)n_keep * 2 <= PV)
        return fail(TGX_ERR_UNSUPPORTED, "tgx_model_create_derived: the parent's table has more slots than 8-byte records address; build this model from scratch");
    {   // every non-empty token of the parent must own a terminal slot
        uint64_t non_empty = 0, terminals = 0;
        for (uint32_t i = 0; i < PV; i++) non_empty += parent->vocab_offs[i + 1] > parent->vocab_offs[i];
        for (uint32_t t : parent->flat.tokid) terminals += t != tgx::kNoToken;
        if (terminals != non_empty) return fail(TGX_ERR_UNSUPPORTED, "tgx_model_create_derived: the parent vocabulary has duplicate tokens");
    }
    tgx_model* m = new tgx_model();
    m->device = parent->device;
    m->vocab_size = n_keep;
    std::vector<uint32_t> new_id(PV, tgx::kNoToken);
    for (uint32_t i = 0; i < n_keep; i++) new_id[keep_ids[i]] = i;
    // the new vocabulary's bytes (the tail of creation copies them into the model)
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offs;
    const uint32_t longest = tgx::gather_derived_vocab(parent->vocab_bytes.data(), parent->vocab_offs.data(), keep_ids, n_keep, &bytes, &offs);
    hp.mark("checks + bytes");
    auto derive = [&](const tgx::FlatTrie& src, tgx::FlatTrie* dst) { tgx::derive_flat_trie(src, new_id, scores, longest, dst); };
    // (the parent's reversed table is built, if ever, under its lock: ensure_reverse_trie)
    std::unique_lock<std::mutex> parent_lock(const_cast<tgx_model*>(parent)->mu);
    std::thread rev_deriver;
    const bool want_rev = (flags & TGX_MODEL_FOR_ESTEP) && parent->rev_host_built && n_keep;
    if (want_rev) rev_deriver = std::thread([&]() { derive(parent->flat_rev, &m->flat_rev); });
    std::thread hash_early;
    if (!(flags & TGX_MODEL_FOR_ESTEP) && n_keep && longest <= 32) {
        bool finite = true;
        for (uint32_t i = 0; i < n_keep; i++) finite = finite && (scores[i] - scores[i] == 0.0);
        if (finite) hash_early = std::thread([&]() { tgx::build_tok_hash(bytes.data(), offs.data(), n_keep, &m->tokhash); });
    }
    derive(parent->flat, &m->flat);
    if (hash_early.joinable()) {
        hash_early.join();
        m->tokhash_host_built = true;
    }
    if (rev_deriver.joinable()) {
        rev_deriver.join();
        m->rev_host_built = true;
    }
    parent_lock.unlock();
    hp.mark("derive tables");
    const tgx_status fst = finish_model_create(m, bytes.data(), offs.data(), scores, n_keep, parent->device, flags, out);
    hp.mark("finish (device tables)");
    return fst;
}

// tgx_prune_alternatives over the model's own double-array (the prune driver has a model of the same vocabulary
// at hand: no second table is built)
tgx_status tgx_model_prune_alternatives(const tgx_model* m, uint8_t* always_keep, uint32_t* alt_offs, uint32_t** alt_ids) {
    if (!m) return fail(TGX_ERR_INVALID, "tgx_model_prune_alternatives: NULL argument");
    return (tgx_status)tgx_prune_alternatives_flat(&m->flat, m->vocab_bytes.data(), m->vocab_offs.data(), m->vocab_scores.data(),
                                                   m->vocab_size, always_keep, alt_offs, alt_ids);
}

void tgx_model_destroy(tgx_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (int i = 0; i < kMaxTimed; i++) {
        if (m->timed[i].start) (void)hipEventDestroy(m->timed[i].start);
        if (m->timed[i].stop) (void)hipEventDestroy(m->timed[i].stop);
    }
    if (m->d_trie) (void)hipFree(m->d_trie);
    if (m->d_trie_rev) (void)hipFree(m->d_trie_rev);
    if (m->d_trie_w) (void)hipFree(m->d_trie_w);
    if (m->d_trie_rev_w) (void)hipFree(m->d_trie_rev_w);
    if (m->d_tokhash) (void)hipFree(m->d_tokhash);
    if (m->d_trie8) (void)hipFree(m->d_trie8);
    if (m->d_top8) (void)hipFree(m->d_top8);
    if (m->d_values) (void)hipFree(m->d_values);
    if (m->d_tokid) (void)hipFree(m->d_tokid);
    if (m->d_ctrl) (void)hipFree(m->d_ctrl);
    if (m->h_ctrl) (void)hipHostFree(m->h_ctrl);
    if (m->d_wvalues) (void)hipFree(m->d_wvalues);
    if (m->d_trie8t) (void)hipFree(m->d_trie8t);
    if (m->d_wtab) (void)hipFree(m->d_wtab);
    if (m->d_dec_len) (void)hipFree(m->d_dec_len);
    if (m->d_dec_slots) (void)hipFree(m->d_dec_slots);
    if (m->d_dec_bytes) (void)hipFree(m->d_dec_bytes);
    if (m->d_dec_offs) (void)hipFree(m->d_dec_offs);
    if (m->d_span_words) (void)hipFree(m->d_span_words);
    if (m->stream2) (void)hipStreamDestroy(m->stream2);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->h_started) (void)hipHostFree(m->h_started);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

uint32_t tgx_model_vocab_size(const tgx_model* m) { return m ? m->vocab_size : 0; }
uint32_t tgx_model_max_token_len(const tgx_model* m) { return m ? m->flat.max_token_len : 0; }
uint64_t tgx_model_trie_bytes(const tgx_model* m) {
    return m ? (uint64_t)m->flat.table.size() * sizeof(tgx::TrieRec) : 0;
}
int tgx_model_device(const tgx_model* m) { return m ? m->device : -1; }

tgx_status tgx_common_prefix_search(const tgx_model* m, const uint8_t* s, uint64_t n, uint32_t* ids,
                                    uint32_t* lens, uint64_t cap, uint64_t* count) {
    if (!m || !count) return fail(TGX_ERR_INVALID, "tgx_common_prefix_search: NULL argument");
    *count = tgx::flat_common_prefix_search(m->flat, s, n, ids, lens, cap);
    return TGX_OK;
}

// ---- host-only trie introspection ----------------------------------------------


tgx_status tgx_flat_trie_build(const uint8_t* bytes, const uint64_t* offs, const double* scores,
                               uint32_t vocab_size, tgx_flat_trie** out) {
    if (!out) return fail(TGX_ERR_INVALID, "tgx_flat_trie_build: out is NULL");
    static const uint64_t zero_offs[1] = {0};
    tgx_flat_trie* t = new tgx_flat_trie();
    tgx::build_flat_trie(bytes, vocab_size ? offs : zero_offs, scores, vocab_size, &t->flat);
    *out = t;
    return TGX_OK;
}
void tgx_flat_trie_free(tgx_flat_trie* t) { delete t; }
uint64_t tgx_flat_trie_search(const tgx_flat_trie* t, const uint8_t* s, uint64_t n, uint32_t* ids,
                              uint32_t* lens, uint64_t cap) {
    return t ? tgx::flat_common_prefix_search(t->flat, s, n, ids, lens, cap) : 0;
}
uint64_t tgx_flat_trie_search8(const tgx_flat_trie* t, const uint8_t* bytes, const uint64_t* offs, const double* scores,
                               uint32_t max_hot, const uint8_t* s, uint64_t n, uint32_t* ids, uint32_t* lens,
                               uint64_t cap, uint32_t* n_hot, uint64_t* n_cold, double* hot_coverage) {
    if (!t) return ~0ULL;
    static const uint64_t zero_offs[1] = {0};
    // (test infrastructure: the records are built on first use and kept on the handle)
    tgx_flat_trie* tm = const_cast<tgx_flat_trie*>(t);
    if (!tm->t8) {
        tm->t8.reset(new tgx::Trie8());
        tgx::build_trie8(t->flat, offs ? offs : zero_offs, scores, tm->t8.get());
    }
    const tgx::Trie8& t8 = *tm->t8;
    (void)bytes;
    if (!t8.ok) return ~0ULL;  // more than 65 535 distinct score values (or more than 2^21 slots): no 8-byte records
    const uint32_t n_values = (uint32_t)t8.values.size() - 1u, k = std::min(max_hot, n_values);
    if (n_hot) *n_hot = k;
    if (n_cold) {
        uint64_t c = 0;
        for (const tgx::Trie8Rec& q : t8.rec) c += (q.sref & tgx::kTrie8RankMask) > k ? 1 : 0;
        *n_cold = c;
    }
    if (hot_coverage) *hot_coverage = t8.coverage[k];
    return tgx::trie8_common_prefix_search(t8, t->flat, s, n, ids, lens, cap);
}
void tgx_flat_trie_stats(const tgx_flat_trie* t, uint64_t* n_slots, uint64_t* n_nodes,
                         uint32_t* max_token_len) {
    if (!t) return;
    if (n_slots) *n_slots = t->flat.table.size();
    if (n_nodes) *n_nodes = t->flat.n_nodes;
    if (max_token_len) *max_token_len = t->flat.max_token_len;
}
tgx_status tgx_tok_hash_selftest(const uint8_t* bytes, const uint64_t* offs, uint32_t vocab_size, uint32_t* seed,
                                 uint64_t* mismatches) {
    if (!offs || !mismatches) return TGX_ERR_INVALID;
    tgx::TokHashTable t;
    tgx::build_tok_hash(bytes, offs, vocab_size, &t);
    if (!t.ok) return TGX_ERR_UNSUPPORTED;
    if (seed) *seed = t.seed;
    // the id a lookup must give: the LAST vocabulary entry with these bytes (src/trie.rs:19)
    uint64_t bad = 0;
    for (uint32_t id = 0; id < vocab_size; id++) {
        const uint32_t len = (uint32_t)(offs[id + 1] - offs[id]);
        if (len == 0) continue;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(w, bytes + offs[id], len);
        const uint64_t h = tgx::tok_hash64_long(w, len, t.seed);
        uint32_t i = (uint32_t)h & t.mask;
        bool found = false;
        for (uint32_t probe = 0; probe <= t.mask; probe++) {  // the device loop of trace_kernel
            const tgx::TokHashEntry& e = t.slots[i];
            if (!e.used) break;
            if (e.hash == h) {
                const uint32_t o = e.id;
                found = offs[o + 1] - offs[o] == len && memcmp(bytes + offs[o], bytes + offs[id], len) == 0 && o >= id;
                break;
            }
            i = (i + 1) & t.mask;
        }
        if (!found) bad++;
    }
    *mismatches = bad;
    return TGX_OK;
}
void tgx_flat_trie_copy(const tgx_flat_trie* t, uint32_t* check, uint32_t* base_flags, uint32_t* tokid) {
    if (!t) return;
    for (size_t i = 0; i < t->flat.table.size(); i++) {
        if (check) check[i] = t->flat.table[i].check;
        if (base_flags) base_flags[i] = t->flat.table[i].base;
        if (tokid) tokid[i] = t->flat.tokid[i];
    }
}
double tgx_dropout_u01_host(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len) {
    return tgx_dropout_u01(seed, sample, pos, len);
}

// ---- corpus ------------------------------------------------------------------

// Host <-> device copies of corpora and results go through two streams of their own per device (one per
// direction): synchronous hipMemcpy calls all share the null stream, so an upload from one thread and a download
// from another took turns on it instead of using the link in both directions (profiles/r02: e2e timeline).
static hipStream_t copy_stream(int device, int dir) {
    static std::mutex mu;
    static hipStream_t streams[64][2] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!streams[device][dir]) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;  // the null stream: correct, only slower
        }
        streams[device][dir] = st;
    }
    return streams[device][dir];
}
hipError_t tgx::dev::copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, int device) {
    hipStream_t st = copy_stream(device, kind == hipMemcpyHostToDevice ? 0 : 1);
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

// A resident corpus over `text` (host memory, memory of `device`, or bytes the caller writes to d_text itself once this
// has returned: text is then not read) and host offsets: what tgx_corpus_upload, tgx_corpus_from_text and
// tgx_corpus_split_specials share, so the three build the same corpus.
tgx_status tgx::dev::corpus_create(const char* who, int device, const uint8_t* text, TextFrom from, const uint64_t* offs,
                                   uint64_t n_samples, tgx_corpus** out) {
    if (!out) return fail(TGX_ERR_INVALID, "%s: out is NULL", who);
    *out = nullptr;
    if (n_samples && !offs) return fail(TGX_ERR_INVALID, "%s: offs is NULL", who);
    int ndev = 0;
    if (const tgx_status dst = require_device(&ndev)) return dst;
    if (device < 0 || device >= ndev)
        return fail(TGX_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
    if (n_samples >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "more than 2^32-1 samples");
    const uint64_t base = n_samples ? offs[0] : 0;
    for (uint64_t i = 0; i < n_samples; i++) {
        if (offs[i + 1] < offs[i]) return fail(TGX_ERR_INVALID, "offsets not monotone at %llu",
                                               (unsigned long long)i);
        if (offs[i + 1] - offs[i] >= 0xFFFFFF00ull)
            return fail(TGX_ERR_UNSUPPORTED, "sample %llu is 4 GiB or longer", (unsigned long long)i);
    }
    std::unique_ptr<tgx_corpus> c(new tgx_corpus());
    c->device = device;
    c->n_samples = n_samples;
    c->n_bytes = n_samples ? offs[n_samples] - base : 0;
    c->h_offs.resize(n_samples + 1);
    for (uint64_t i = 0; i <= n_samples; i++) c->h_offs[i] = n_samples ? offs[i] - base : 0;
    if (n_samples && c->n_bytes && !text && from != TextFrom::Caller) return fail(TGX_ERR_INVALID, "%s: text is NULL", who);
    // longest first: the tail of a pass is then made of short samples
    std::vector<uint32_t> order(n_samples);
    std::iota(order.begin(), order.end(), 0u);
    const uint64_t* ho = c->h_offs.data();
    std::stable_sort(order.begin(), order.end(), [ho](uint32_t a, uint32_t b) {
        return ho[a + 1] - ho[a] > ho[b + 1] - ho[b];
    });

    c->max_len = n_samples ? ho[order[0] + 1] - ho[order[0]] : 0;
    c->h_sorted_len.resize(n_samples);
    c->h_sorted_cum.resize(n_samples);
    for (uint64_t i = 0, run = 0; i < n_samples; i++) {
        c->h_sorted_len[i] = (uint32_t)(ho[order[i] + 1] - ho[order[i]]);
        run += c->h_sorted_len[i];
        c->h_sorted_cum[i] = run;
    }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(c->d_text_alloc.alloc(device, (size_t)c->n_bytes + 512));
    c->d_text = c->d_text_alloc + 256;
    HIP_TRY(hipMemset(c->d_text_alloc, 0, 256));
    HIP_TRY(c->d_offs.alloc(device, (size_t)(n_samples + 1) * 8));
    HIP_TRY(c->d_order.alloc(device, (size_t)n_samples * 4 + 4));
    if (c->n_bytes && from != TextFrom::Caller)
        HIP_TRY(copy_sync(c->d_text, text + base, c->n_bytes, from == TextFrom::Device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, device));
    HIP_TRY(hipMemset(c->d_text + c->n_bytes, 0, 256));
    HIP_TRY(hipMemcpy(c->d_offs, c->h_offs.data(), (n_samples + 1) * 8, hipMemcpyHostToDevice));
    if (n_samples) HIP_TRY(hipMemcpy(c->d_order, order.data(), n_samples * 4, hipMemcpyHostToDevice));
    *out = c.release();
    return TGX_OK;
}

tgx_status tgx_corpus_upload(int device, const uint8_t* text, const uint64_t* offs,
                             uint64_t n_samples, tgx_corpus** out) {
    return corpus_create("tgx_corpus_upload", device, text, TextFrom::Host, offs, n_samples, out);
}

// (every pass has finished with the corpus's buffers when it returns: they go straight back to the pool)
void tgx_corpus_free(tgx_corpus* c) { delete c; }

uint64_t tgx_corpus_num_samples(const tgx_corpus* c) { return c ? c->n_samples : 0; }
uint64_t tgx_corpus_num_bytes(const tgx_corpus* c) { return c ? c->n_bytes : 0; }

uint64_t tgx_result_num_samples(const tgx_result* r) { return r ? r->n_samples : 0; }
uint64_t tgx_result_num_tokens(const tgx_result* r) { return r ? r->n_tokens : 0; }

const uint32_t* tgx_result_ids(tgx_result* r) {
    if (!r) return nullptr;
    if (!r->have_ids) {
        r->h_ids.reset(new (std::nothrow) uint32_t[r->n_tokens ? r->n_tokens : 1]);
        if (!r->h_ids) {
            fail(TGX_ERR_DEVICE, "out of host memory (ids)");
            return nullptr;
        }
        if (r->n_tokens) {
            (void)hipSetDevice(r->device);
            if (hipMemcpy(r->h_ids.get(), r->d_ids, r->n_tokens * 4, hipMemcpyDeviceToHost) != hipSuccess) {
                fail(TGX_ERR_DEVICE, "D2H copy of ids failed");
                return nullptr;
            }
        }
        r->have_ids = true;
    }
    return r->h_ids.get();
}

const uint64_t* tgx_result_offsets(tgx_result* r) {
    if (!r) return nullptr;
    if (!r->have_offs) {
        r->h_offs.resize(r->n_samples + 1);
        (void)hipSetDevice(r->device);
        if (hipMemcpy(r->h_offs.data(), r->d_offs, (r->n_samples + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            fail(TGX_ERR_DEVICE, "D2H copy of offsets failed");
            return nullptr;
        }
        r->have_offs = true;
    }
    return r->h_offs.data();
}

tgx_status tgx_result_copy_ids(const tgx_result* r, uint32_t* dst, uint64_t cap) {
    if (!r || (!dst && r->n_tokens)) return fail(TGX_ERR_INVALID, "tgx_result_copy_ids: NULL argument");
    if (cap < r->n_tokens) return fail(TGX_ERR_INVALID, "tgx_result_copy_ids: %llu ids, room for %llu", (unsigned long long)r->n_tokens, (unsigned long long)cap);
    if (!r->n_tokens) return TGX_OK;
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(copy_sync(dst, r->d_ids, r->n_tokens * 4, hipMemcpyDeviceToHost, r->device));
    return TGX_OK;
}

tgx_status tgx_result_copy_offsets(const tgx_result* r, uint64_t* dst, uint64_t cap) {
    if (!r || !dst) return fail(TGX_ERR_INVALID, "tgx_result_copy_offsets: NULL argument");
    if (cap < r->n_samples + 1) return fail(TGX_ERR_INVALID, "tgx_result_copy_offsets: %llu offsets, room for %llu", (unsigned long long)(r->n_samples + 1), (unsigned long long)cap);
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(copy_sync(dst, r->d_offs, (r->n_samples + 1) * 8, hipMemcpyDeviceToHost, r->device));
    return TGX_OK;
}

const void* tgx_result_ids_device(const tgx_result* r) { return r ? r->d_ids.get() : nullptr; }
const void* tgx_result_offsets_device(const tgx_result* r) { return r ? r->d_offs.get() : nullptr; }

void tgx_result_free(tgx_result* r) { delete r; }
int tgx_result_device(const tgx_result* r) { return r ? r->device : -1; }
uint32_t tgx_result_vocab_size(const tgx_result* r) { return r ? r->vocab_size : 0; }

// ---- what the calls on a caller's stream share (device_internal.h; result_ops.cpp, corpus_ops.cpp) -----------------

namespace tgx::dev {

// What a caller gets when it passes no stream of its own: one per device.  It is a BLOCKING stream (hipStreamDefault),
// so what is queued on it starts after everything queued earlier on the device's null stream, which is where a
// caller that "has no stream" has its work (torch's default stream is the null stream, handle 0).
hipStream_t stream_or_default(void* stream, int device) {
    if (stream) return static_cast<hipStream_t>(stream);
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!streams[device]) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamDefault) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;  // the null stream itself: ordered the same way
        }
        streams[device] = st;
    }
    return streams[device];
}

// p (may be NULL when optional) must be device memory of `device`, which is the current device and that of `owner`
// ("result" or "model")
tgx_status check_device_ptr(const char* who, const char* what, const void* p, int device, const char* owner) {
    if (!p) return TGX_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TGX_ERR_INVALID, "%s: %s is not device memory", who, what);
    }
    if (attr.type != hipMemoryTypeDevice) return fail(TGX_ERR_INVALID, "%s: %s is not device memory", who, what);
    if (attr.device != device) return fail(TGX_ERR_INVALID, "%s: %s is on device %d, the %s on device %d", who, what, attr.device, owner, device);
    return TGX_OK;
}

int stage_times(const char* const* stage_names, const float* stage_ms, int n, const char** names, float* ms, int cap) {
    int k = 0;
    for (; k < n && k < cap; k++) {
        if (names) names[k] = stage_names[k];
        if (ms) ms[k] = stage_ms[k];
    }
    return k;
}

tgx_status read_u64(hipStream_t hs, const void* d_src, void* host_words, size_t n) {
    HIP_TRY(hipMemcpyAsync(host_words, d_src, n * 8, hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    return TGX_OK;
}

namespace {
template <class Guard>
tgx_status scan_room_of(ScanScratch* s, Guard& guard, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n, const char* oom) {
    if (s->ptr && n <= s->n) return TGX_OK;
    if (temp_bytes(n, &s->bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan temp-size query failed");
    const hipError_t e = guard.alloc(s->bytes, &s->ptr);  // (never NULL: that asks the scan for its size)
    if (e != hipSuccess && oom) return fail(TGX_ERR_DEVICE, "%s", oom);
    HIP_TRY(e);
    s->n = n;
    return TGX_OK;
}
}  // namespace
tgx_status scan_room(ScanScratch* s, StreamGuard& guard, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n, const char* oom) {
    return scan_room_of(s, guard, temp_bytes, n, oom);
}
tgx_status scan_room(ScanScratch* s, Pass& pass, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n, const char* oom) {
    return scan_room_of(s, pass, temp_bytes, n, oom);
}

}  // namespace tgx::dev

// ---- frequency pass ------------------------------------------------------------

tgx_status tgx_count_tokens(tgx_model* m, tgx_corpus* c, uint64_t* freq) {
    if (!m || !c || !freq) return fail(TGX_ERR_INVALID, "tgx_count_tokens: NULL argument");
    if (m->device != c->device) return fail(TGX_ERR_INVALID, "model and corpus on different devices");
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkc(c->mu);
    // model.encode(sample, 0.0) for every sample (src/prune.rs:218), then a histogram of the ids: per-block LDS
    // histograms when the vocabulary's counters fit a block's LDS, radix sort + run-length encode otherwise
    tgx_result* r = nullptr;
    tgx_status st = encode_corpus_locked(m, c, 0.0, 0, &r);
    if (st != TGX_OK) return st;
    Pass pass(m);
    pass.adopt_result(r);
    const uint64_t T = r->n_tokens;
    if (T >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "frequency pass over more than 2^32-1 tokens per call");
    if (T && m->vocab_size <= tgx::kHistMaxVocab && !knob("TGX_FREQ_SORT")) {
        // the vocabulary's counters fit a block's LDS: one private histogram per block (pairs.hip)
        unsigned long long* d_hist = nullptr;
        const size_t hb = (size_t)m->vocab_size * 8 + 256;
        if (pass.alloc(hb, &d_hist) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (frequency pass)");
        if (hipMemsetAsync(d_hist, 0, hb, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "memset failed");
        time_begin(m, "ids_histogram_kernel");
        if (tgx::launch_ids_histogram(r->d_ids, T, m->vocab_size, d_hist, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "histogram launch failed");
        time_end(m);
        std::vector<unsigned long long> hh(m->vocab_size);
        if (hipMemcpyAsync(hh.data(), d_hist, (size_t)m->vocab_size * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "frequency pass failed: %s", hipGetErrorString(hipGetLastError()));
        for (uint32_t i = 0; i < m->vocab_size; i++) freq[i] += hh[i];
        m->last_alg_bytes = c->n_bytes + 8 * (c->n_samples + 1) + 8ull * m->vocab_size;
        return pass.done();
    }
    uint32_t *d_sorted = nullptr, *d_unique = nullptr;
    unsigned int *d_cnt = nullptr, *d_runs = nullptr;
    void* d_temp = nullptr;
    size_t tb1 = 0, tb2 = 0;
    const size_t kb = (size_t)T * 4 + 256;
    if (T == 0) return pass.done();
    if (tgx::ids_sort_temp_bytes(T, &tb1) != hipSuccess || tgx::ids_rle_temp_bytes(T, &tb2) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "rocPRIM temp-size query failed");
    if (pass.alloc(kb, &d_sorted) != hipSuccess || pass.alloc(kb, &d_unique) != hipSuccess || pass.alloc(kb, &d_cnt) != hipSuccess ||
        pass.alloc(256, &d_runs) != hipSuccess || pass.alloc(std::max(tb1, tb2) + 256, &d_temp) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (frequency pass)");
    unsigned int end_bit = 1;
    while (end_bit < 32 && (1ull << end_bit) < (uint64_t)m->vocab_size) end_bit++;
    time_begin(m, "ids_sort+rle");
    if (tgx::ids_sort(d_temp, tb1, r->d_ids, d_sorted, T, end_bit, m->stream) != hipSuccess ||
        tgx::ids_rle(d_temp, tb2, d_sorted, T, d_unique, d_cnt, d_runs, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "id sort / run-length encode failed");
    time_end(m);
    unsigned int runs = 0;
    if (hipMemcpyAsync(&runs, d_runs, 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "frequency pass failed: %s", hipGetErrorString(hipGetLastError()));
    std::vector<uint32_t> hu(runs ? runs : 1);
    std::vector<unsigned int> hc(runs ? runs : 1);
    if (runs && (hipMemcpy(hu.data(), d_unique, (size_t)runs * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(hc.data(), d_cnt, (size_t)runs * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "D2H copy of the histogram failed");
    for (unsigned int i = 0; i < runs; i++)
        if (hu[i] < m->vocab_size) freq[hu[i]] += hc[i];
    m->last_alg_bytes = c->n_bytes + 8 * (c->n_samples + 1) + 8ull * m->vocab_size;
    return pass.done();
}

// max_pairs == 0: the whole table in ascending key order (tgx_count_pairs); otherwise the max_pairs most
// frequent pairs, by descending count and ascending key among equal counts (tgx_count_pairs_top)
static tgx_status count_pairs_impl(tgx_model* m, tgx_corpus* c, uint64_t max_pairs, uint64_t** keys, uint64_t** counts,
                                   uint64_t* n_pairs, uint64_t* n_total) {
    if (!m || !c || !keys || !counts || !n_pairs) return fail(TGX_ERR_INVALID, "tgx_count_pairs: NULL argument");
    *keys = *counts = nullptr;
    *n_pairs = 0;
    if (n_total) *n_total = 0;
    if (m->device != c->device) return fail(TGX_ERR_INVALID, "model and corpus on different devices");
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkc(c->mu);
    tgx_result* r = nullptr;
    tgx_status st = encode_corpus_locked(m, c, 0.0, 0, &r);  // model.encode(sample, 0.0), merge.rs:58
    if (st != TGX_OK) return st;
    Pass pass(m);
    pass.adopt_result(r);
    const uint64_t T = r->n_tokens, S = r->n_samples;
    if (T >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "pair scan over more than 2^32-1 tokens per pass");
    unsigned long long *d_keys = nullptr, *d_sorted = nullptr, *d_unique = nullptr;
    unsigned int *d_cnt = nullptr, *d_runs = nullptr;
    void* d_temp = nullptr;
    size_t tb1 = 0, tb2 = 0;
    const size_t kb = (size_t)T * 8 + 256, cb = (size_t)T * 4 + 256;
    if (T == 0) {
        // no token at all (no sample, or only empty ones): an empty table, in malloc'd arrays like every other
        *keys = (uint64_t*)malloc(sizeof(uint64_t));
        *counts = (uint64_t*)malloc(sizeof(uint64_t));
        if (!*keys || !*counts) {
            free(*keys);
            free(*counts);
            *keys = *counts = nullptr;
            return fail(TGX_ERR_DEVICE, "out of host memory (pair table of 0 entries)");
        }
        return pass.done();
    }
    if (tgx::pair_sort_temp_bytes(T, &tb1) != hipSuccess || tgx::pair_rle_temp_bytes(T, &tb2) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "rocPRIM temp-size query failed");
    if (pass.alloc(kb, &d_keys) != hipSuccess || pass.alloc(kb, &d_sorted) != hipSuccess || pass.alloc(kb, &d_unique) != hipSuccess ||
        pass.alloc(cb, &d_cnt) != hipSuccess || pass.alloc(256, &d_runs) != hipSuccess || pass.alloc(std::max(tb1, tb2) + 256, &d_temp) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (pair scan)");
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((S + 3) / 4, (uint64_t)m->num_cus * 8));
    // pair keys of 2 shift (+ 1 for the sentinel) bits, shift = bits of the largest id; widened to the API's
    // (a << 32) | b on the host
    uint32_t shift = 1;
    while (shift < 32 && (1ull << shift) < (unsigned long long)m->vocab_size) shift++;
    const unsigned long long sentinel = shift < 32 ? (1ull << (2 * shift)) : ~0ULL;
    const unsigned int end_bit = shift < 32 ? 2 * shift + 1 : 64;
    time_begin(m, "pair_keys_kernel");
    if (tgx::launch_pair_keys(r->d_ids, r->d_offs, S, shift, sentinel, d_keys, blocks, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "pair key launch failed");
    time_end(m);
    time_begin(m, "pair_sort+rle");
    if (tgx::pair_sort(d_temp, tb1, d_keys, d_sorted, T, end_bit, m->stream) != hipSuccess ||
        tgx::pair_rle(d_temp, tb2, d_sorted, T, d_unique, d_cnt, d_runs, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "pair sort / run-length encode failed");
    time_end(m);
    unsigned int runs = 0;
    if (hipMemcpyAsync(&runs, d_runs, 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "pair scan failed: %s", hipGetErrorString(hipGetLastError()));
    // the sentinel run (one per non-empty sample) has the largest key: it is the last run
    unsigned long long last_key = 0;
    if (runs && hipMemcpy(&last_key, d_unique + (runs - 1), 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "D2H copy failed");
    if (runs && last_key == sentinel) runs--;
    const unsigned long long* src_keys = d_unique;
    const unsigned int* src_cnt = d_cnt;
    if (n_total) *n_total = runs;
    if (max_pairs && runs) {
        // order by count on the device and hand back the head only: the merge loop looks at a few hundred
        // candidates of a table of millions (src/merge.rs:84-126)
        size_t tb3 = 0;
        if (tgx::pair_count_sort_temp_bytes(runs, &tb3) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "rocPRIM temp-size query failed");
        void* d_temp3 = nullptr;
        if (pass.alloc(tb3 + 256, &d_temp3) != hipSuccess) return fail(TGX_ERR_DEVICE, "out of device memory (pair scan)");
        unsigned int* cnt_out = reinterpret_cast<unsigned int*>(d_sorted);  // the sorted keys are no longer needed
        time_begin(m, "pair_count_sort");
        hipError_t e3 = tgx::pair_count_sort(d_temp3, tb3, d_cnt, cnt_out, d_unique, d_keys, runs, m->stream);
        time_end(m);
        if (e3 == hipSuccess) e3 = hipStreamSynchronize(m->stream);
        if (e3 != hipSuccess) return fail(TGX_ERR_DEVICE, "pair count sort failed");
        src_keys = d_keys;
        src_cnt = cnt_out;
        runs = (unsigned int)std::min<uint64_t>(runs, max_pairs);
    }
    uint64_t* ok = (uint64_t*)malloc(sizeof(uint64_t) * (runs ? runs : 1));
    uint64_t* oc = (uint64_t*)malloc(sizeof(uint64_t) * (runs ? runs : 1));
    if (!ok || !oc) {
        free(ok);
        free(oc);
        return fail(TGX_ERR_DEVICE, "out of host memory (pair table of %llu entries)", (unsigned long long)runs);
    }
    if (!max_pairs && runs) {
        // the whole table (millions of pairs: the multi-GPU merge exchanges it): brought into the ABI's form on the
        // device and copied straight into the caller's arrays — two zero-filled staging vectors and a host loop
        // over every pair took three times the kernels' time.  d_sorted and d_keys are free by now.
        unsigned long long* ek = d_sorted;
        unsigned long long* ec = d_keys;
        if (tgx::launch_pair_expand(src_keys, src_cnt, runs, (uint32_t)shift, ek, ec, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess ||
            copy_sync(ok, ek, (size_t)runs * 8, hipMemcpyDeviceToHost, m->device) != hipSuccess ||
            copy_sync(oc, ec, (size_t)runs * 8, hipMemcpyDeviceToHost, m->device) != hipSuccess) {
            free(ok);
            free(oc);
            return fail(TGX_ERR_DEVICE, "D2H copy of pair table failed");
        }
    } else {
        std::vector<unsigned long long> hk(runs ? runs : 1);
        std::vector<unsigned int> hc(runs ? runs : 1);
        if (runs && (hipMemcpy(hk.data(), src_keys, (size_t)runs * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(hc.data(), src_cnt, (size_t)runs * 4, hipMemcpyDeviceToHost) != hipSuccess)) {
            free(ok);
            free(oc);
            return fail(TGX_ERR_DEVICE, "D2H copy of pair table failed");
        }
        const unsigned long long low = shift < 32 ? (1ull << shift) - 1 : 0xFFFFFFFFull;
        for (unsigned int i = 0; i < runs; i++) {
            ok[i] = ((hk[i] >> shift) << 32) | (hk[i] & low);
            oc[i] = hc[i];
        }
    }
    *keys = ok;
    *counts = oc;
    *n_pairs = runs;
    // N + 8(S+1) + 16P
    m->last_alg_bytes = c->n_bytes + 8 * (S + 1) + 16ull * runs;
    return pass.done();
}

tgx_status tgx_count_pairs(tgx_model* m, tgx_corpus* c, uint64_t** keys, uint64_t** counts, uint64_t* n_pairs) {
    return count_pairs_impl(m, c, 0, keys, counts, n_pairs, nullptr);
}

tgx_status tgx_count_pairs_top(tgx_model* m, tgx_corpus* c, uint64_t max_pairs, uint64_t** keys, uint64_t** counts,
                               uint64_t* n_pairs, uint64_t* n_total) {
    if (max_pairs == 0) return fail(TGX_ERR_INVALID, "tgx_count_pairs_top: max_pairs must be positive");
    return count_pairs_impl(m, c, max_pairs, keys, counts, n_pairs, n_total);
}

// ---- measurement ---------------------------------------------------------------

int tgx_last_kernel_times(const tgx_model* m, const char** names, float* ms, int cap) {
    if (!m) return 0;
    int n = 0;
    for (int i = 0; i < m->n_timed && n < cap; i++) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, m->timed[i].start, m->timed[i].stop) != hipSuccess) t = -1.f;
        if (names) names[n] = m->timed[i].name;
        if (ms) ms[n] = t;
        n++;
    }
    return n;
}

uint64_t tgx_last_algorithmic_bytes(const tgx_model* m) { return m ? m->last_alg_bytes : 0; }
uint64_t tgx_last_estep_pieces(const tgx_model* m) { return m ? m->last_estep_pieces : 0; }
uint64_t tgx_last_estep_redo(const tgx_model* m) { return m ? m->last_estep_redo : 0; }
uint32_t tgx_model_score_values(const tgx_model* m) { return m && m->have_trie8 ? m->n_values : 0u; }
