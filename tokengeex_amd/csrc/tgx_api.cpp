// C ABI (include/tgx.h) over the HIP kernels: handles, HBM buffers, launch
// sequencing, error reporting.  Host side of the reference's batch loops
// (src/tokenizer.rs:102-123, src/prune.rs:205-244); there is no CPU fallback —
// without a usable gfx950 device every compute entry point returns TGX_ERR_DEVICE.
// Here: the error state, the buffer pool, models and corpora, the encode pass and the counting passes.  The E-step is in
// estep_pass.cpp, sampling, lattice statistics and n-best in lattice_pass.cpp (pass_internal.h: what they take from
// here).  The transforms of a resident result or corpus on a caller's stream are in result_ops.cpp and corpus_ops.cpp
// (device_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <chrono>
#include <condition_variable>
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
#include "ids_in_place.h"
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

hipError_t pool_alloc(int device, size_t bytes, void** out) {
    if (bytes == 0) bytes = 256;
    bytes = (bytes + 255) & ~size_t(255);
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        size_t best = g_pool.size();
        for (size_t i = 0; i < g_pool.size(); i++) {
            const PoolEntry& e = g_pool[i];
            if (e.device != device || e.bytes < bytes || e.bytes > bytes * 2 + (1u << 20)) continue;
            if (best == g_pool.size() || e.bytes < g_pool[best].bytes) best = i;
        }
        if (best != g_pool.size()) {
            *out = g_pool[best].ptr;
            g_pool_bytes -= g_pool[best].bytes;
            g_pool.erase(g_pool.begin() + (long)best);
            return hipSuccess;
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

// encode5_kernel: the depth at which a trip's live walks are compacted (0: never; TGX_E5_COMPACT=off|4..8 overrides)
constexpr int kE5CompactDepth = 5;

int usable_device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

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

}  // namespace

namespace tgx::dev {

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

// ---- what the passes share (pass_internal.h; estep_pass.cpp, lattice_pass.cpp) -------------------------------------

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

namespace {

uint32_t grid_blocks(const tgx_model* m, uint64_t n_samples) {
    const uint64_t wpb = tgx::encode_waves_per_block(m->lm);
    uint64_t want = (n_samples + wpb - 1) / wpb;
    uint64_t cap = (uint64_t)m->num_cus * (uint64_t)std::max(1, m->blocks_per_cu);
    return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

// encode5_kernel keeps the first ranks of the score values in LDS.  build_trie8 ranks a value by the probability mass of
// its tokens — how often they are CHOSEN — but a value is read whenever one of its tokens MATCHES: a vocabulary after an
// M-step has a value per token, and its kept single-byte tokens have tiny scores and match at every position.  So, as
// for the E-step's ranks (ensure_estep_trie8t), the first time a model with more values than fit LDS meets text the
// values are re-ranked by match counts over a sample of it (value_count_kernel, 4 MiB): the records' ranks are remapped on
// the device, the value table(s) permuted.  Caller holds m->mu.
tgx_status ensure_value_ranks(tgx_model* m, const tgx_corpus* c) {
    if (m->values_ranked || !m->have_trie8 || !c->n_bytes) return TGX_OK;
    m->values_ranked = true;
    const char* vr = knob("TGX_VALUE_RANK");  // "model": keep build_trie8's order; "counts": re-rank even when every value fits (measurements, tests)
    if (vr && strcmp(vr, "model") == 0) return TGX_OK;
    if (m->n_values <= tgx::encode5_max_hot(false, 13, 3, 160u * 1024u) && !(vr && strcmp(vr, "counts") == 0)) return TGX_OK;  // (every value in LDS anyway)
    tgx::HostPhases hp("ensure_value_ranks");
    HIP_TRY(hipSetDevice(m->device));
    const uint32_t nv = m->n_values, chunk = 65536u;
    const uint64_t stride = std::max<uint64_t>(chunk, (c->n_bytes + 63) / 64);
    const size_t cb = ((size_t)nv + 1) * 4 + 256;
    Pass pass(m);
    unsigned int* d_cnt = nullptr;
    uint32_t* d_perm = nullptr;
    if (pass.alloc(cb, &d_cnt) != hipSuccess || pass.alloc(cb, &d_perm) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (value counts)");
    std::vector<unsigned int> cnt((size_t)nv + 1, 0u);
    std::vector<double> values((size_t)nv + 1), wvalues;
    bool ok = hipMemsetAsync(d_cnt, 0, cb, m->stream) == hipSuccess &&
              tgx::launch_value_count(c->d_text, c->n_bytes, chunk, stride, m->d_trie8, (uint32_t)m->flat.table.size(), m->root_base8, nv,
                                      std::max<uint32_t>(1, m->flat.max_token_len), d_cnt, (uint32_t)m->num_cus, m->stream) == hipSuccess &&
              hipMemcpyAsync(cnt.data(), d_cnt, ((size_t)nv + 1) * 4, hipMemcpyDeviceToHost, m->stream) == hipSuccess &&
              hipMemcpyAsync(values.data(), m->d_values, ((size_t)nv + 1) * 8, hipMemcpyDeviceToHost, m->stream) == hipSuccess;
    if (ok && m->have_wvalues) {
        wvalues.resize((size_t)nv + 1);
        ok = hipMemcpyAsync(wvalues.data(), m->d_wvalues, ((size_t)nv + 1) * 8, hipMemcpyDeviceToHost, m->stream) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "value count pass failed: %s", hipGetErrorString(hipGetLastError()));
    hp.mark("value counts");
    std::vector<uint32_t> order(nv);
    for (uint32_t r = 0; r < nv; r++) order[r] = r + 1u;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cnt[a] > cnt[b]; });  // ties: the old order
    std::vector<uint32_t> perm((size_t)nv + 1, 0u);
    std::vector<double> v2((size_t)nv + 1), w2(wvalues.size());
    v2[0] = values[0];
    if (!w2.empty()) w2[0] = wvalues[0];
    unsigned long long total = 0, run = 0;
    for (uint32_t r = 0; r < nv; r++) total += cnt[order[r]];
    std::vector<double> cov((size_t)nv + 1, 0.0);
    for (uint32_t r = 0; r < nv; r++) {
        perm[order[r]] = r + 1u;
        v2[r + 1u] = values[order[r]];
        if (!w2.empty()) w2[r + 1u] = wvalues[order[r]];
        run += cnt[order[r]];
        cov[r + 1u] = total ? (double)run / (double)total : 1.0;
    }
    cov[nv] = 1.0;
    ok = hipMemcpyAsync(d_perm, perm.data(), ((size_t)nv + 1) * 4, hipMemcpyHostToDevice, m->stream) == hipSuccess &&
         tgx::launch_rank_remap(m->d_trie8, (uint32_t)m->flat.table.size(), d_perm, m->stream) == hipSuccess &&
         hipMemcpyAsync(m->d_values, v2.data(), ((size_t)nv + 1) * 8, hipMemcpyHostToDevice, m->stream) == hipSuccess &&
         (w2.empty() || hipMemcpyAsync(m->d_wvalues, w2.data(), ((size_t)nv + 1) * 8, hipMemcpyHostToDevice, m->stream) == hipSuccess) &&
         hipStreamSynchronize(m->stream) == hipSuccess;
    if (!ok) return fail(TGX_ERR_DEVICE, "value re-rank failed: %s", hipGetErrorString(hipGetLastError()));
    m->value_coverage = std::move(cov);
    hp.mark("re-rank");
    return pass.done();
}

}  // namespace

namespace tgx::dev {

// What every encode and sampling kernel is told about the model, the corpus and its scratch (ensure_scratch); dropout,
// flags and the kernel's own fields are the caller's.
tgx::EncodeParams base_encode_params(const tgx_model* m, const tgx_corpus* c, uint64_t seed) {
    tgx::EncodeParams p{};
    p.text = c->d_text;
    p.offs = c->d_offs;
    p.order = c->d_order;
    p.n_samples = c->n_samples;
    p.trie = m->d_trie;
    p.tokid = m->d_tokid;
    p.root_base = m->flat.table[0].base & ~tgx::kTerminalBit;
    p.lm = m->lm;
    p.n_slots = (uint32_t)m->flat.table.size();
    p.bp = c->d_bp;
    p.tmp = c->d_tmp;
    p.counts = c->d_counts;
    p.status = c->d_status;
    p.bp8 = reinterpret_cast<uint8_t*>(c->d_bp.get());  // the rows4 path uses the scratch row as bytes
    p.tokhash = m->d_tokhash;
    p.tokhash_mask = m->tokhash.mask;
    p.tokhash_seed = m->tokhash.seed;
    p.err_sample = &m->d_ctrl->err;
    p.queue = &m->d_ctrl->queue;
    p.seed = seed;
    // samples of less than 2 KiB on average: the trace keeps its waiting tokens across samples (trace_body.h; 140-byte samples
    // 5.5 -> 4.6 ms per GiB, 9 KiB samples 2.93 -> 3.04)
    p.trace_carry = (c->n_samples && c->n_bytes / c->n_samples < 2048) ? 1u : 0u;
    p.trace_stride = tgx::kTraceStride;
    return p;
}

tgx_status check_no_path(tgx_model* m, const tgx_corpus* c) {
    unsigned long long bad = m->h_ctrl->err;
    if (bad == ~0ULL) return TGX_OK;
    if (bad & tgx::kErrCorruptBp)
        return fail(TGX_ERR_DEVICE, "internal error: corrupt back-pointer (sample or text byte %llu)",
                    (unsigned long long)(bad & ~tgx::kErrCorruptBp));
    if (bad & tgx::kErrCountMismatch)  // (the in-place trace's self-check: ids_in_place.h)
        return fail(TGX_ERR_DEVICE, "internal error: the token count of sample %llu differs between the relaxation and the trace",
                    (unsigned long long)(bad & ~tgx::kErrCountMismatch));
    uint64_t n = c->h_offs[bad + 1] - c->h_offs[bad];
    set_error_detail(bad, n, n);
    // Display of Error::NoPath, reference src/lib.rs:243-245
    return fail(TGX_ERR_NO_PATH, "no path to position %llu/%llu", (unsigned long long)n,
                (unsigned long long)n);
}

}  // namespace tgx::dev

namespace {

// The samples whose wave ran out of list entries for long matches (encode4l_kernel, the LONG build of encode5_kernel:
// p.redo_count, the list in c->d_counts) go to encode2_kernel.  Waits for the kernel that filled the list.
tgx_status redo_long_matches(tgx_model* m, tgx_corpus* c, const tgx::EncodeParams& p) {
    unsigned long long n_redo = 0;
    HIP_TRY(hipMemcpyAsync(&n_redo, &m->d_ctrl->encode_redo, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (n_redo > c->n_samples) return fail(TGX_ERR_DEVICE, "redo list longer than the batch");
    m->last_redo_samples = n_redo;
    if (n_redo) {
        tgx::EncodeParams q = p;
        q.order = c->d_counts;
        q.n_samples = n_redo;
        HIP_TRY(hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream));  // the work queue
        time_begin(m, "encode2_kernel");
        HIP_TRY(tgx::launch_encode2(q, (uint32_t)m->num_cus, true, m->stream));
        time_end(m);
    }
    return TGX_OK;
}

tgx_status scan_ids_offsets(tgx_model* m, tgx_corpus* c, tgx_result* r, const char* what, bool with_err);

// Queues the encode kernels and the back-trace over the corpus: every sample's token count in c->d_counts, its ids
// right-aligned in c->d_tmp, the lowest failing sample in d_ctrl->err.  Diagnostic scratch belongs to `pass`.
// A pass that can (ids_in_place.h) writes the ids in place instead: encode5_kernel leaves the counts,
// they are scanned into r's offsets, the host waits once for the total and sizes r's ids, and the trace writes them
// there.  m->last_ids_in_place tells the caller, which then has neither scan nor compaction left to do: it reads
// d_ctrl->err once the trace is through.
tgx_status run_encode_kernel(tgx_model* m, tgx_corpus* c, double dropout, uint64_t seed, Pass& pass, tgx_result* r) {
    m->last_ids_in_place = false;
    tgx_status st = ensure_scratch(c, false);  // (`tmp` once the pass knows that it writes through it)
    if (st != TGX_OK) return st;
    HIP_TRY(hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream));
    HIP_TRY(hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream));
    tgx::EncodeParams p = base_encode_params(m, c, seed);
    p.dropout = dropout;
    if (const char* e = knob("TGX_TRACE_CARRY")) p.trace_carry = atoi(e) ? 1u : 0u;
    if (const char* e = knob("TGX_TRACE_STRIDE")) p.trace_stride = (uint32_t)std::min(3, std::max(0, atoi(e)));
    p.flags = debug_flags();
    // TGX_PATH=fused forces the one-sample-per-wave kernel (A/B timing, tests of both paths)
    const char* force = knob("TGX_PATH");
    const bool use4 = m->lm <= 16 && m->scores_finite && m->d_tokhash && !(force && strcmp(force, "fused") == 0);
    // vocabularies with tokens of 17..32 bytes (after `merge`): two samples per wave (encode2.hip)
    const bool use2 = !use4 && m->lm <= 32 && m->scores_finite && m->d_tokhash && !(force && strcmp(force, "fused") == 0);
    // encode5_kernel / encode6_kernel (8-byte label-checked records, match indices = ranks of score values, the
    // hottest values in LDS and the rest read from L2 by the relaxing lanes) for every vocabulary with finite scores
    // and at most 65 535 distinct score values — round 3: that includes vocabularies in which every token has its own
    // score (after an M-step or merge: any trained vocabulary) and vocabularies with tokens of 17..32 bytes (after
    // `merge`: the LONG build of encode5_kernel).  encode4_kernel / encode4l_kernel remain for more distinct values
    // than that (the 500 000-entry stages of prune).  TGX_PATH=rows4 / rows5 / rows2 force a kernel (A/B timing,
    // tests of every path).
    const bool long_tokens = m->lm > 16;
    const bool use5 = (use4 || use2) && m->have_trie8 &&
                      !(force && (strcmp(force, "rows4") == 0 || strcmp(force, "rows2") == 0 || strcmp(force, "rows4l") == 0));
    if (debug_on())
        fprintf(stderr, "[tgx] encode: S=%llu N=%llu lm=%u path=%s slots=%zu root_base=%u values=%u\n",
                (unsigned long long)c->n_samples, (unsigned long long)c->n_bytes, p.lm, use4 ? (use5 ? "rows5" : "rows4") : (use2 ? "rows2" : "fused"),
                m->flat.table.size(), p.root_base, m->n_values);
    m->last_lean_items = 0;
    if (!use5) {
        if ((st = ensure_scratch(c, true)) != TGX_OK) return st;
        p.tmp = c->d_tmp;
    }
    if (use5) {
        {
            const tgx_status rst = ensure_value_ranks(m, c);
            if (rst != TGX_OK) return rst;
        }
        // One block of sixteen waves per CU, and the block's LDS (160 KiB) is shared by the match-index buffers (2 KiB
        // per wave and 16 positions per lane) and the copy of the hottest score values.  Three geometries, by the
        // number of distinct score values (1 GiB of the bench corpus, profiles/r03):
        //   * four positions per lane (the four staggered walks of a lane hide most of each other's gather latency,
        //     encode5.hip: Walk5) with EVERY value in LDS: up to ~3 700 values, 11.0 ms;
        //   * the same with 15 / 14 / 13 waves, every value in LDS: up to ~4 700 / 5 700 / 6 800 values, 11.4 - 12.3 ms;
        //   * two positions per lane, every value in LDS: up to ~11 900 values — the generate-style vocabularies
        //     of SURVEY.md 8(d), 9 652 values at 32 000 entries, 10 569 at 65 536 —, 12.7 ms;
        //   * three positions per lane x 13 waves, every value in LDS: up to ~10 100 values, 12.5 ms;
        //   * three positions per lane with the ~7 800 hottest values in LDS and the others read from L2 by the
        //     relaxing lanes (COLD builds; every token its own score: after an M-step or merge), 14.0 ms.
        // Fewer waves when the batch has fewer samples than the chip has rows, so that they spread over the CUs.
        // Tokens of 17..32 bytes: the LONG build (four positions per lane, a list of long matches per wave).
        m->last_redo_samples = 0;
        // Long samples first, four to a block (encode6_kernel: three walker waves per sample ahead of one row of the
        // block's relaxing wave), when that shortens the pass.  encode5_kernel takes ~0.104 us per byte of a
        // sample's serial chain (6.8 ms per 64 KiB) and ~1 s per 88 GB of batch; encode6_kernel ~0.037 us per byte
        // of chain (2.4 ms per 64 KiB) but ~55 GB/s once every CU has its two blocks (eight relaxing rows per CU;
        // profiles/r02: e6 shapes).  The two run one after the other, so the split is chosen among the powers of
        // two as thresholds by the sum of the two estimates; TGX_LONG_THRESHOLD forces one (0: never).
        // Its LDS copy of the value table is what two blocks per CU leave room for (~4 500 values).
        int e6_bpc = 2;
        if (const char* e = knob("TGX_E6_BPC")) e6_bpc = std::min(4, std::max(1, atoi(e)));
        uint32_t n_hot6 = std::min(m->n_values, tgx::encode6_max_hot(160u * 1024u / (uint32_t)e6_bpc, 0u));
        // More values than that: the walkers fetch the values beyond the LDS copy into `pool6` pool entries per ring
        // slot (encode5.hip: Res5), and the relaxer reads from L2 only what a full pool left behind.
        // 128 entries per slot (64 positions): 64 MiB / 256 MiB of the bench corpus take 2.70 / 6.06 ms with the
        // 9 652-value vocabulary and 2.73 / 6.12 ms with 32 000 values (64 entries: 2.91 / 6.20 and 3.69 / 7.54;
        // no pool, round 2: 4.88 / 9.82 and 5.04 / 10.11; every value in LDS: 2.64 / 5.45 — profiles/r03).
        uint32_t pool6 = 0;
        bool e6_usable = true;
        if (n_hot6 < m->n_values) {
            pool6 = 128;
            if (const char* e = knob("TGX_E6_POOL")) pool6 = (uint32_t)std::min(192, std::max(0, atoi(e)));
            if ((uint64_t)m->n_values + tgx::encode6_pool_total(pool6) > 65535ull) {
                // indices are 16 bits: no room for pool entries, and a relaxer that reads the cold values itself is
                // slower than encode5_kernel on everything but a lone long sample
                pool6 = 0;
                e6_usable = knob("TGX_E6_POOL") != nullptr || knob("TGX_LONG_THRESHOLD") != nullptr;
            }
            n_hot6 = std::min(m->n_values, tgx::encode6_max_hot(160u * 1024u / (uint32_t)e6_bpc, pool6));
        }
        n_hot6 = knob_cap_hot("TGX_E5_HOT", n_hot6);
        const bool cold6 = n_hot6 < m->n_values;
        uint64_t n_long = 0;
        uint32_t corun_cus = 0;  // CUs of encode6_kernel when both kernels run at once (0: one after the other)
        if (c->n_samples && !long_tokens && e6_usable) {  // (encode6_kernel walks 16 bytes)
            const auto count_ge = [&](uint64_t thr) {  // h_sorted_len descends: the long samples are a prefix of the order
                return (uint64_t)(std::partition_point(c->h_sorted_len.begin(), c->h_sorted_len.end(),
                                                       [thr](uint32_t len) { return len >= thr; }) - c->h_sorted_len.begin());
            };
            if (const char* e = knob("TGX_LONG_THRESHOLD")) {
                const uint64_t thr = (uint64_t)std::max(0ll, atoll(e));
                if (thr) n_long = count_ge(thr);
            } else {
                const double N = (double)c->n_bytes;
                // encode5_kernel's chain of a long sample on the few waves such a batch gets: 7.1 ms per 64 KiB with every
                // value in LDS, 8.7 ms with the COLD build (profiles/r03/l_*, o_*)
                const double c5 = m->n_values > tgx::encode5_max_hot(false, 8, 4, 160u * 1024u) ? 0.135e-6 : 0.108e-6;
                auto cost = [&](uint64_t k) {  // the k longest samples to encode6_kernel
                    const double bytes_long = k ? (double)c->h_sorted_cum[k - 1] : 0.0;
                    const double t6 = k ? std::max((double)c->h_sorted_len[0] * (cold6 ? 0.042e-6 : 0.0369e-6), bytes_long / (cold6 ? 46e9 : 55e9)) + 20e-6 : 0.0;
                    const double rest_max = k < c->n_samples ? (double)c->h_sorted_len[k] : 0.0;
                    const double t5 = std::max(rest_max * c5, (N - bytes_long) / 88e9);
                    return t6 + t5;
                };
                double best = cost(0);
                for (uint64_t thr = 1024; thr <= c->max_len; thr *= 2) {
                    const uint64_t k = count_ge(thr);
                    const double ck = cost(k);
                    if (k && ck < best * 0.9) {  // switch for a clear gain only
                        best = ck;
                        n_long = k;
                    }
                }
                // Both kernels at once, each on CUs of its own: between ~200 and ~450 MiB neither wins alone — the
                // long-sample kernel is bound by its eight relaxing rows per CU, encode5_kernel by the chains of the
                // longest samples.  `corun_cus` CUs (two blocks each) take the samples of at least thr bytes, the others
                // run encode5_kernel on the rest; its blocks are launched first and ask for more than half of a CU's
                // LDS, so no block of the other kernel shares their CU.  Estimates: a long-sample row does
                // 1 / 0.0369 us (0.042 us with cold values) per byte, a CU 55 (46) GB/s / 256; encode5_kernel 0.12 us
                // per byte of chain (measured beside the other kernel) and 70 GB/s x its share of the CUs.
                const double c6 = cold6 ? 0.042e-6 : 0.0369e-6, r6 = (cold6 ? 46e9 : 55e9) / (double)m->num_cus;
                double best_co = best * 0.9;
                uint64_t k_co = 0;
                static const uint64_t thrs[] = {8192, 12288, 16384, 24576, 32768, 40960, 49152};
                static const uint32_t shares[] = {32, 48, 64, 96, 128, 160, 192};
                // (only when encode5_kernel keeps every value in LDS on its few waves: its COLD builds are bound by the
                // chains of mid-length samples at twice the estimate — profiles/r03/p_corun_sweep*.txt)
                // (and never again after a pass whose host wait for encode5_kernel's blocks timed out: the device's atomic to
                // mapped host memory was not delivered, every co-run would pay the full 2 ms and lose the CU separation)
                const bool corun_off = (knob("TGX_CORUN") && atoi(knob("TGX_CORUN")) == 0) || m->corun_wait_timeouts != 0 ||
                                       m->n_values > tgx::encode5_max_hot(false, 8, 4, 160u * 1024u);
                for (uint64_t thr : thrs) {
                    if (corun_off || thr > c->max_len || e6_bpc != 2) break;
                    const uint64_t k = count_ge(thr);
                    if (!k || k >= c->n_samples) continue;
                    const double bytes_long = (double)c->h_sorted_cum[k - 1];
                    const double r_max = (double)c->h_sorted_len[k], r_bytes = N - bytes_long;
                    for (uint32_t X : shares) {
                        if ((int)X >= m->num_cus) break;
                        const double t6 = std::max((double)c->h_sorted_len[0] * c6, bytes_long / (X * r6)) + 20e-6;
                        const double t5 = std::max(r_max * 0.12e-6, r_bytes / ((double)(m->num_cus - (int)X) / (double)m->num_cus * 70e9));
                        const double t = std::max(t5, t6);
                        if (t < best_co) {
                            best_co = t;
                            k_co = k;
                            corun_cus = X;
                        }
                    }
                }
                if (corun_cus) n_long = k_co;
            }
            if (const char* e = knob("TGX_CORUN")) {  // forces the share of the long-sample kernel (0: no co-run)
                const int v = atoi(e);
                corun_cus = (v > 0 && v < m->num_cus && n_long > 0 && n_long < c->n_samples && e6_bpc == 2) ? (uint32_t)v : 0u;
            }
        }
        const int cus5 = m->num_cus - (int)corun_cus;  // CUs of encode5_kernel
        // what is left for encode5_kernel: the samples from n_long on in the longest-first order
        const uint64_t rest_n = c->n_samples - n_long;
        const uint64_t rest_bytes = c->n_bytes - (n_long ? c->h_sorted_cum[n_long - 1] : 0);
        const uint64_t rest_max = rest_n ? c->h_sorted_len[n_long] : 0;
        int ppl = 4, bpc = 1, hot_waves = 16;  // hot_waves: the most waves beside which every value fits
        // the depth at which a trip's live walks are packed into fewer lanes (encode5.hip: Walk5)
        int compact = kE5CompactDepth;
        if (const char* e = knob("TGX_E5_COMPACT")) compact = (strcmp(e, "off") == 0 || atoi(e) == 0) ? 0 : std::min(8, std::max(4, atoi(e)));
        // the lean relaxation step (device_common.h: relax5_lean_step) for models whose scores pass
        // the gate (lean_gate.h); TGX_E5_LEAN=0: the kernels as they were
        // (the gate is the lean STEP's: a model that fails it runs the lean builds without the step)
        bool lean = tgx::encode5_has_lean(dropout > 0.0, long_tokens);
        if (const char* e = knob("TGX_E5_LEAN")) lean = lean && atoi(e) != 0;
        const bool step_ok = m->lean_scores_ok;
        // ids in place (ids_in_place.h): everything but the build's own term is known here, and the geometry below is
        // sized by the registers of the build that will run — the counting one where this holds and the build has one
        tgx::IdsInPlaceQuery iq{};
        iq.rows5 = true;
        iq.long_tokens = long_tokens;
        iq.dropout = dropout > 0.0;
        iq.n_long = n_long;
        iq.build_counts = true;  // (set below, once the build is chosen)
        iq.max_len = c->max_len;
        iq.switched_on = !(knob("TGX_IDS_IN_PLACE") && atoi(knob("TGX_IDS_IN_PLACE")) == 0);
        iq.diagnostics = p.flags != 0u || (debug_on() && getenv("TGX_STAMPS") != nullptr);
        const bool want_count = r != nullptr && tgx::ids_in_place(iq);
        {
            int ps4 = 0;
            HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, false, 4, long_tokens, compact, lean, step_ok, want_count, &ps4));
            hot_waves = std::min(16, ps4 * 4);
            const int least = long_tokens ? 12 : 13;  // (the long-token build has four positions per lane only)
            while (hot_waves >= least && m->n_values > tgx::encode5_max_hot(long_tokens, hot_waves, 4, 160u * 1024u)) hot_waves--;
            if (hot_waves < least) {
                hot_waves = 0;  // not with four positions per lane
                if (!long_tokens) {
                    // three positions per lane x 13 waves with every value in LDS (up to ~10 100: the 32 000-entry spec
                    // vocabulary, 12.5 ms against 12.8 with two positions per lane); two x 16 (up to ~11 900: the
                    // 65 536-entry one, 13.0 ms); else three x 16 with the ~7 800 hottest in LDS (every token its own
                    // score: 14.0 ms against 14.4 with four positions per lane and 3 712) — profiles/r03/n_e5_ppl3_sweep.txt
                    if (m->n_values <= tgx::encode5_max_hot(false, 13, 3, 160u * 1024u)) {
                        ppl = 3;
                        hot_waves = 13;
                    } else if (m->n_values <= tgx::encode5_max_hot(false, 16, 2, 160u * 1024u)) {
                        ppl = 2;
                    } else {
                        ppl = 3;
                    }
                }
            }
        }
        // A batch whose longest sample is more than a row's share of it is not bound by throughput but by the rows that
        // drew the long samples: with rows = bytes / longest sample every row's share is one such sample, fewer waves run
        // each faster, and their LDS takes every value with four positions per lane (the longest trips).  512 MiB of the
        // bench corpus: 8 waves, 9.7 ms against 10.5 (three positions x 13 waves); with distinct scores 11.3 against 12.5
        // (profiles/r03/o_split_and_geometry_by_size.txt).  From 11 waves on the throughput geometries above are faster.
        int balance_waves = 0;
        if (rest_max > 0) {
            const uint64_t rows_bal = (rest_bytes + rest_max - 1) / rest_max;
            const uint64_t wb = (rows_bal + 4ull * (uint64_t)cus5 - 1) / (4ull * (uint64_t)cus5);
            if (wb <= 10) {
                balance_waves = (int)std::max<uint64_t>(4, wb);
                ppl = 4;
                hot_waves = 0;
            }
        }
        if (const char* e = long_tokens ? nullptr : knob("TGX_PPL")) {
            const int v = atoi(e);
            if (v >= 1 && v <= 4) {
                ppl = v;
                bpc = ppl >= 3 ? 1 : 2;
            }
        }
        knob_int("TGX_BPC", 1, 8, &bpc);
        const uint32_t budget = 160u * 1024u / (uint32_t)bpc;
        bool cold = false;
        int per_simd = 0;
        HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, false, ppl, long_tokens, compact, lean, step_ok, want_count, &per_simd));
        int waves = std::min(16, (per_simd / bpc) * 4);
        if ((ppl == 4 || ppl == 3) && bpc == 1 && hot_waves > 0) waves = std::min(waves, hot_waves);
        if (m->n_values > tgx::encode5_max_hot(long_tokens, waves, ppl, budget)) {
            cold = true;
            HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, true, ppl, long_tokens, compact, lean, step_ok, want_count, &per_simd));
            waves = std::min(16, (per_simd / bpc) * 4);
        }
        if (balance_waves > 0 && ppl == 4 && bpc == 1) waves = std::min(waves, balance_waves);
        waves = waves_for_units(waves, rest_n, (uint64_t)cus5 * bpc);
        knob_int("TGX_WAVES", 1, 16, &waves);
        while (waves > 1 && tgx::encode5_max_hot(long_tokens, waves, ppl, budget) < 16u) waves--;
        uint32_t n_hot = std::min(m->n_values, tgx::encode5_max_hot(long_tokens, waves, ppl, budget));
        n_hot = knob_cap_hot("TGX_E5_HOT", n_hot);
        cold = n_hot < m->n_values;
        m->last_n_hot = n_hot;
        iq.build_counts = tgx::encode5_counts(dropout > 0.0, cold, ppl, long_tokens);
        const bool in_place = want_count && tgx::ids_in_place(iq);
        if (!in_place) {  // the trace writes through `tmp`
            if ((st = ensure_scratch(c, true)) != TGX_OK) return st;
            p.tmp = c->d_tmp;
        }
        // (self-check) the lean items of this pass's kernels: encode5_kernel's in the low byte, encode6_kernel's in the next
        m->last_lean_items = !lean ? 0u : ((rest_n ? (uint32_t)tgx::encode5_lean_items(cold, ppl, step_ok) : 0u) |
                                           (n_long ? (uint32_t)tgx::encode6_lean_items() << 8 : 0u));
        // whole blocks only: a block's waves are dealt round-robin to the SIMDs, ceil(waves / 4) on the fullest
        m->last_encode_waves_per_cu = std::min(bpc, per_simd / ((waves + 3) / 4)) * waves;
        const uint64_t rows_per_block = 4 * (uint64_t)waves;
        const uint32_t blocks5 = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>((rest_n + rows_per_block - 1) / rows_per_block, (uint64_t)cus5 * bpc));
        tgx::Encode5Params q{};
        q.trie8 = m->d_trie8;
        q.trie_bytes = (uint32_t)(m->flat.table.size() * sizeof(tgx::Trie8Rec));
        q.values = m->d_values;
        q.root_base = m->root_base8;
        q.n_values = m->n_values;
        q.n_hot = n_hot;
        q.claim_chunk = claim_chunk_for(c->n_bytes, c->n_samples);
        if (const char* e = knob("TGX_CLAIM_CHUNK")) q.claim_chunk = (uint32_t)std::min(64, std::max(1, atoi(e)));
        m->last_long_samples = n_long;
        m->last_corun_cus = n_long ? corun_cus : 0u;
        tgx::EncodeParams p6 = p;
        tgx::Encode5Params q6 = q;
        uint32_t blocks6 = 0;
        if (n_long) {
            p6.n_samples = n_long;
            // four samples per block (one per row of its relaxing wave); 13 waves of 64 registers: two blocks per CU
            blocks6 = (uint32_t)std::min<uint64_t>((n_long + 3) / 4, (uint64_t)(corun_cus ? (int)corun_cus : m->num_cus) * (uint64_t)e6_bpc);
            q6.n_hot = n_hot6;
            q6.pool = cold6 ? pool6 : 0u;
            if (!corun_cus) {
                time_begin(m, "encode6_kernel");
                HIP_TRY(tgx::launch_encode6(p6, q6, cold6, lean, blocks6, m->stream));
                time_end(m);
                HIP_TRY(hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream));  // the work queue, for encode5_kernel
            } else {
                if (!m->stream2) {
                    HIP_TRY(hipStreamCreateWithFlags(&m->stream2, hipStreamNonBlocking));
                    HIP_TRY(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
                    HIP_TRY(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
                    HIP_TRY(hipHostMalloc((void**)&m->h_started, 64, hipHostMallocMapped | hipHostMallocPortable));
                }
                *reinterpret_cast<volatile unsigned int*>(m->h_started) = 0u;
                q.started = m->h_started;
                p6.queue = &m->d_ctrl->queue6;  // a work queue of its own
                HIP_TRY(hipMemsetAsync(&m->d_ctrl->queue6, 0x00, 8, m->stream));
                HIP_TRY(hipEventRecord(m->ev_fork, m->stream));
                HIP_TRY(hipStreamWaitEvent(m->stream2, m->ev_fork, 0));
            }
            p.order = c->d_order + n_long;
            p.n_samples = c->n_samples - n_long;
        }
        const Stamps stamps5 = stamps_begin(m, pass, '1', (size_t)blocks5 * (size_t)waves);
        p.stamps = stamps5.d;
        time_begin(m, "encode5_kernel");
        {
            if (long_tokens) {  // samples whose wave ran out of list entries for long matches go to encode2_kernel
                p.redo_count = &m->d_ctrl->encode_redo;
                p.redo_list = c->d_counts;  // free until the trace writes the token counts
                HIP_TRY(hipMemsetAsync(&m->d_ctrl->encode_redo, 0x00, 8, m->stream));
            }
            // (co-run: more than half of the CU's LDS, so that no block of the long-sample kernel shares the CU)
            const hipError_t le = tgx::launch_encode5(p, q, cold, ppl, long_tokens, compact, lean, step_ok, in_place, waves, blocks5, corun_cus && n_long ? 84u * 1024u : 0u, m->stream);
            if (le != hipSuccess) return fail(TGX_ERR_DEVICE, "encode5 launch failed: %s", hipGetErrorString(le));
        }
        bool joined = false, joined_slot = false;
        if (n_long && corun_cus) {  // the long-sample kernel beside it, on the second stream, with a timing slot of its own
            const bool slot = m->n_timed + 1 < kMaxTimed;
            if (slot) {
                KernelTime& tb = m->timed[m->n_timed + 1];
                tb.name = "encode6_kernel";
                tb.used = true;
                (void)hipEventRecord(tb.start, m->stream2);
            }
            {   // the long-sample kernel's blocks must find the CUs of encode5_kernel's blocks taken: wait (at most 2 ms)
                // until every one of those has reported itself resident
                const auto t0 = std::chrono::steady_clock::now();
                volatile unsigned int* started = m->h_started;
                bool timed_out = false;
                while (*started < blocks5 && !(timed_out = std::chrono::steady_clock::now() - t0 >= std::chrono::milliseconds(2))) {
                }
                if (timed_out && *started < blocks5) m->corun_wait_timeouts++;
            }
            const hipError_t l6 = tgx::launch_encode6(p6, q6, cold6, lean, blocks6, m->stream2);
            if (slot) (void)hipEventRecord(m->timed[m->n_timed + 1].stop, m->stream2);
            (void)hipEventRecord(m->ev_join, m->stream2);
            if (l6 != hipSuccess) return fail(TGX_ERR_DEVICE, "encode6 launch failed: %s", hipGetErrorString(l6));
            joined = true;
            joined_slot = slot;
        }
        time_end(m);
        if (joined) {
            if (joined_slot) m->n_timed++;
            HIP_TRY(hipStreamWaitEvent(m->stream, m->ev_join, 0));  // the trace needs both kernels' back-pointers
        }
        if (stamps5.d) stamps_report(m, stamps5, ppl, "encode5 stamps", "iteration", {"switch", "text+reset", "walk", "relax", "store"});
        p.stamps = nullptr;
        if (long_tokens) {
            const tgx_status rst = redo_long_matches(m, c, p);
            if (rst != TGX_OK) return rst;
        }
        p.order = c->d_order;
        p.n_samples = c->n_samples;
        const uint32_t blocks_t = trace_blocks(m, c->n_samples);
        if (in_place) {
            // the counts are there before the trace: offsets, total (the pass's one wait), the ids buffer, and the trace
            // writes every id where it belongs.  d_ctrl->err is the caller's to read, after the trace.
            if ((st = scan_ids_offsets(m, c, r, "encode", false)) != TGX_OK) return st;
            time_begin(m, "trace_kernel");
            HIP_TRY(tgx::launch_trace_in_place(p, tgx::TraceInPlace{r->d_offs, r->d_ids}, blocks_t, m->stream));
            time_end(m);
            m->last_ids_in_place = true;
            return TGX_OK;
        }
        // TGX_STAMPS=2: the STAMP build of trace_kernel (tokens <= 16 bytes, ring flushed per sample)
        Stamps stamps_t;
        if (!long_tokens) stamps_t = stamps_begin(m, pass, '2', (size_t)blocks_t * 4);
        p.stamps = stamps_t.d;
        time_begin(m, long_tokens ? "trace32_kernel" : "trace_kernel");
        if (long_tokens) HIP_TRY(tgx::launch_trace32(p, blocks_t, true, m->stream));
        else HIP_TRY(tgx::launch_trace(p, blocks_t, m->stream));
        time_end(m);
        if (stamps_t.d) stamps_report(m, stamps_t, 0, "trace stamps", "window", {"setup", "loads", "hops", "append+lookups", "-"});
        p.stamps = nullptr;
    } else if (use4) {
        // Vocabularies without 8-byte records (more than 65 535 distinct score values): round 1's kernel over the
        // 16-byte records, scores through the match buffer.
        // `bpc` blocks per CU of `waves` waves each (8 KiB of LDS per wave and position group).
        // TGX_PPL (positions per lane: 1, 2, 4), TGX_WAVES, TGX_BPC override the defaults (with TGX_DEBUG=1).
        // Two blocks of ten waves per CU (20 x 8 KiB of LDS); rows claim samples dynamically, so the
        // geometry only has to fill the CU.
        int ppl = 1, waves = 10, bpc = 2;
        // Positions per lane.  A sample is a serial chain of 16 * ppl positions per trip, so the longest
        // sample bounds the pass from below, while more positions per lane cost LDS and with it waves per CU.
        // Measured on 1 x MI355X (tools/ppl_sweep.py): throughput 60 / 50 / 34 GB/s and 13.5 / 10.7 / 9.1 ms per
        // 64 KiB of chain for ppl = 1 / 2 / 4; take the smallest estimate.
        const double gbps4[3] = {60.0, 50.0, 34.0}, chain4_ms[3] = {13.5, 10.7, 9.1};
        auto cost4 = [&](double bytes, double longest, int* ppl_out) {
            double best_t = 0;
            int best_ppl = 1;
            for (int i = 0; i < 3; i++) {
                const double t = std::max(bytes / (gbps4[i] * 1e9), longest / 65536.0 * chain4_ms[i] * 1e-3);
                if (i == 0 || t < best_t * 0.95) {  // switch only for a clear gain
                    best_t = t;
                    best_ppl = 1 << i;
                }
            }
            if (ppl_out) *ppl_out = best_ppl;
            return best_t;
        };
        m->last_long_samples = 0;
        m->last_redo_samples = 0;
        cost4((double)c->n_bytes, c->n_samples ? (double)c->h_sorted_len[0] : 0.0, &ppl);
        if (const char* e = knob("TGX_PPL")) {  // (also set by tests: every positions-per-lane build against the oracle)
            const int v = atoi(e);
            if (v == 1 || v == 2 || v == 4) ppl = v;
        }
        if (ppl == 2) { waves = 5; bpc = 2; }
        if (ppl == 4) { waves = 5; bpc = 1; }
        knob_int("TGX_WAVES", 1, 16, &waves);
        knob_int("TGX_BPC", 1, 8, &bpc);
        bool root = ppl == 1;  // first trie level in LDS (4 KiB per block)
        if (const char* e = knob("TGX_ROOT")) root = root && atoi(e) != 0;
        while (waves > 1 && tgx::encode4_lds_bytes(waves, ppl, root) > (160u * 1024u) / (uint32_t)bpc) waves--;
        {
            // The geometry must really fit: a block's waves are dealt round-robin to the four SIMDs, so
            // `bpc` blocks put bpc * ceil(waves / 4) waves on some SIMD, which its registers must allow
            // (see encode4_kernel's note); otherwise five blocks of four waves: one wave per SIMD and block.
            int per_simd = 0;
            HIP_TRY(tgx::encode4_waves_per_simd(dropout > 0.0, ppl, root, &per_simd));
            if (bpc * ((waves + 3) / 4) > per_simd && ppl == 1) {
                waves = 4;
                bpc = std::min(5, per_simd);
                root = false;
                HIP_TRY(tgx::encode4_waves_per_simd(dropout > 0.0, ppl, root, &per_simd));
            }
            m->last_encode_waves_per_cu = std::min(bpc * ((waves + 3) / 4), per_simd) * 4 >= bpc * waves
                                              ? bpc * waves
                                              : per_simd / ((waves + 3) / 4) * waves;
        }
        const uint64_t rows_per_block = 4 * (uint64_t)waves;
        const uint32_t blocks4 = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>((p.n_samples + rows_per_block - 1) / rows_per_block, (uint64_t)m->num_cus * bpc));
        Stamps stamps4;  // (the kernel has them without dropout, one position per lane)
        if (dropout <= 0.0 && ppl == 1) stamps4 = stamps_begin(m, pass, '1', (size_t)blocks4 * (size_t)waves);
        p.stamps = stamps4.d;
        time_begin(m, "encode4_kernel");
        HIP_TRY(tgx::launch_encode4(p, ppl, waves, blocks4, root, m->stream));
        time_end(m);
        if (stamps4.d) stamps_report(m, stamps4, 0, "stamps", "iteration", {"switch", "text", "walk", "relax", "store"});
        p.stamps = nullptr;
        p.order = c->d_order;
        p.n_samples = c->n_samples;
        time_begin(m, "trace_kernel");
        HIP_TRY(tgx::launch_trace(p, trace_blocks(m, c->n_samples), m->stream));
        time_end(m);
    } else if (use2) {
        // Tokens of 17..32 bytes: the 16-lane rows with an overflow list for the long matches (encode4l.hip);
        // samples whose wave ran out of overflow entries are redone two per wave on 32-lane rows (encode2.hip),
        // as is the whole batch with TGX_PATH=rows2.
        const bool rows2 = force && strcmp(force, "rows2") == 0;
        m->last_redo_samples = 0;
        if (!rows2) {
            p.redo_count = &m->d_ctrl->encode_redo;
            p.redo_list = c->d_counts;  // free until the trace writes the token counts
            HIP_TRY(hipMemsetAsync(&m->d_ctrl->encode_redo, 0x00, 8, m->stream));
            time_begin(m, "encode4l_kernel");
            HIP_TRY(tgx::launch_encode4l(p, (uint32_t)m->num_cus, m->stream));
            time_end(m);
            const tgx_status rst = redo_long_matches(m, c, p);
            if (rst != TGX_OK) return rst;
        } else {
            time_begin(m, "encode2_kernel");
            HIP_TRY(tgx::launch_encode2(p, (uint32_t)m->num_cus, false, m->stream));
            time_end(m);
        }
        time_begin(m, "trace32_kernel");
        HIP_TRY(tgx::launch_trace32(p, trace_blocks(m, c->n_samples), !rows2, m->stream));
        time_end(m);
    } else {
        time_begin(m, "encode_kernel");
        HIP_TRY(tgx::launch_encode(p, grid_blocks(m, c->n_samples), m->stream));
        time_end(m);
    }
    return TGX_OK;
}

// The first half of what follows a pass's counts (c->d_counts): the counts scanned into r's offsets, the total read back —
// the pass's one mid-pass synchronisation — and the ids buffer allocated.  with_err: the trace has run, so the lowest
// failing sample is read in the same wait and checked (a pass that traces in place reads it after its trace instead).
tgx_status scan_ids_offsets(tgx_model* m, tgx_corpus* c, tgx_result* r, const char* what, bool with_err) {
    const uint64_t S = c->n_samples;
    if (!c->d_scan_tmp) {  // scratch of the device-wide scan (large sample counts only), kept on the corpus
        if (tgx::scan_temp_bytes(S, &c->scan_tmp_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan temp-size query failed");
        if (c->scan_tmp_bytes && c->d_scan_tmp.alloc(m->device, c->scan_tmp_bytes) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (scan)");
    }
    time_begin(m, "scan_counts_kernel");
    if (tgx::launch_scan(c->d_counts, r->d_offs, S, c->d_scan_tmp, c->scan_tmp_bytes, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "scan launch failed");
    time_end(m);
    if ((with_err && hipMemcpyAsync(&m->h_ctrl->err, &m->d_ctrl->err, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
        hipMemcpyAsync(&m->h_ctrl->total_tokens, r->d_offs + S, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "%s pass failed: %s", what, hipGetErrorString(hipGetLastError()));
    if (with_err) {
        const tgx_status st = check_no_path(m, c);
        if (st != TGX_OK) return st;
    }
    r->n_tokens = m->h_ctrl->total_tokens;
    if (r->n_tokens > c->n_bytes) return fail(TGX_ERR_DEVICE, "internal error: %s pass counted more tokens than bytes", what);
    if (r->d_ids.alloc(m->device, (size_t)r->n_tokens * 4 + 256) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (result ids)");
    return TGX_OK;
}

}  // namespace

// The ids of an encode or sampling pass whose kernels left every sample's token count in c->d_counts and its ids
// right-aligned in c->d_tmp: the counts scanned into r's offsets, the lowest failing sample and the total read back,
// the ids buffer, the compaction.  The compaction is queued, not waited for.  `what` names the pass in messages.
tgx_status tgx::dev::compact_ids(tgx_model* m, tgx_corpus* c, tgx_result* r, const char* what) {
    const uint64_t S = c->n_samples;
    const tgx_status sst = scan_ids_offsets(m, c, r, what, true);
    if (sst != TGX_OK) return sst;
    tgx::CompactParams cp{};
    cp.offs = c->d_offs;
    cp.order = c->d_order;
    cp.n_samples = S;
    cp.tmp = c->d_tmp;
    cp.out_offs = r->d_offs;
    cp.ids = r->d_ids;
    // short samples (fewer than 128 ids on average): a 16-lane row per sample instead of a wave
    const bool rows = S && r->n_tokens / S < 128;
    const uint64_t units = rows ? 16 : 4;  // samples per block and round
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((S + units - 1) / units, (uint64_t)m->num_cus * 8));
    time_begin(m, "compact_kernel");
    if (tgx::launch_compact(cp, blocks, rows, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "compact launch failed");
    time_end(m);
    return TGX_OK;
}

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

// Tables that only the encode path reads (built at creation, or at the first encode of a model created with
// TGX_MODEL_FOR_ESTEP: prune builds two such models per iteration and never encodes with them).  Caller holds
// m->mu (or is the creating thread).
tgx_status tgx::dev::ensure_encode_tables(tgx_model* m) {
    if (m->encode_tables_ready) return TGX_OK;
    HIP_TRY(hipSetDevice(m->device));
    // the bytes -> id table and the 8-byte records are independent: the first is built on a second host thread
    // while this one builds the second (each ~50 ms at 500 000 tokens)
    tgx::HostPhases hp("ensure_encode_tables");
    const bool want_hash = m->lm <= 32 && m->scores_finite;
    const bool want_trie8 = m->lm <= 32 && m->scores_finite && m->flat.table.size() <= tgx::kTrie8MaxSlots;
    std::thread hash_builder;
    if (want_hash && !m->tokhash_host_built)
        hash_builder = std::thread([m]() { tgx::build_tok_hash(m->vocab_bytes.data(), m->vocab_offs.data(), m->vocab_size, &m->tokhash); });
    tgx::Trie8 t8;
    if (want_trie8) tgx::build_trie8(m->flat, m->vocab_offs.data(), m->vocab_scores.data(), &t8);
    if (hash_builder.joinable()) hash_builder.join();
    hp.mark("trie8 | tok hash");
    // (a failure part-way leaves the tables that exist in place, pointers set: the next call finds them — nothing is
    // allocated twice — and tgx_model_destroy frees them)
    if (want_hash && m->tokhash.ok && !m->d_tokhash) {
        const size_t hb = m->tokhash.slots.size() * sizeof(tgx::TokHashEntry);
        HIP_TRY(hipMalloc(&m->d_tokhash, hb));
        HIP_TRY(hipMemcpyAsync(m->d_tokhash, m->tokhash.slots.data(), hb, hipMemcpyHostToDevice, m->stream));
    }
    if (want_trie8 && t8.ok && m->d_tokhash) {
        const size_t ns = t8.rec.size();
        if (!m->d_trie8) HIP_TRY(hipMalloc(&m->d_trie8, ns * sizeof(tgx::Trie8Rec)));
        if (!m->d_values) HIP_TRY(hipMalloc((void**)&m->d_values, t8.values.size() * 8));
        HIP_TRY(hipMemcpy(m->d_trie8, t8.rec.data(), ns * sizeof(tgx::Trie8Rec), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m->d_values, t8.values.data(), t8.values.size() * 8, hipMemcpyHostToDevice));
        m->n_values = (uint32_t)t8.values.size() - 1u;
        m->value_coverage = std::move(t8.coverage);
        m->root_base8 = t8.root_base;
        m->have_trie8 = true;
    }
    HIP_TRY(hipStreamSynchronize(m->stream));
    hp.mark("uploads");
    m->encode_tables_ready = true;
    return TGX_OK;
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

// ---- encode --------------------------------------------------------------------

// caller holds m->mu
static tgx_status encode_corpus_locked(tgx_model* m, tgx_corpus* c, double dropout, uint64_t seed,
                                       tgx_result** out) {
    HIP_TRY(hipSetDevice(m->device));
    {
        const tgx_status est = ensure_encode_tables(m);
        if (est != TGX_OK) return est;
    }
    m->n_timed = 0;
    const uint64_t S = c->n_samples;

    Pass pass(m);
    tgx_result* r = pass.new_result(S);
    if (r->d_offs.alloc(m->device, (size_t)(S + 1) * 8) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (result offsets)");
    tgx_status st = run_encode_kernel(m, c, dropout, seed, pass, r);
    if (st != TGX_OK) return st;
    if (m->last_ids_in_place) {
        // offsets and ids are in r already: what is left is the lowest failing sample (no path, or the trace's check of
        // the relaxation's counts), read in the wait that ends the pass
        if (hipMemcpyAsync(&m->h_ctrl->err, &m->d_ctrl->err, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "encode pass failed: %s", hipGetErrorString(hipGetLastError()));
        st = check_no_path(m, c);
        if (st != TGX_OK) return st;
    } else {
        st = compact_ids(m, c, r, "encode");
        if (st != TGX_OK) return st;
        if (hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "compact failed: %s", hipGetErrorString(hipGetLastError()));
    }
    // N + 4T + 16(S+1)
    m->last_alg_bytes = c->n_bytes + 4 * r->n_tokens + 16 * (S + 1);
    *out = pass.release_result();
    return pass.done();
}

tgx_status tgx_encode_corpus(tgx_model* m, tgx_corpus* c, double dropout, uint64_t seed,
                             tgx_result** out) {
    if (!m || !c || !out) return fail(TGX_ERR_INVALID, "tgx_encode_corpus: NULL argument");
    *out = nullptr;
    if (m->device != c->device) return fail(TGX_ERR_INVALID, "model and corpus on different devices");
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkc(c->mu);
    return encode_corpus_locked(m, c, dropout, seed, out);
}

tgx_status tgx_encode_batch(tgx_model* m, const uint8_t* text, const uint64_t* offs,
                            uint64_t n_samples, double dropout, uint64_t seed, tgx_result** out) {
    if (!m || !out) return fail(TGX_ERR_INVALID, "tgx_encode_batch: NULL argument");
    *out = nullptr;
    return on_uploaded_batch(m, text, offs, n_samples, [&](tgx_corpus* c) { return tgx_encode_corpus(m, c, dropout, seed, out); });
}

// Host buffers in, host buffers out (what a Rust caller of Tokenizer::encode_batch has: bindings/python/src/lib.rs:51-59
// hands over borrowed strings and takes owned vectors back).  A large batch is cut at sample boundaries into chunks
// of 256 MiB that go through three stages — upload, kernels, download — each on a thread of its own: the kernels of
// one chunk run while the text of the next goes to the device and the ids of the previous come back, so
// the PCIe link works in both directions beside the kernels instead of before and after them.  ids_out must hold
// ids_cap entries (at most one token per byte: ids_cap = bytes always suffices); offs_out[n_samples + 1].
// Dropout passes keep the one-chunk path (the keep rule hashes the sample's index in the batch).
tgx_status tgx_encode_batch_host(tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, double dropout,
                                 uint64_t seed, uint32_t* ids_out, uint64_t ids_cap, uint64_t* offs_out, uint64_t* n_tokens) {
    if (!m || !offs_out || !n_tokens || (n_samples && !offs)) return fail(TGX_ERR_INVALID, "tgx_encode_batch_host: NULL argument");
    *n_tokens = 0;
    offs_out[0] = 0;
    if (n_samples == 0) return TGX_OK;
    for (uint64_t i = 0; i < n_samples; i++)
        if (offs[i + 1] < offs[i]) return fail(TGX_ERR_INVALID, "offsets not monotone at %llu", (unsigned long long)i);
    const uint64_t N = offs[n_samples] - offs[0];
    // chunk boundaries
    std::vector<uint64_t> cut(1, 0);
    {
        uint64_t chunk = 256ull << 20;  // a chunk's pass is bounded below by the serial chain of its longest sample: few, large chunks
        if (dropout > 0.0) chunk = ~0ull;
        if (const char* e = knob("TGX_E2E_CHUNK_MB")) {
            const long v = atol(e);
            if (v > 0 && dropout <= 0.0) chunk = (uint64_t)v << 20;
        }
        uint64_t start = offs[0];
        for (uint64_t i = 0; i < n_samples; i++)
            if (offs[i + 1] - start >= chunk && i + 1 < n_samples) {
                cut.push_back(i + 1);
                start = offs[i + 1];
            }
        cut.push_back(n_samples);
    }
    const size_t C = cut.size() - 1;
    // Three stages, each chunk through them in order: this thread downloads, one thread uploads, one runs the
    // kernels.  (Workers that each took a chunk through all three stages started their uploads together, shared
    // the link, and the first kernel waited for all of them.)
    struct ChunkState {
        tgx_corpus* corpus = nullptr;
        tgx_result* result = nullptr;
        uint64_t tokens = 0;
        int stage = 0;  // 1 uploaded, 2 encoded, 3 downloaded
    };
    std::vector<ChunkState> cs(C);
    std::mutex mu;
    std::condition_variable cv;
    tgx_status first_err = TGX_OK;
    std::string err_msg;
    uint64_t err_sample = 0, err_pos = 0, err_len = 0;
    bool abort_all = false;
    size_t downloaded = 0;
    uint64_t err_base = ~0ull;  // first sample of the chunk the recorded error belongs to
    auto set_error = [&](tgx_status st, uint64_t sample_base) {  // under mu; g_err_* are this thread's
        // the error of the LOWEST chunk is the batch's (an upload failure of a later chunk must not hide the NoPath of
        // an earlier one that is still being encoded: the encoder records its own when it gets there)
        if (first_err == TGX_OK || sample_base < err_base) {
            first_err = st;
            err_base = sample_base;
            err_msg = g_err_msg;
            err_sample = g_err_sample + sample_base;
            err_pos = g_err_pos;
            err_len = g_err_len;
        }
        abort_all = true;
        cv.notify_all();
    };
    const auto t_start = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what, size_t k, std::chrono::steady_clock::time_point t0) {  // TGX_DEBUG=1: stage timeline
        if (!debug_on()) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[tgx] e2e chunk %zu %-8s %7.2f -> %7.2f ms\n", k, what,
                std::chrono::duration<double, std::milli>(t0 - t_start).count(),
                std::chrono::duration<double, std::milli>(now - t_start).count());
    };
    std::thread uploader([&]() {
        for (size_t k = 0; k < C; k++) {
            {
                std::unique_lock<std::mutex> lk(mu);  // at most three chunks between upload and download
                cv.wait(lk, [&]() { return abort_all || k < downloaded + 3; });
                if (abort_all) return;
            }
            tgx_corpus* c = nullptr;
            const auto t0 = std::chrono::steady_clock::now();
            const tgx_status st = tgx_corpus_upload(m->device, text, offs + cut[k], cut[k + 1] - cut[k], &c);
            stamp("upload", k, t0);
            std::lock_guard<std::mutex> lk(mu);
            if (st != TGX_OK) {
                set_error(st, cut[k]);
                return;
            }
            cs[k].corpus = c;
            cs[k].stage = 1;
            cv.notify_all();
        }
    });
    std::thread encoder([&]() {
        for (size_t k = 0; k < C; k++) {
            tgx_corpus* c = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&]() { return abort_all || cs[k].stage >= 1; });
                if (cs[k].stage < 1) return;  // aborted before this chunk was uploaded
                c = cs[k].corpus;
                if (abort_all && cut[k] >= err_base) continue;  // (the main thread frees what is left; a chunk BELOW a
                                                                // failed upload is still encoded: its own error would come first)
            }
            tgx_result* r = nullptr;
            const auto t0 = std::chrono::steady_clock::now();
            const tgx_status st = tgx_encode_corpus(m, c, dropout, seed, &r);
            tgx_corpus_free(c);  // text and scratch go back to the pool for the next chunk's upload
            stamp("kernels", k, t0);
            std::lock_guard<std::mutex> lk(mu);
            cs[k].corpus = nullptr;
            if (st != TGX_OK) {
                set_error(st, cut[k]);  // chunks are encoded in order: the lowest failing sample of the batch
                return;
            }
            cs[k].result = r;
            cs[k].tokens = r->n_tokens;
            cs[k].stage = 2;
            cv.notify_all();
        }
    });
    uint64_t base = 0;
    for (size_t k = 0; k < C; k++) {
        tgx_result* r = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&]() { return abort_all || cs[k].stage >= 2; });
            if (cs[k].stage < 2) break;
            r = cs[k].result;
        }
        const uint64_t lo = cut[k], hi = cut[k + 1];
        const auto t0 = std::chrono::steady_clock::now();
        tgx_status st2 = TGX_OK;
        if (base + r->n_tokens > ids_cap) {
            st2 = fail(TGX_ERR_INVALID, "tgx_encode_batch_host: ids_out holds %llu ids, the batch has more", (unsigned long long)ids_cap);
        } else {
            if (r->n_tokens) st2 = tgx_result_copy_ids(r, ids_out + base, r->n_tokens);
            if (st2 == TGX_OK) {
                std::vector<uint64_t> lo_offs(hi - lo + 1);
                st2 = tgx_result_copy_offsets(r, lo_offs.data(), hi - lo + 1);
                for (uint64_t i = 0; i <= hi - lo && st2 == TGX_OK; i++) offs_out[lo + i] = base + lo_offs[i];
            }
        }
        base += r->n_tokens;
        stamp("download", k, t0);
        // the chunk's ids are in the caller's memory: its device buffers go back to the pool now (a batch larger
        // than the free HBM streams through; kept until the end they grew by a byte per input byte)
        if (st2 == TGX_OK) tgx_result_free(r);
        std::lock_guard<std::mutex> lk(mu);
        if (st2 != TGX_OK) {
            g_err_sample = 0;
            set_error(st2, 0);
            break;
        }
        cs[k].result = nullptr;
        cs[k].stage = 3;
        downloaded = k + 1;
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        if (downloaded < C && first_err == TGX_OK) abort_all = true;  // (cannot happen: a stage that stops sets the error)
        cv.notify_all();
    }
    uploader.join();
    encoder.join();
    for (size_t k = 0; k < C; k++) {
        if (cs[k].result) tgx_result_free(cs[k].result);
        if (cs[k].corpus) tgx_corpus_free(cs[k].corpus);
    }
    if (first_err != TGX_OK) {
        g_err_msg = err_msg;
        g_err_sample = err_sample;
        g_err_pos = err_pos;
        g_err_len = err_len;
        return first_err;
    }
    uint64_t total = 0;
    for (size_t k = 0; k < C; k++) total += cs[k].tokens;
    *n_tokens = total;
    m->last_alg_bytes = N + 4 * total + 16 * (n_samples + 1);
    return TGX_OK;
}

// One host process, several devices: the batch is cut at sample boundaries into one byte-balanced shard per model
// handle (one handle per GPU; the reference's batch is ONE call from one process, src/tokenizer.rs:102-111), every shard
// goes through tgx_encode_batch_host on a host thread of its own, and the shards' ids are packed in sample order.  No
// collective: the path shards by samples.  ids_out must hold one id per input byte (ids_cap >= bytes: every shard writes
// at its text offset first).  With dropout the keep decisions hash the sample's index in its SHARD.
tgx_status tgx_encode_batch_multi(tgx_model* const* models, uint32_t n_models, const uint8_t* text, const uint64_t* offs,
                                  uint64_t n_samples, double dropout, uint64_t seed, uint32_t* ids_out, uint64_t ids_cap,
                                  uint64_t* offs_out, uint64_t* n_tokens) {
    if (!models || n_models == 0 || !offs_out || !n_tokens || (n_samples && !offs)) return fail(TGX_ERR_INVALID, "tgx_encode_batch_multi: NULL argument");
    for (uint32_t k = 0; k < n_models; k++)
        if (!models[k]) return fail(TGX_ERR_INVALID, "tgx_encode_batch_multi: NULL model handle");
    *n_tokens = 0;
    offs_out[0] = 0;
    if (n_samples == 0) return TGX_OK;
    const uint64_t N = offs[n_samples] - offs[0];
    if (ids_cap < N) return fail(TGX_ERR_INVALID, "tgx_encode_batch_multi: ids_out must hold one id per input byte (%llu), it holds %llu",
                                 (unsigned long long)N, (unsigned long long)ids_cap);
    // shard bounds: the first sample whose start is at or beyond k / n_models of the bytes
    std::vector<uint64_t> cut(n_models + 1, n_samples);
    cut[0] = 0;
    for (uint32_t k = 1; k < n_models; k++) {
        const uint64_t want = offs[0] + N / n_models * k;
        cut[k] = (uint64_t)(std::lower_bound(offs, offs + n_samples, want) - offs);
        cut[k] = std::max(cut[k], cut[k - 1]);
    }
    struct Shard {
        tgx_status st = TGX_OK;
        uint64_t tokens = 0;
        std::string msg;
        uint64_t es = 0, ep = 0, el = 0;
        std::vector<uint64_t> lo;
    };
    std::vector<Shard> sh(n_models);
    std::vector<std::thread> th;
    for (uint32_t k = 0; k < n_models; k++) {
        th.emplace_back([&, k]() {
            Shard& S = sh[k];
            const uint64_t a = cut[k], b = cut[k + 1];
            if (b == a) return;
            S.lo.assign(b - a + 1, 0);
            const uint64_t region = offs[a] - offs[0];  // (at most one token per byte: the shard's ids fit behind its text offset)
            S.st = tgx_encode_batch_host(models[k], text, offs + a, b - a, dropout, seed, ids_out + region, ids_cap - region, S.lo.data(), &S.tokens);
            if (S.st != TGX_OK) {  // the error state is this thread's
                S.msg = g_err_msg;
                S.es = g_err_sample + a;
                S.ep = g_err_pos;
                S.el = g_err_len;
            }
        });
    }
    for (std::thread& t : th) t.join();
    for (uint32_t k = 0; k < n_models; k++)
        if (sh[k].st != TGX_OK) {  // the lowest failing shard: the lowest failing sample of the batch
            g_err_msg = sh[k].msg;
            g_err_sample = sh[k].es;
            g_err_pos = sh[k].ep;
            g_err_len = sh[k].el;
            return sh[k].st;
        }
    uint64_t base = 0;
    for (uint32_t k = 0; k < n_models; k++) {
        const uint64_t a = cut[k], b = cut[k + 1];
        if (b == a) continue;
        const uint64_t region = offs[a] - offs[0];
        if (region != base && sh[k].tokens) memmove(ids_out + base, ids_out + region, sh[k].tokens * sizeof(uint32_t));
        for (uint64_t i = 0; i <= b - a; i++) offs_out[a + i] = base + sh[k].lo[i];
        base += sh[k].tokens;
    }
    *n_tokens = base;
    return TGX_OK;
}

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

tgx_status scan_room(ScanScratch* s, StreamGuard& guard, hipError_t (*temp_bytes)(uint64_t, size_t*), uint64_t n) {
    if (n <= s->n) return TGX_OK;
    if (temp_bytes(n, &s->bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan temp-size query failed");
    HIP_TRY(guard.alloc(s->bytes, &s->ptr));  // (never NULL: that asks the scan for its size)
    s->n = n;
    return TGX_OK;
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

uint32_t tgx_last_encode_waves_per_cu(const tgx_model* m) { return m ? (uint32_t)m->last_encode_waves_per_cu : 0u; }
uint64_t tgx_last_algorithmic_bytes(const tgx_model* m) { return m ? m->last_alg_bytes : 0; }
uint64_t tgx_last_encode_redo_samples(const tgx_model* m) { return m ? m->last_redo_samples : 0; }
uint64_t tgx_last_encode_long_samples(const tgx_model* m) { return m ? m->last_long_samples : 0; }
uint64_t tgx_last_estep_pieces(const tgx_model* m) { return m ? m->last_estep_pieces : 0; }
uint64_t tgx_last_estep_redo(const tgx_model* m) { return m ? m->last_estep_redo : 0; }
uint32_t tgx_last_encode_corun_cus(const tgx_model* m) { return m ? m->last_corun_cus : 0; }
uint32_t tgx_encode_corun_timeouts(const tgx_model* m) { return m ? m->corun_wait_timeouts : 0; }
uint32_t tgx_model_score_values(const tgx_model* m) { return m && m->have_trie8 ? m->n_values : 0u; }
uint32_t tgx_last_encode_hot_values(const tgx_model* m) { return m ? m->last_n_hot : 0u; }
uint32_t tgx_last_encode_lean_items(const tgx_model* m) { return m ? m->last_lean_items : 0u; }
int tgx_last_encode_ids_in_place(const tgx_model* m) { return (m && m->last_ids_in_place) ? 1 : 0; }
