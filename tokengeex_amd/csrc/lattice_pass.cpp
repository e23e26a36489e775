// The C ABI's passes over the whole lattice of a sample (include/tgx.h): sampling (sample.hip), lattice statistics
// (stats.hip) and n-best (nbest.hip), each over a resident corpus or an uploaded batch.  They run on the model's own
// stream under a Pass, take the knobs and the corpus's scratch from tgx_api.cpp, and share the encode parameters, the
// tables and the end of a pass with encode in encode_pass.cpp (pass_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <utility>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "pass_internal.h"
#include "kernels.h"
#include "nbest.h"
#include "sample.h"
#include "stats.h"

using namespace tgx::host;
using namespace tgx::dev;

// ---- what the six entry points share ---------------------------------------------------

// A *_corpus entry point, in the order that decides a bad call's status and message: a device, the arguments (`who`
// names the call), *out cleared, one device for both handles, `check` under the model's lock, `run` under the corpus's
// too.  Statistics has no result: it hands in a pointer of its own.
template <class Check, class Run>
static tgx_status on_corpus(const char* who, tgx_model* m, tgx_corpus* c, tgx_result** out, Check check, Run run) {
    if (const tgx_status dst = require_device()) return dst;
    if (!m || !c || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    if (m->device != c->device) return fail(TGX_ERR_INVALID, "model and corpus on different devices");
    std::lock_guard<std::mutex> lk(m->mu);
    const tgx_status st = check();
    if (st != TGX_OK) return st;
    std::lock_guard<std::mutex> lkc(c->mu);
    return run();
}

// A *_batch entry point: a device, the arguments, *out cleared, `check` under the model's lock — released before the
// upload —, then `run` (the call's *_corpus entry point) over the uploaded batch.
template <class Check, class Run>
static tgx_status on_batch(const char* who, tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, tgx_result** out,
                           Check check, Run run) {
    if (const tgx_status dst = require_device()) return dst;
    if (!m || !out) return fail(TGX_ERR_INVALID, "%s: NULL argument", who);
    *out = nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        const tgx_status st = check();
        if (st != TGX_OK) return st;
    }
    return on_uploaded_batch(m, text, offs, n_samples, run);
}

// ---- sampling (sample.hip) ---------------------------------------------------------

double tgx_sample_u01(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len) {
    uint64_t x = seed ^ 0xD6E8FEB86659FD93ULL ^ (sample * 0x9E3779B97F4A7C15ULL) ^ (pos * 0xC2B2AE3D27D4EB4FULL) ^
                 ((uint64_t)len * 0x165667B19E3779F9ULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    const double u = ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;  // (2^53 - 1 + 0.5 rounds to 2^53)
}

// alpha finite and >= 0, scores finite, alpha · score finite; caller holds m->mu
static tgx_status sample_check(const tgx_model* m, double alpha) {
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(TGX_ERR_INVALID, "alpha must be finite and >= 0 (got %g)", alpha);
    if (!m->scores_finite) return fail(TGX_ERR_UNSUPPORTED, "sampling needs every score to be finite");
    for (double sc : m->vocab_scores)
        if (!std::isfinite(alpha * sc)) return fail(TGX_ERR_INVALID, "alpha * score overflows (alpha %g)", alpha);
    return TGX_OK;
}

// what the rows kernels of sampling and statistics ask of the scores: every w = exp(alpha · score) in [2^-300, 2^300]
static bool linear_weights_fit(const tgx_model* m, double alpha) {
    for (double sc : m->vocab_scores)
        if (!(std::fabs(alpha * sc) <= 207.0)) return false;
    return true;
}
// ... and their first step: w by slot of the forward trie into d_wslot (f64[n_slots])
static tgx_status queue_wslot(tgx_model* m, double alpha, double* d_wslot) {
    time_begin(m, "sample_wslot_kernel");
    if (tgx::launch_sample_wslot(m->d_trie, (uint32_t)m->flat.table.size(), alpha, d_wslot, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "sample_wslot_kernel launch failed");
    time_end(m);
    return TGX_OK;
}

// caller holds m->mu and c->mu
static tgx_status sample_corpus_locked(tgx_model* m, tgx_corpus* c, double alpha, uint64_t seed, double* logz, tgx_result** out) {
    HIP_TRY(hipSetDevice(m->device));
    {
        const tgx_status est = ensure_encode_tables(m);
        if (est != TGX_OK) return est;
    }
    m->n_timed = 0;
    const uint64_t S = c->n_samples;
    const uint32_t n_slots = (uint32_t)m->flat.table.size();

    // the rows kernel: tokens <= 32 bytes, the token hash table of the trace, every w = exp(alpha · score) in [2^-300, 2^300]
    bool rows = m->lm <= 32 && m->d_tokhash != nullptr && linear_weights_fit(m, alpha);
    if (const char* e = knob("TGX_SAMPLE_PATH")) {
        if (strcmp(e, "generic") == 0) rows = false;
    }

    Pass pass(m);
    tgx_result* r = pass.new_result(S);
    double* d_logz = nullptr;     // f64[S], then the range flag
    double* d_wslot = nullptr;    // f64[n_slots]
    const size_t lb = (size_t)S * 8 + 16, wb = (size_t)n_slots * 8 + 16;
    if (r->d_offs.alloc(m->device, (size_t)(S + 1) * 8) != hipSuccess || pass.alloc(lb, &d_logz) != hipSuccess ||
        (rows && pass.alloc(wb, &d_wslot) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "out of device memory (sampling)");
    tgx_status st = ensure_scratch(c);
    if (st != TGX_OK) return st;
    unsigned long long* d_range = reinterpret_cast<unsigned long long*>(d_logz + S);
    if (hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream) != hipSuccess || hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess ||
        hipMemsetAsync(d_range, 0x00, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "memset failed");

    const tgx::EncodeParams p = base_encode_params(m, c, seed);
    tgx::SampleParams q{};
    q.alpha = alpha;
    q.logz = d_logz;
    q.wslot = d_wslot;
    q.range_flag = d_range;
    if (rows) {
        if (const tgx_status wst = queue_wslot(m, alpha, d_wslot)) return wst;
        time_begin(m, "sample_rows_kernel");
        if (tgx::launch_sample_rows(p, q, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "sample_rows_kernel launch failed");
        time_end(m);
        unsigned long long range = 0;
        if (hipMemcpyAsync(&range, d_range, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "sampling pass failed: %s", hipGetErrorString(hipGetLastError()));
        if (range) {  // a value the linear domain cannot hold exactly: the whole call on the log-domain kernel
            rows = false;
            if (hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "memset failed");
        } else {
            time_begin(m, "trace32_kernel");
            if (tgx::launch_trace32(p, trace_blocks(m, S), false, m->stream) != hipSuccess)
                return fail(TGX_ERR_DEVICE, "trace32_kernel launch failed");
            time_end(m);
        }
    }
    if (!rows) {
        time_begin(m, "sample_kernel");
        if (tgx::launch_sample(p, q, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "sample_kernel launch failed");
        time_end(m);
    }

    st = compact_ids(m, c, r, "sampling");
    if (st != TGX_OK) return st;
    if ((logz && S && hipMemcpyAsync(logz, d_logz, (size_t)S * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "compact failed: %s", hipGetErrorString(hipGetLastError()));
    m->last_alg_bytes = c->n_bytes + 4 * r->n_tokens + 16 * (S + 1);
    *out = pass.release_result();
    return pass.done();
}

tgx_status tgx_encode_corpus_sample(tgx_model* m, tgx_corpus* c, double alpha, uint64_t seed, double* logz, tgx_result** out) {
    return on_corpus("tgx_encode_corpus_sample", m, c, out, [&] { return sample_check(m, alpha); },
                     [&] { return sample_corpus_locked(m, c, alpha, seed, logz, out); });
}

tgx_status tgx_encode_batch_sample(tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, double alpha,
                                   uint64_t seed, double* logz, tgx_result** out) {
    return on_batch("tgx_encode_batch_sample", m, text, offs, n_samples, out, [&] { return sample_check(m, alpha); },
                    [&](tgx_corpus* c) { return tgx_encode_corpus_sample(m, c, alpha, seed, logz, out); });
}

// ---- lattice statistics (stats.hip) ---------------------------------------------------

// caller holds m->mu and c->mu
static tgx_status stats_corpus_locked(tgx_model* m, tgx_corpus* c, double alpha, double* logz, double* escore, double* etokens,
                                      uint64_t* n_no_path) {
    HIP_TRY(hipSetDevice(m->device));
    m->n_timed = 0;
    const uint64_t S = c->n_samples;
    const uint32_t n_slots = (uint32_t)m->flat.table.size();
    if (S == 0) {  // nothing to launch, nothing to write
        if (n_no_path) *n_no_path = 0;
        return TGX_OK;
    }

    // the rows kernel: tokens <= 32 bytes, every w = exp(alpha · score) in [2^-300, 2^300] (sampling's rule; nothing is
    // traced, so the token hash table is not asked for)
    bool rows = m->lm <= 32 && linear_weights_fit(m, alpha);
    bool forced_rows = false;
    if (const char* e = knob("TGX_STATS_PATH")) {
        if (strcmp(e, "generic") == 0) rows = false;
        if (strcmp(e, "rows") == 0) {
            if (!rows) return fail(TGX_ERR_UNSUPPORTED, "TGX_STATS_PATH=rows: the rows kernel cannot take this model at alpha %g", alpha);
            forced_rows = true;
        }
    }

    Pass pass(m);
    double* d_out = nullptr;    // f64[3 S]: logz, escore, etokens; then the range flag
    double* d_wslot = nullptr;  // f64[n_slots]
    const size_t ob = (size_t)S * 24 + 16, wb = (size_t)n_slots * 8 + 16;
    if (pass.alloc(ob, &d_out) != hipSuccess || (rows && pass.alloc(wb, &d_wslot) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "out of device memory (lattice statistics)");
    unsigned long long* d_range = reinterpret_cast<unsigned long long*>(d_out + 3 * S);
    if (hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream) != hipSuccess || hipMemsetAsync(d_range, 0x00, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "memset failed");

    const tgx::EncodeParams p = base_encode_params(m, c, 0);
    tgx::StatsParams q{};
    q.alpha = alpha;
    q.logz = d_out;
    q.escore = d_out + S;
    q.etokens = d_out + 2 * S;
    q.wslot = d_wslot;
    q.range_flag = d_range;
    if (rows) {
        if (const tgx_status wst = queue_wslot(m, alpha, d_wslot)) return wst;
        time_begin(m, "stats_rows_kernel");
        if (tgx::launch_stats_rows(p, q, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "stats_rows_kernel launch failed");
        time_end(m);
        unsigned long long range = 0;
        if (hipMemcpyAsync(&range, d_range, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "lattice statistics pass failed: %s", hipGetErrorString(hipGetLastError()));
        if (range) {  // a value the linear domain cannot hold exactly: the whole call on the log-domain kernel
            if (forced_rows) return fail(TGX_ERR_UNSUPPORTED, "TGX_STATS_PATH=rows: a value left the range of the rows kernel");
            rows = false;
            if (hipMemsetAsync(&m->d_ctrl->queue, 0x00, 8, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "memset failed");
        }
    }
    if (!rows) {
        time_begin(m, "stats_kernel");
        if (tgx::launch_stats(p, q, (uint32_t)m->num_cus, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "stats_kernel launch failed");
        time_end(m);
    }

    std::vector<double> h_logz;
    if (n_no_path && !logz && S) {  // the count reads logz
        h_logz.resize(S);
        logz = h_logz.data();
    }
    if (S && ((logz && hipMemcpyAsync(logz, q.logz, (size_t)S * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
              (escore && hipMemcpyAsync(escore, q.escore, (size_t)S * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
              (etokens && hipMemcpyAsync(etokens, q.etokens, (size_t)S * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess)))
        return fail(TGX_ERR_DEVICE, "lattice statistics: copy failed: %s", hipGetErrorString(hipGetLastError()));
    if (hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "lattice statistics pass failed: %s", hipGetErrorString(hipGetLastError()));
    if (n_no_path) {
        uint64_t bad = 0;
        for (uint64_t i = 0; i < S; i++) bad += logz[i] == -HUGE_VAL ? 1u : 0u;
        *n_no_path = bad;
    }
    m->last_alg_bytes = c->n_bytes + 24 * S + 8 * (S + 1);
    return pass.done();
}

tgx_status tgx_lattice_stats_corpus(tgx_model* m, tgx_corpus* c, double alpha, double* logz, double* escore, double* etokens,
                                    uint64_t* n_no_path) {
    tgx_result* no_result = nullptr;  // (statistics writes to the caller's arrays)
    return on_corpus("tgx_lattice_stats_corpus", m, c, &no_result, [&] { return sample_check(m, alpha); },
                     [&] { return stats_corpus_locked(m, c, alpha, logz, escore, etokens, n_no_path); });
}

tgx_status tgx_lattice_stats_batch(tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, double alpha, double* logz,
                                   double* escore, double* etokens, uint64_t* n_no_path) {
    tgx_result* no_result = nullptr;
    return on_batch("tgx_lattice_stats_batch", m, text, offs, n_samples, &no_result, [&] { return sample_check(m, alpha); },
                    [&](tgx_corpus* c) { return tgx_lattice_stats_corpus(m, c, alpha, logz, escore, etokens, n_no_path); });
}

// ---- n-best segmentation (nbest.hip) ------------------------------------------------

// caller holds m->mu
static tgx_status nbest_check(const tgx_model* m, uint32_t nbest) {
    if (nbest == 0 || nbest > TGX_MAX_NBEST) return fail(TGX_ERR_INVALID, "nbest must be in 1..%d (got %u)", TGX_MAX_NBEST, nbest);
    if (!m->scores_finite) return fail(TGX_ERR_UNSUPPORTED, "n-best needs every score to be finite");
    if (m->vocab_size >= tgx::kNbestMaxVocab)
        return fail(TGX_ERR_UNSUPPORTED, "n-best supports vocabularies of fewer than %u tokens", tgx::kNbestMaxVocab);
    return TGX_OK;
}

// Scratch of a chunk: K back-pointers per position (N + S positions) and nbest ids per byte.  A call whose scratch would
// exceed the budget is cut at sample boundaries (input order); a sample larger than the budget is a chunk of its own.
static uint64_t nbest_chunk_budget() {
    uint64_t mb = 8192;
    if (const char* e = knob("TGX_NBEST_CHUNK_MB")) {
        const long long v = atoll(e);
        if (v > 0) mb = (uint64_t)v;
    }
    return mb << 20;
}

// caller holds m->mu and c->mu
static tgx_status nbest_corpus_locked(tgx_model* m, tgx_corpus* c, uint32_t k, double* scores, uint32_t* n_found, tgx_result** out) {
    HIP_TRY(hipSetDevice(m->device));
    m->n_timed = 0;
    const uint64_t S = c->n_samples;
    const uint32_t K = k <= 1 ? 1u : k <= 2 ? 2u : k <= 4 ? 4u : k <= 8 ? 8u : 16u;
    const uint64_t rows_all = S * k;
    const uint64_t* ho = c->h_offs.data();

    // chunks [cs[i], cs[i + 1]) of samples in input order
    const uint64_t budget = nbest_chunk_budget();
    std::vector<uint64_t> cs{0};
    uint64_t max_bytes = 0, max_samples = 0;
    {
        uint64_t s0 = 0;
        for (uint64_t s = 0; s < S; s++) {
            const uint64_t bytes = ho[s + 1] - ho[s0], samples = s + 1 - s0;
            const uint64_t need = (bytes + samples) * K * 4 + bytes * k * 4;
            if (s > s0 && need > budget) {
                cs.push_back(s);
                s0 = s;
            }
        }
        cs.push_back(S);
        if (S == 0) cs.assign({0, 0});
        for (size_t i = 0; i + 1 < cs.size(); i++) {
            max_bytes = std::max(max_bytes, ho[cs[i + 1]] - ho[cs[i]]);
            max_samples = std::max(max_samples, cs[i + 1] - cs[i]);
        }
    }
    // every chunk's samples longest first (the order the kernel hands them to its waves)
    std::vector<uint32_t> order(S);
    for (size_t i = 0; i + 1 < cs.size(); i++) {
        std::iota(order.begin() + (long)cs[i], order.begin() + (long)cs[i + 1], (uint32_t)cs[i]);
        std::stable_sort(order.begin() + (long)cs[i], order.begin() + (long)cs[i + 1],
                         [ho](uint32_t a, uint32_t b) { return ho[a + 1] - ho[a] > ho[b + 1] - ho[b]; });
    }

    Pass pass(m);
    tgx_result* r = pass.new_result(rows_all);
    uint32_t *d_bp = nullptr, *d_tmp = nullptr, *d_counts = nullptr, *d_nfound = nullptr, *d_order = nullptr;
    double* d_scores = nullptr;
    void* d_scan = nullptr;
    size_t scan_bytes = 0;
    const bool one_chunk = cs.size() == 2;  // its ids are the result's; else every chunk's ids, gathered at the end
    std::vector<std::pair<uint32_t*, uint64_t>> parts;
    const size_t bpb = (size_t)(max_bytes + max_samples) * K * 4 + 256, tb = (size_t)max_bytes * k * 4 + 256;
    const size_t cb = (size_t)rows_all * 4 + 256, sb = (size_t)rows_all * 8 + 256, nb = (size_t)S * 4 + 256;
    if (tgx::scan_temp_bytes(max_samples * k, &scan_bytes) != hipSuccess) return fail(TGX_ERR_DEVICE, "scan temp-size query failed");
    if (r->d_offs.alloc(m->device, (size_t)(rows_all + 1) * 8) != hipSuccess || pass.alloc(bpb, &d_bp) != hipSuccess ||
        pass.alloc(tb, &d_tmp) != hipSuccess || pass.alloc(cb, &d_counts) != hipSuccess || pass.alloc(sb, &d_scores) != hipSuccess ||
        pass.alloc(nb, &d_nfound) != hipSuccess || pass.alloc(nb, &d_order) != hipSuccess ||
        (scan_bytes && pass.alloc(scan_bytes, &d_scan) != hipSuccess))
        return fail(TGX_ERR_DEVICE, "out of device memory (n-best)");
    if ((S && hipMemcpyAsync(d_order, order.data(), (size_t)S * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
        hipMemsetAsync(r->d_offs, 0, 8, m->stream) != hipSuccess || hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "n-best upload failed");

    tgx::NbestParams p{};
    p.text = c->d_text;
    p.offs = c->d_offs;
    p.trie = m->d_trie;
    p.tokid = m->d_tokid;
    p.root_base = m->flat.table[0].base & ~tgx::kTerminalBit;
    p.n_slots = (uint32_t)m->flat.table.size();
    p.lm = m->lm;
    p.k = k;
    p.bp = d_bp;
    p.tmp = d_tmp;
    p.scores = d_scores;
    p.n_found = d_nfound;
    p.err_sample = &m->d_ctrl->err;
    uint64_t total = 0;
    for (size_t ci = 0; ci + 1 < cs.size() && cs[ci] < cs[ci + 1]; ci++) {
        const uint64_t s0 = cs[ci], ns = cs[ci + 1] - s0, R0 = s0 * k;
        p.order = d_order + s0;
        p.n_samples = ns;
        p.s0 = s0;
        p.byte0 = ho[s0];
        p.chunk_bytes = ho[s0 + ns] - ho[s0];
        p.counts = d_counts + R0;
        time_begin(m, "nbest_kernel");
        if (tgx::launch_nbest(p, K, (uint32_t)m->num_cus, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "nbest_kernel launch failed");
        time_end(m);
        time_begin(m, "nbest_trace_kernel");
        if (tgx::launch_nbest_trace(p, K, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "nbest_trace_kernel launch failed");
        time_end(m);
        time_begin(m, "scan_counts_kernel");
        if (tgx::launch_scan(d_counts + R0, r->d_offs + R0, ns * k, d_scan, scan_bytes, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "scan launch failed");
        time_end(m);
        uint64_t tc = 0;
        if (hipMemcpyAsync(&m->h_ctrl->err, &m->d_ctrl->err, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipMemcpyAsync(&m->h_ctrl->total_tokens, r->d_offs + R0 + ns * k, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "n-best pass failed: %s", hipGetErrorString(hipGetLastError()));
        const tgx_status st = check_no_path(m, c);  // chunks go in input order: the first failing one holds the lowest sample
        if (st != TGX_OK) return st;
        tc = m->h_ctrl->total_tokens;
        uint32_t* ids = nullptr;
        const size_t ib = (size_t)tc * 4 + 256;
        if ((one_chunk ? r->d_ids.alloc(m->device, ib) : pass.alloc(ib, &ids)) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (n-best ids)");
        if (one_chunk) ids = r->d_ids;
        parts.push_back({ids, tc});
        time_begin(m, "nbest_compact_kernel");
        if (tgx::launch_nbest_compact(p, r->d_offs + R0, ids, (uint32_t)m->num_cus, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "nbest_compact_kernel launch failed");
        time_end(m);
        if (total && tgx::launch_offs_add(r->d_offs + R0, ns * k, total, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "offset launch failed");
        total += tc;
    }
    r->n_tokens = total;
    if (!r->d_ids) {
        if (r->d_ids.alloc(m->device, (size_t)total * 4 + 256) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (result ids)");
        uint64_t at = 0;
        for (auto& pt : parts) {
            if (pt.second && hipMemcpyAsync(r->d_ids + at, pt.first, (size_t)pt.second * 4, hipMemcpyDeviceToDevice, m->stream) != hipSuccess)
                return fail(TGX_ERR_DEVICE, "n-best gather failed");
            at += pt.second;
        }
    }
    if ((scores && rows_all && hipMemcpyAsync(scores, d_scores, (size_t)rows_all * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
        (n_found && S && hipMemcpyAsync(n_found, d_nfound, (size_t)S * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "n-best pass failed: %s", hipGetErrorString(hipGetLastError()));
    m->h_ctrl->err = ~0ULL;
    if (hipMemcpy(&m->h_ctrl->err, &m->d_ctrl->err, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "n-best pass failed");
    const tgx_status st = check_no_path(m, c);  // (a corrupt back-pointer found by the trace: never a fault)
    if (st != TGX_OK) return st;
    m->last_alg_bytes = c->n_bytes + 4 * r->n_tokens + 8 * (rows_all + 1) + 12 * rows_all;
    *out = pass.release_result();
    return pass.done();
}

tgx_status tgx_encode_corpus_nbest(tgx_model* m, tgx_corpus* c, uint32_t nbest, double* scores, uint32_t* n_found, tgx_result** out) {
    return on_corpus("tgx_encode_corpus_nbest", m, c, out, [&] { return nbest_check(m, nbest); },
                     [&] { return nbest_corpus_locked(m, c, nbest, scores, n_found, out); });
}

tgx_status tgx_encode_batch_nbest(tgx_model* m, const uint8_t* text, const uint64_t* offs, uint64_t n_samples, uint32_t nbest,
                                  double* scores, uint32_t* n_found, tgx_result** out) {
    return on_batch("tgx_encode_batch_nbest", m, text, offs, n_samples, out, [&] { return nbest_check(m, nbest); },
                    [&](tgx_corpus* c) { return tgx_encode_corpus_nbest(m, c, nbest, scores, n_found, out); });
}
