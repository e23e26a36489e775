// The C ABI's E-step (include/tgx.h: tgx_estep): the tables a model builds at its first E-step, the work list and the
// pieces of a corpus, and the pass on the fused kernel (estep7.hip), the chained kernels (estep4.hip, estep4l.hip,
// encode5.hip) or the generic one (estep.hip).  It runs on the model's own stream under a Pass and takes the knobs and
// the launch arithmetic from tgx_api.cpp (pass_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <unordered_set>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "pass_internal.h"
#include "kernels.h"
#include "trie_build.h"

using namespace tgx::host;
using namespace tgx::dev;

// Builds (once) the double-array of the REVERSED tokens used by the backward sweep.
static tgx_status ensure_reverse_trie(tgx_model* m) {
    if (m->d_trie_rev) return TGX_OK;
    const uint32_t V = m->vocab_size;
    if (!m->rev_host_built) {
        std::vector<uint8_t> rev(m->vocab_bytes.size());
        for (uint32_t i = 0; i < V; i++) {
            const uint64_t b = m->vocab_offs[i], e = m->vocab_offs[i + 1];
            for (uint64_t k = b; k < e; k++) rev[k] = m->vocab_bytes[e - 1 - (k - b)];
        }
        tgx::build_flat_trie(rev.data(), m->vocab_offs.data(), m->vocab_scores.data(), V, &m->flat_rev);
    }
    if (m->flat_rev.table.size() >= (1u << 26)) return fail(TGX_ERR_UNSUPPORTED, "reversed trie needs more than 2^26 slots");
    HIP_TRY(hipSetDevice(m->device));
    const size_t tbytes = m->flat_rev.table.size() * sizeof(tgx::TrieRec);
    HIP_TRY(hipMalloc(&m->d_trie_rev, tbytes));
    HIP_TRY(hipMemcpy(m->d_trie_rev, m->flat_rev.table.data(), tbytes, hipMemcpyHostToDevice));
    int occ = 0;
    HIP_TRY(tgx::estep_max_blocks_per_cu(m->lm, &occ));
    m->estep_blocks_per_cu = std::max(1, std::min(occ, 16));
    HIP_TRY(tgx::estep4_prepare());
    // Linear-domain E-step (estep4l.hip): its tables carry w = exp(score).  Whether a pass can use it
    // (every position has an incoming token, values stay inside the f64 range) is decided per pass by
    // the forward kernel itself; scores beyond +-300 would overflow exp() or underflow within a block.
    bool ok = m->lm <= 32 && m->scores_finite;  // (17..32 bytes: the long-token builds, one position per lane)
    for (uint32_t i = 0; ok && i < V; i++) ok = m->vocab_scores[i] >= -300.0 && m->vocab_scores[i] <= 300.0;
    if (ok) {
        auto upload_weights = [&](const tgx::FlatTrie& ft, void** dst) -> hipError_t {
            std::vector<tgx::TrieRec> w(ft.table);
            for (tgx::TrieRec& r : w) {
                double sc = 0.0, wt = 0.0;
                if (r.base & tgx::kTerminalBit) {
                    memcpy(&sc, &r.score_bits, 8);
                    wt = std::exp(sc);
                }
                memcpy(&r.score_bits, &wt, 8);
            }
            hipError_t e = hipMalloc(dst, w.size() * sizeof(tgx::TrieRec));
            if (e != hipSuccess) return e;
            return hipMemcpy(*dst, w.data(), w.size() * sizeof(tgx::TrieRec), hipMemcpyHostToDevice);
        };
        HIP_TRY(upload_weights(m->flat, &m->d_trie_w));
        HIP_TRY(upload_weights(m->flat_rev, &m->d_trie_rev_w));
        HIP_TRY(tgx::estep4l_prepare());
    }
    m->estep_linear_ok = ok;
    return TGX_OK;
}

// The 8-byte ranked records and the table of w = exp(score value) by rank for estep5_fwd_kernel (encode5.hip): built at
// the first E-step of a model whose vocabulary allows them (tokens of at most 16 bytes, finite scores, at most 65 535
// distinct values, at most 2^21 slots); models created for E-step passes do not have the encode tables.
static tgx_status ensure_estep_trie8(tgx_model* m) {
    if (m->estep_trie8_tried) return TGX_OK;
    m->estep_trie8_tried = true;
    if (!(m->lm <= 16 && m->scores_finite && m->vocab_size && m->flat.table.size() <= tgx::kTrie8MaxSlots)) return TGX_OK;
    {   // more than 65 535 distinct values (every model of a prune run above that many tokens): known after a fraction
        // of a millisecond, not after build_trie8 has sorted them
        std::unordered_set<uint64_t> seen;
        seen.reserve(1u << 17);
        for (uint32_t i = 0; i < m->vocab_size && seen.size() <= tgx::kTrie8MaxValues; i++) {
            uint64_t b;
            memcpy(&b, &m->vocab_scores[i], 8);
            seen.insert(b);
        }
        if (seen.size() > tgx::kTrie8MaxValues) return TGX_OK;
    }
    tgx::Trie8 t8;
    tgx::build_trie8(m->flat, m->vocab_offs.data(), m->vocab_scores.data(), &t8);
    if (!t8.ok) return TGX_OK;
    const size_t ns = t8.rec.size(), nv = t8.values.size();
    std::vector<double> w(nv);
    w[0] = 0.0;  // "no token"
    for (size_t r = 1; r < nv; r++) {
        double v;
        memcpy(&v, &t8.values[r], 8);
        w[r] = std::exp(v);  // the same function of the same double as the weights of the 16-byte tables (upload_weights)
    }
    if (!m->d_trie8) HIP_TRY(hipMalloc(&m->d_trie8, ns * sizeof(tgx::Trie8Rec)));
    if (!m->d_values) HIP_TRY(hipMalloc((void**)&m->d_values, nv * 8));
    if (!m->d_wvalues) HIP_TRY(hipMalloc((void**)&m->d_wvalues, nv * 8));
    HIP_TRY(hipMemcpy(m->d_trie8, t8.rec.data(), ns * sizeof(tgx::Trie8Rec), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_values, t8.values.data(), nv * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_wvalues, w.data(), nv * 8, hipMemcpyHostToDevice));
    {   // (the records are in build_trie8's order again: so is the top table an encode of this model reads)
        const tgx_status tst = upload_top_table(m, t8.rec.data(), ns, t8.root_base);
        if (tst != TGX_OK) return tst;
    }
    m->n_values = (uint32_t)nv - 1u;
    m->root_base8 = t8.root_base;
    if (m->values_ranked || m->value_coverage.empty()) m->value_coverage = std::move(t8.coverage);
    m->values_ranked = false;  // (the tables just written are in build_trie8's order again: the next encode re-ranks them)
    m->have_wvalues = true;
    return TGX_OK;
}

// The E-step's work list of a corpus: every sample cut at multiples of snippet_len (src/prune.rs:83), longest snippet
// first, with its device copies; kept with the corpus (caller holds both locks).
static tgx_status ensure_estep_work(tgx_model* m, tgx_corpus* c, uint64_t snippet_len) {
    tgx_corpus::EstepWork& es = c->es;
    if (es.snippet_len == snippet_len) return TGX_OK;
    const uint64_t S = c->n_samples, N = c->n_bytes;
    {
        es = tgx_corpus::EstepWork{};  // (the old list's buffers go back to the pool)
        es.soffs.reserve(S + N / snippet_len + 2);
        for (uint64_t i = 0; i < S; i++) {
            const uint64_t b = c->h_offs[i], e = c->h_offs[i + 1];
            for (uint64_t o = b; o < e; o += snippet_len) {
                es.soffs.push_back(o);
                es.ssample.push_back((uint32_t)i);
                es.sbase.push_back(o - b);
            }
        }
        const uint64_t K0 = es.soffs.size();
        es.soffs.push_back(N);
        // a snippet's end is the next snippet's start except across empty samples: offsets stay exact
        // because snippets tile [0, N) in order
        es.order.resize(K0);
        std::iota(es.order.begin(), es.order.end(), 0u);
        const std::vector<uint64_t>& so = es.soffs;
        std::stable_sort(es.order.begin(), es.order.end(), [&so](uint32_t a, uint32_t b) {
            return so[a + 1] - so[a] > so[b + 1] - so[b];
        });
        const size_t obytes = (size_t)(K0 + 1) * 8 + 256, ordbytes = (size_t)K0 * 4 + 256;
        if (es.d_soffs.alloc(c->device, obytes) != hipSuccess || es.d_sbase.alloc(c->device, obytes) != hipSuccess ||
            es.d_order.alloc(c->device, ordbytes) != hipSuccess || es.d_ssample.alloc(c->device, ordbytes) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (E-step work list)");
        if (hipMemcpyAsync(es.d_soffs, es.soffs.data(), (K0 + 1) * 8, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
            (K0 && hipMemcpyAsync(es.d_sbase, es.sbase.data(), K0 * 8, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
            (K0 && hipMemcpyAsync(es.d_order, es.order.data(), K0 * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
            (K0 && hipMemcpyAsync(es.d_ssample, es.ssample.data(), K0 * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess) ||
            hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step work list upload failed");
        es.snippet_len = snippet_len;
    }
    return TGX_OK;
}

// ---- pieces (cuts.hip): long snippets cut where no token match crosses — the lattice factorises there.  The buffers
// belong to the pass that built the list.
struct EstepPieces {
    uint64_t n = 0, longest = 0;
    uint64_t *d_bound = nullptr, *d_pos = nullptr, *d_offs = nullptr, *d_base = nullptr;
    uint32_t *d_flag = nullptr, *d_sample = nullptr, *d_snip = nullptr, *d_len = nullptr, *d_idx = nullptr, *d_len2 = nullptr, *d_order = nullptr;
    void *d_scan = nullptr, *d_sort = nullptr;
    double* d_zsnip = nullptr;
    size_t scan_bytes = 0, sort_bytes = 0, zsnip_bytes = 0;
};
// the windows of the corpus's snippets (one boundary is sought per window), kept with the work list
static tgx_status ensure_estep_windows(tgx_model* m, tgx_corpus* c, uint32_t window) {
    tgx_corpus::EstepWork& es = c->es;
    if (es.window == window && es.d_win_snip) return TGX_OK;
    const uint64_t K = es.soffs.size() - 1, N = c->n_bytes;
    es.d_win_snip.reset();
    es.d_win_k.reset();
    es.window = 0;
    std::vector<uint32_t> ws, wk;
    ws.reserve(K + N / window + 2);
    wk.reserve(K + N / window + 2);
    for (uint64_t k = 0; k < K; k++) {
        const uint64_t len = es.soffs[k + 1] - es.soffs[k];
        for (uint64_t j = 0; j * window < len; j++) {
            ws.push_back((uint32_t)k);
            wk.push_back((uint32_t)j);
        }
    }
    es.n_windows = ws.size();
    const size_t winbytes = es.n_windows * 4 + 256;
    if (es.d_win_snip.alloc(c->device, winbytes) != hipSuccess || es.d_win_k.alloc(c->device, winbytes) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (E-step windows)");
    if (hipMemcpyAsync(es.d_win_snip, ws.data(), es.n_windows * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
        hipMemcpyAsync(es.d_win_k, wk.data(), es.n_windows * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "E-step window list upload failed");
    es.window = window;
    return TGX_OK;
}
// cut_windows_kernel, scan, scatter, lengths, longest-first order: the piece list of this pass (dropout decides the
// matches, so the list is per pass).  trie16: a 16-byte-record table of the forward tokens (scores or weights alike).
static tgx_status estep_pieces_build(tgx_model* m, tgx_corpus* c, const void* trie16, double dropout, uint64_t seed, Pass& pass,
                                     EstepPieces* out) {
    tgx_corpus::EstepWork& es = c->es;
    EstepPieces& pc = *out;
    const uint64_t K = es.soffs.size() - 1, N = c->n_bytes;
    const uint64_t W = es.n_windows;
    pc.zsnip_bytes = (size_t)K * 8 + 256;
    auto bad = [&](const char* what) { return fail(TGX_ERR_DEVICE, "E-step pieces: %s", what); };
    if (tgx::scan_temp_bytes(W, &pc.scan_bytes) != hipSuccess || tgx::piece_sort_temp_bytes(W, &pc.sort_bytes) != hipSuccess)
        return bad("scratch sizes");
    if (pass.alloc(W * 8 + 256, &pc.d_bound) != hipSuccess || pass.alloc((W + 1) * 8 + 256, &pc.d_pos) != hipSuccess ||
        pass.alloc((W + 1) * 8 + 256, &pc.d_offs) != hipSuccess || pass.alloc(W * 8 + 256, &pc.d_base) != hipSuccess ||
        pass.alloc((W + 1) * 4 + 256, &pc.d_flag) != hipSuccess || pass.alloc(W * 4 + 256, &pc.d_sample) != hipSuccess ||
        pass.alloc(W * 4 + 256, &pc.d_snip) != hipSuccess || pass.alloc(W * 4 + 256, &pc.d_len) != hipSuccess ||
        pass.alloc(W * 4 + 256, &pc.d_idx) != hipSuccess || pass.alloc(W * 4 + 256, &pc.d_len2) != hipSuccess ||
        pass.alloc(W * 4 + 256, &pc.d_order) != hipSuccess ||
        (pc.scan_bytes && pass.alloc(pc.scan_bytes, &pc.d_scan) != hipSuccess) ||
        (pc.sort_bytes && pass.alloc(pc.sort_bytes, &pc.d_sort) != hipSuccess) ||
        pass.alloc(pc.zsnip_bytes, &pc.d_zsnip) != hipSuccess)
        return bad("out of device memory");
    tgx::CutParams q{};
    q.text = c->d_text;
    q.soffs = es.d_soffs;
    q.snip_sample = es.d_ssample;
    q.snip_base = es.d_sbase;
    q.win_snip = es.d_win_snip;
    q.win_k = es.d_win_k;
    q.n_windows = W;
    q.window = es.window;
    q.trie = trie16;
    q.root = m->flat.table[0].base & ~tgx::kTerminalBit;
    q.lmx = m->lm > 16 ? 32u : 16u;
    q.dropout = dropout;
    q.seed = seed;
    q.bound = pc.d_bound;
    q.flag = pc.d_flag;
    unsigned long long* const d_longest = &m->d_ctrl->longest;
    time_begin(m, "cut_windows_kernel");
    if (tgx::launch_cut_windows(q, m->stream) != hipSuccess) return bad("cut kernel launch failed");
    time_end(m);
    time_begin(m, "piece_list");
    if (hipMemsetAsync(d_longest, 0, 8, m->stream) != hipSuccess || hipMemsetAsync(pc.d_zsnip, 0, pc.zsnip_bytes, m->stream) != hipSuccess ||
        tgx::launch_scan(pc.d_flag, pc.d_pos, W, pc.d_scan, pc.scan_bytes, m->stream) != hipSuccess ||
        tgx::launch_cut_scatter(q, pc.d_pos, N, pc.d_offs, pc.d_sample, pc.d_base, pc.d_snip, m->stream) != hipSuccess ||
        tgx::launch_piece_len(pc.d_offs, pc.d_pos + W, pc.d_len, pc.d_idx, d_longest, W, m->stream) != hipSuccess ||
        tgx::piece_sort(pc.d_sort, pc.sort_bytes, pc.d_len, pc.d_len2, pc.d_idx, pc.d_order, W, m->stream) != hipSuccess)
        return bad("piece list kernels failed");
    time_end(m);
    unsigned long long h_n = 0, h_longest = 0;
    if (hipMemcpyAsync(&h_n, pc.d_pos + W, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipMemcpyAsync(&h_longest, d_longest, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return bad("piece list read-back failed");
    if (h_n < K || h_n > W) return bad("inconsistent piece count");
    pc.n = h_n;
    pc.longest = h_longest;
    return TGX_OK;
}

// The token-ranked records and weights of estep7_kernel (estep7.hip): vocabularies with finite scores within +-300
// (w = exp(score) and its products must stay inside the f64 range, as for the other linear-domain kernels) and tokens of
// at most 16 bytes.  ~40 ns of host time per token.
// The 8-byte records of estep7_kernel.  Built at the model's first E-step, where there is text: the ranks that the kernels
// keep in LDS are the tokens that MATCH most often in a sample of the corpus (match_count_kernel) — every match is one add
// to the token's expected count, whatever its score, and adds outside LDS are memory-side atomics that queue up per
// address.  (Ranked by exp(score) / length, prune's second sub-iteration at 500 000 entries — M-step scores — left one
// token with 1.9 M matches outside: 61 ms against the first sub-iteration's 13; ranked by the probability mass below
// the token's node, 74 ms.)
static tgx_status ensure_estep_trie8t(tgx_model* m, const tgx_corpus* c) {
    if (m->trie8t_tried) return TGX_OK;
    m->trie8t_tried = true;
    if (!(m->lm <= 16 && m->scores_finite && m->vocab_size && m->flat.table.size() <= tgx::kTrie8TMaxSlots)) return TGX_OK;
    for (uint32_t i = 0; i < m->vocab_size; i++)
        if (!(m->vocab_scores[i] >= -300.0 && m->vocab_scores[i] <= 300.0)) return TGX_OK;
    tgx::HostPhases hp("ensure_estep_trie8t");
    tgx::Trie8T t8;
    tgx::build_trie8t(m->flat, m->vocab_offs.data(), m->vocab_scores.data(), &t8);
    if (!t8.ok || t8.n_tok == 0) return TGX_OK;
    hp.mark("build_trie8t");
    HIP_TRY(hipSetDevice(m->device));
    const size_t ns = t8.rec.size(), nw = t8.w.size();
    if (!m->d_trie8t) HIP_TRY(hipMalloc(&m->d_trie8t, ns * sizeof(tgx::Trie8TRec)));
    if (!m->d_wtab) HIP_TRY(hipMalloc((void**)&m->d_wtab, nw * 8));
    HIP_TRY(hipMemcpy(m->d_trie8t, t8.rec.data(), ns * sizeof(tgx::Trie8TRec), hipMemcpyHostToDevice));
    hp.mark("upload records");
    const char* norank = knob("TGX_E7_RANK");  // "model": keep build_trie8t's order (measurements)
    if (c && c->n_bytes && !(norank && strcmp(norank, "model") == 0)) {
        // up to 64 chunks of 64 KiB spread over the corpus (4 MiB: ~13 M matches)
        const uint32_t chunk = 65536u;
        const uint64_t stride = std::max<uint64_t>(chunk, (c->n_bytes + 63) / 64);
        const size_t cb = nw * 4 + 256;
        Pass pass(m);
        unsigned int* d_cnt = nullptr;
        uint32_t* d_perm = nullptr;
        if (pass.alloc(cb, &d_cnt) != hipSuccess || pass.alloc(cb, &d_perm) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (match counts)");
        std::vector<unsigned int> cnt(nw, 0u);
        if (hipMemsetAsync(d_cnt, 0, cb, m->stream) != hipSuccess ||
            tgx::launch_match_count(c->d_text, c->n_bytes, chunk, stride, m->d_trie8t, (uint32_t)ns, t8.root_base, t8.n_tok, d_cnt, (uint32_t)m->num_cus, m->stream) != hipSuccess ||
            hipMemcpyAsync(cnt.data(), d_cnt, nw * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "match count pass failed: %s", hipGetErrorString(hipGetLastError()));
        hp.mark("match counts");
        // new order: the kTrie8TSortedRanks most matched tokens by descending count (ties: the old rank), the others as they were
        const uint32_t n_tok = t8.n_tok;
        std::vector<uint32_t> order(n_tok);
        for (uint32_t r = 0; r < n_tok; r++) order[r] = r + 1u;
        const auto hotter = [&](uint32_t a, uint32_t b) { return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : a < b; };
        const size_t head = std::min<size_t>(n_tok, tgx::kTrie8TSortedRanks);
        if (head < n_tok) {
            std::nth_element(order.begin(), order.begin() + (long)head, order.end(), hotter);
            // the others in their old order, without a sort: mark the head, read the marks in order
            std::vector<uint8_t> in_head(nw, 0);
            for (size_t i = 0; i < head; i++) in_head[order[i]] = 1;
            size_t k = head;
            for (uint32_t r = 1; r <= n_tok; r++)
                if (!in_head[r]) order[k++] = r;
        }
        std::sort(order.begin(), order.begin() + (long)head, hotter);
        std::vector<uint32_t> perm(nw, 0u);
        std::vector<double> w2(nw, 0.0);
        std::vector<uint32_t> id2(nw, tgx::kNoToken);
        unsigned long long all_matches = 0, far_matches = 0;
        for (uint32_t r = 0; r < n_tok; r++) {
            perm[order[r]] = r + 1u;
            w2[r + 1u] = t8.w[order[r]];
            id2[r + 1u] = t8.id_of_rank[order[r]];
            all_matches += cnt[order[r]];
            if (r + 1u > 65535u) far_matches += cnt[order[r]];
        }
        m->e7_overflow_share = all_matches ? (double)far_matches / (double)all_matches : 0.0;
        t8.w.swap(w2);
        t8.id_of_rank.swap(id2);
        if (hipMemcpyAsync(d_perm, perm.data(), nw * 4, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
            tgx::launch_rank_remap(m->d_trie8t, (uint32_t)ns, d_perm, ~0u, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "rank remap failed: %s", hipGetErrorString(hipGetLastError()));
        pass.done();
        hp.mark("re-rank");
    }
    HIP_TRY(hipMemcpy(m->d_wtab, t8.w.data(), nw * 8, hipMemcpyHostToDevice));
    m->id_of_rank = std::move(t8.id_of_rank);
    m->n_tok7 = t8.n_tok;
    m->root_base7 = t8.root_base;
    m->have_trie8t = true;
    return TGX_OK;
}

// Whether this pass cuts its snippets into pieces, and then their list (pc->n != 0: cut; m->last_estep_pieces says the
// same).  A pass cuts when its longest snippet spans more than four windows and `worth` says that its serial chain is a
// sizeable part of the pass; TGX_ESTEP_PIECES=0 / 1 forces, TGX_ESTEP_WINDOW sets the window.
static tgx_status estep_pieces_if_worth(tgx_model* m, tgx_corpus* c, uint32_t window, const void* trie16, bool (*worth)(double longest0, double n_bytes),
                                        double dropout, uint64_t seed, Pass& pass, EstepPieces* pc) {
    const tgx_corpus::EstepWork& es = c->es;
    if (const char* e = knob("TGX_ESTEP_WINDOW")) window = (uint32_t)std::min(1 << 20, std::max(256, atoi(e)));
    const double longest0 = (double)(es.soffs[es.order[0] + 1] - es.soffs[es.order[0]]);
    bool pieces = longest0 > 4.0 * window && worth(longest0, (double)c->n_bytes);
    if (const char* e = knob("TGX_ESTEP_PIECES")) pieces = atoi(e) != 0 && longest0 > (double)window;
    if (pieces) {
        tgx_status st = ensure_estep_windows(m, c, window);
        if (st != TGX_OK) return st;
        st = estep_pieces_build(m, c, trie16, dropout, seed, pass, pc);
        if (st != TGX_OK) return st;
    }
    m->last_estep_pieces = pc->n;
    return TGX_OK;
}

// The end of an E-step pass, the same on every path: the lowest failing snippet (into m->h_ctrl->err), the h->size() counts
// at d_counts and log Z come back with one synchronisation — with them the linear-domain kernels' range flag where
// `range_flag` is given.  The caller looks at the range flag, then at estep_z_failure, and only then adds to `expected`.
static tgx_status estep_read_back(tgx_model* m, const tgx_corpus* c, const double* d_counts, std::vector<double>* h, const double* d_z, double* hz,
                                  unsigned long long* range_flag) {
    if (hipMemcpyAsync(&m->h_ctrl->err, &m->d_ctrl->err, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        (range_flag && hipMemcpyAsync(range_flag, &m->d_ctrl->estep.range_flag, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess) ||
        hipMemcpyAsync(h->data(), d_counts, h->size() * 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipMemcpyAsync(hz, d_z, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "E-step pass failed: %s", hipGetErrorString(hipGetLastError()));
    m->last_alg_bytes = c->n_bytes + 8 * (c->n_samples + 1) + 8ull * m->vocab_size;  // N + 8 (S + 1) + 8 V
    return TGX_OK;
}
// TGX_ERR_Z_NOT_NORMAL if the pass read back found a snippet (snip_sample: its sample; nullptr: the units are samples)
// whose normalisation constant is not a normal number: nothing of such a pass may reach the caller's `expected` or log Z.
static tgx_status estep_z_failure(const tgx_model* m, const tgx_corpus* c, const uint32_t* snip_sample) {
    const unsigned long long bad = m->h_ctrl->err;
    if (bad == ~0ULL) return TGX_OK;
    const uint64_t smp = snip_sample ? snip_sample[bad] : bad;
    const uint64_t len = c->h_offs[smp + 1] - c->h_offs[smp];
    set_error_detail(smp, len, len);
    return fail(TGX_ERR_Z_NOT_NORMAL, "normalization constant is not a normal number (sample %llu, len=%llu)",
                (unsigned long long)smp, (unsigned long long)len);  // the reference panics here: src/prune.rs:90-96
}
// counts by slot of the reversed trie -> expected[id]
static void add_slot_counts(const tgx_model* m, const std::vector<double>& h, double* expected) {
    for (size_t t = 0; t < h.size(); t++) {
        const uint32_t id = m->flat_rev.tokid[t];
        if (id != tgx::kNoToken) expected[id] += h[t];
    }
}

// E-step on estep7_kernel (estep7.hip): one walk per position, every trip of a row a lattice of its own.  Caller holds
// both locks.  `fallback`: the chained kernels must do the pass (no records for this vocabulary, a position nothing
// reaches, a value out of range); `expected` is untouched then.
static tgx_status estep_fused(tgx_model* m, tgx_corpus* c, uint64_t snippet_len, double dropout, uint64_t seed, double* expected,
                              double* logz_sum, bool* fallback) {
    *fallback = false;
    tgx::HostPhases hp("estep_fused");
    Pass pass(m);
    {
        const tgx_status tst = ensure_estep_trie8t(m, c);
        if (tst != TGX_OK) return tst;
        if (!m->have_trie8t) {
            *fallback = true;
            return pass.done();
        }
        hp.mark("trie8t");
        const tgx_status wst = ensure_estep_work(m, c, snippet_len);
        if (wst != TGX_OK) return wst;
        hp.mark("work list");
    }
    tgx_corpus::EstepWork& es = c->es;
    const uint64_t S = c->n_samples, N = c->n_bytes, K = es.soffs.size() - 1;
    m->last_estep_pieces = 0;
    m->last_estep_redo = 0;
    if (K == 0) {
        if (logz_sum) *logz_sum = 0.0;
        m->last_alg_bytes = N + 8 * (S + 1) + 8ull * m->vocab_size;
        return pass.done();
    }
    // A piece is a chain of trips (~0.12 us per byte: a 64 KiB snippet takes ~8 ms) while a pass runs at ~33 GB/s: long
    // snippets are cut where no match crosses (cuts.hip) when the longest chain is a sizeable part of the pass — 256 MiB:
    // 21.2 -> 8.6 ms; 1 GiB: 33.6 ms uncut, 34.3 cut (the cut search and the piece list cost 0.5 - 0.8 ms).  Windows of
    // 4 KiB: 8.64 ms at 256 MiB against 8.91 with 2 KiB and 9.23 with 1 KiB (profiles/r04)
    EstepPieces pc;
    {
        const auto worth = [](double longest0, double n_bytes) { return longest0 * 0.12e-6 > 0.4 * (n_bytes / 33e9); };
        const tgx_status pst = estep_pieces_if_worth(m, c, 4096, m->d_trie, worth, dropout, seed, pass, &pc);
        if (pst != TGX_OK) return pst;
    }
    const bool pieces = pc.n != 0;
    const uint64_t units = pieces ? pc.n : K;
    // 16-bit match entries hold 65 535 ranks.  A vocabulary of a few more tokens (the usual "64 K": 65 536) keeps them — 34
    // against 24 GB/s with 32-bit entries — and leaves the trips in which one of its least matched tokens (the ranks beyond
    // 65 535: the tokens are ranked by match counts) matches to the redo kernel, which has 32-bit entries then.
    // TGX_E7_OVF_AT=<rank> (tests) makes the ranks beyond <rank> such tokens.
    uint32_t ovf_limit = 0xFFFFFFFFu;
    // (only while those tokens are rare in the text: a trip holds ~150 matches, the redo kernel is several times slower per trip)
    if (m->n_tok7 > 65535u && m->n_tok7 <= 65535u + 1024u && m->e7_overflow_share < 1e-4) ovf_limit = 65535u;
    if (const char* e = knob("TGX_E7_OVF_AT")) {
        const long v = atol(e);
        if (v >= 1 && v <= 65535 && m->n_tok7 <= 65535u + 1024u) ovf_limit = (uint32_t)v;
        if (v == 0) ovf_limit = 0xFFFFFFFFu;
    }
    bool ovf = ovf_limit < m->n_tok7;
    const bool wide = m->n_tok7 > 65535u && !ovf;
    const bool wide_redo = wide || ovf;
    // (1 GiB, 32 000 entries: 12 waves x 4 positions per lane 32.5 ms, 10 waves 36.2, 8 waves 41.7; three positions per lane
    // 34.2 / 38.5 / 44.3 and forty times the stretches without a cut in a trip — profiles/r04)
    int ppl = wide ? 2 : 4, waves = 12;
    const bool ppl_forced = ovf;  // (the overflow build exists for four positions per lane)
    knob_int("TGX_EPPL", 1, 4, &ppl);
    if (ppl_forced) ppl = 4;
    knob_int("TGX_E7_WAVES", 1, 12, &waves);
    waves = waves_for_units(waves, units, (uint64_t)m->num_cus);
    // (32-bit entries take twice the LDS: the geometry must leave room for a table worth having)
    while (waves > 1 && tgx::estep7_max_hot(wide, waves, ppl, 160u * 1024u) < 1024u) waves--;
    uint32_t n_hot = std::min(m->n_tok7, tgx::estep7_max_hot(wide, waves, ppl, 160u * 1024u));
    n_hot = knob_cap_hot("TGX_E7_HOT", n_hot);
    if (ovf && n_hot >= m->n_tok7) n_hot = m->n_tok7 - 1u;  // (the overflow build is a COLD build)
    const size_t ebytes = ((size_t)m->n_tok7 + 1) * 8 + 256, zbytes = (size_t)K * 8 + 256;
    // (the redo list: a piece can leave several stretches, each longer than a trip's reach)
    const uint64_t redo_cap = units + N / 32 + 16;
    const size_t r8 = (size_t)redo_cap * 2 * 8 + 256, r4 = (size_t)redo_cap * 2 * 4 + 256;
    double *d_exp = nullptr, *d_z = nullptr, *d_zsnip = nullptr;
    void* d_work = nullptr;  // Estep7Work in device memory (kernels.h)
    uint64_t *d_roffs = nullptr, *d_rbase = nullptr;
    uint32_t *d_rsample = nullptr, *d_rsnip = nullptr;
    static_assert(sizeof(tgx::Estep7Work) <= 512, "Estep7Work scratch");
    if (pass.alloc(ebytes, &d_exp) != hipSuccess || pass.alloc(256, &d_z) != hipSuccess || pass.alloc(512, &d_work) != hipSuccess ||
        pass.alloc(zbytes, &d_zsnip) != hipSuccess || pass.alloc(r8, &d_roffs) != hipSuccess || pass.alloc(r8, &d_rbase) != hipSuccess ||
        pass.alloc(r4, &d_rsample) != hipSuccess || pass.alloc(r4, &d_rsnip) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (E-step scratch)");
    if (hipMemsetAsync(d_exp, 0, ebytes, m->stream) != hipSuccess || hipMemsetAsync(d_z, 0, 256, m->stream) != hipSuccess ||
        hipMemsetAsync(d_zsnip, 0, zbytes, m->stream) != hipSuccess || hipMemsetAsync(&m->d_ctrl->estep, 0x00, sizeof(DeviceCtrl::Estep), m->stream) != hipSuccess ||
        hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "E-step setup failed");
    tgx::Estep7Params p{};
    tgx::Estep7Work& wk = p.host_work;
    p.text = c->d_text;
    p.work = reinterpret_cast<const tgx::Estep7Work*>(d_work);
    wk.soffs = pieces ? pc.d_offs : es.d_soffs;
    wk.order = pieces ? pc.d_order : es.d_order;
    wk.n_snips = units;
    wk.snip_sample = pieces ? pc.d_sample : es.d_ssample;
    wk.snip_base = pieces ? pc.d_base : es.d_sbase;
    wk.snip_of = pieces ? pc.d_snip : nullptr;
    p.trie8t = m->d_trie8t;
    p.n_slots = (uint32_t)m->flat.table.size();
    p.root_base = m->root_base7;
    p.wtab = m->d_wtab;
    p.n_tok = m->n_tok7;
    p.n_hot = n_hot;
    p.ovf_limit = ovf ? ovf_limit : 0xFFFFFFFFu;
    p.expected = d_exp;
    wk.zsnip = d_zsnip;
    wk.logz_sum = d_z;
    wk.queue = &m->d_ctrl->estep.queue;
    wk.redo_count = &m->d_ctrl->estep.redo_count;
    wk.range_flag = &m->d_ctrl->estep.range_flag;
    wk.redo_offs = d_roffs;
    wk.redo_sample = d_rsample;
    wk.redo_base = d_rbase;
    wk.redo_snip = d_rsnip;
    wk.redo_cap = redo_cap;
    p.dropout = dropout;
    p.seed = seed;
    p.claim_chunk = claim_chunk_for(N, units);
    const uint64_t rows_per_block = 4ull * (uint64_t)waves;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((units + rows_per_block - 1) / rows_per_block, (uint64_t)m->num_cus));
    const Stamps stamps = stamps_begin(m, pass, '7', (size_t)blocks * (size_t)waves);
    p.stamps = stamps.d;
    p.flags = debug_flags();
    hp.mark("pieces + buffers");
    time_begin(m, "estep7_kernel");
    if (tgx::launch_estep7(p, wide, ppl, waves, blocks, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "estep7 launch failed");
    time_end(m);
    if (stamps.d) stamps_report(m, stamps, ppl, "estep7 stamps", "trip", {"claim", "walk", "cut", "forward", "z", "backward"});
    unsigned long long flag = 0, n_redo = 0;
    if (hipMemcpyAsync(&flag, &m->d_ctrl->estep.range_flag, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipMemcpyAsync(&n_redo, &m->d_ctrl->estep.redo_count, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "E-step pass failed: %s", hipGetErrorString(hipGetLastError()));
    m->last_estep_redo = n_redo;
    if (flag != 0) {  // a position nothing reaches, a value out of range: the pass belongs to the log-domain kernels
        *fallback = true;
        return pass.done();
    }
    if (n_redo != 0) {
        // the stretches the kernel could not close within a trip: estep7_redo_kernel, trips spilled to scratch
        if (n_redo > redo_cap) return fail(TGX_ERR_DEVICE, "E-step redo list longer than its buffers");
        std::vector<uint64_t> ro(2 * n_redo), tbase(n_redo + 1, 0);
        if (hipMemcpy(ro.data(), d_roffs, 2 * n_redo * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(TGX_ERR_DEVICE, "redo list read-back failed");
        for (uint64_t i = 0; i < n_redo; i++) {
            if (ro[2 * i + 1] < ro[2 * i] || ro[2 * i + 1] > N) return fail(TGX_ERR_DEVICE, "corrupt E-step redo list");
            tbase[i + 1] = tbase[i] + (ro[2 * i + 1] - ro[2 * i]) / 16 + 1;
        }
        const uint64_t TT = tbase[n_redo];
        const size_t rs = wide_redo ? 1024 : 512;
        const size_t ab = (size_t)TT * 16 * 8 + 256, xb = (size_t)TT * 4 + 256, mb = (size_t)TT * rs + 256, tbb = (size_t)(n_redo + 1) * 8 + 256;
        double* d_alpha = nullptr;
        int32_t* d_aexp = nullptr;
        unsigned char* d_ms = nullptr;
        uint64_t* d_tbase = nullptr;
        if (pass.alloc(ab, &d_alpha) != hipSuccess || pass.alloc(xb, &d_aexp) != hipSuccess || pass.alloc(mb, &d_ms) != hipSuccess ||
            pass.alloc(tbb, &d_tbase) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "out of device memory (E-step redo scratch)");
        if (hipMemcpyAsync(d_tbase, tbase.data(), (n_redo + 1) * 8, hipMemcpyHostToDevice, m->stream) != hipSuccess ||
            hipMemsetAsync(&m->d_ctrl->estep.queue, 0x00, 8, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step redo setup failed");
        tgx::Estep7RedoParams q{};
        q.text = c->d_text;
        q.redo_offs = d_roffs;
        q.redo_sample = d_rsample;
        q.redo_base = d_rbase;
        q.redo_snip = d_rsnip;
        q.n_redo = n_redo;
        q.tbase = d_tbase;
        q.trie8t = m->d_trie8t;
        q.n_slots = p.n_slots;
        q.root_base = p.root_base;
        q.wtab = m->d_wtab;
        q.n_tok = m->n_tok7;
        q.n_hot = std::min(std::min(m->n_tok7, tgx::estep7_redo_max_hot(wide_redo)), n_hot);
        q.expected = d_exp;
        q.zsnip = d_zsnip;
        q.logz_sum = d_z;
        q.range_flag = &m->d_ctrl->estep.range_flag;
        q.queue = &m->d_ctrl->estep.queue;
        q.alpha = d_alpha;
        q.aexp = d_aexp;
        q.mscratch = d_ms;
        q.dropout = dropout;
        q.seed = seed;
        time_begin(m, "estep7_redo_kernel");
        const hipError_t le = tgx::launch_estep7_redo(q, wide_redo, (uint32_t)m->num_cus, m->stream);
        time_end(m);
        if (le != hipSuccess) return fail(TGX_ERR_DEVICE, "estep7 redo launch failed: %s", hipGetErrorString(le));
        if (hipMemcpyAsync(&flag, &m->d_ctrl->estep.range_flag, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step redo pass failed");
        (void)hipStreamSynchronize(m->stream);
        if (hipGetLastError() != hipSuccess) return fail(TGX_ERR_DEVICE, "E-step redo pass failed");
        if (flag != 0) {
            *fallback = true;
            return pass.done();
        }
    }
    hp.mark("kernel + redo");
    if (tgx::launch_snip_z_check(d_zsnip, K, &m->d_ctrl->err, m->stream) != hipSuccess) return fail(TGX_ERR_DEVICE, "z check launch failed");
    std::vector<double> h((size_t)m->n_tok7 + 1);
    double hz = 0.0;
    tgx_status st = estep_read_back(m, c, d_exp, &h, d_z, &hz, nullptr);
    if (st == TGX_OK) st = estep_z_failure(m, c, es.ssample.data());
    if (st != TGX_OK) return st;
    hp.mark("download");
    for (uint32_t r = 1; r <= m->n_tok7; r++) expected[m->id_of_rank[r]] += h[r];
    hp.mark("rank -> id");
    if (logz_sum) *logz_sum = hz;
    m->estep_calls++;
    return pass.done();
}

// E-step on the four-snippets-per-wave kernels (estep4.hip).  Caller holds m->mu and has
// built the reversed trie.
// `fallback` (vocabularies with tokens of 17..32 bytes only): set when the linear-domain kernels cannot do the
// pass (a position without an incoming token, the f64 range left, an overflow list full) — there are no log-domain
// rows4 kernels for such vocabularies, the caller goes on to the generic kernel; `expected` is untouched then.
static tgx_status estep_rows4(tgx_model* m, tgx_corpus* c, uint64_t snippet_len, double dropout,
                              uint64_t seed, double* expected, double* logz_sum, bool* fallback) {
    const bool long_tokens = m->lm > 16;
    if (fallback) *fallback = false;
    const uint64_t N = c->n_bytes;
    Pass pass(m);
    {
        const tgx_status wst = ensure_estep_work(m, c, snippet_len);
        if (wst != TGX_OK) return wst;
    }
    tgx_corpus::EstepWork& es = c->es;
    const std::vector<uint64_t>& soffs = es.soffs;
    const std::vector<uint32_t>& ssample = es.ssample;
    const std::vector<uint32_t>& order = es.order;
    const uint64_t K = soffs.size() - 1;
    uint64_t* const d_soffs = es.d_soffs;
    uint64_t* const d_sbase = es.d_sbase;
    uint32_t* const d_order = es.d_order;
    uint32_t* const d_ssample = es.d_ssample;
    const size_t n_rev = m->flat_rev.table.size();
    // TGX_ESTEP=log keeps the log-domain kernels (A/B timing, tests of both)
    const char* force_log = knob("TGX_ESTEP");
    const bool linear = m->estep_linear_ok && !(force_log && strcmp(force_log, "log") == 0);

    // ---- pieces (cuts.hip): a pass bound by the serial chains of its longest snippets cuts them where no token match
    // crosses — the lattice factorises there — and runs the linear-domain kernels on pieces of about `window` bytes.
    // Estimates as below (1 position per lane: forward 52 GB/s and 14.5 ms per 64 KiB of chain, backward 21 GB/s and
    // 29 ms); TGX_ESTEP_PIECES=0 / 1 forces, TGX_ESTEP_WINDOW sets the window.
    EstepPieces pc;
    m->last_estep_pieces = 0;
    if (linear && K && m->lm <= 32) {
        // (measured, 32 000 entries, samples <= 64 KiB: 64 MiB 31.3 -> 4.1 ms, 256 MiB 33.0 -> 14.4, 512 MiB 44.8 -> 28.3,
        // 1 GiB 57.1 -> 57.2: the longest chains delay a pass well before they bound it — profiles/r03)
        const auto worth = [](double longest0, double n_bytes) {
            const double t_chain = longest0 / 65536.0 * (9.0 + 20.9) * 1e-3;  // the best chains of either kernel
            const double t_thru = n_bytes / 52e9 + n_bytes / 21e9;
            return t_chain > 0.5 * t_thru;
        };
        const tgx_status pst = estep_pieces_if_worth(m, c, 2048, m->d_trie_w, worth, dropout, seed, pass, &pc);
        if (pst != TGX_OK) return pst;
    }
    const bool pieces = pc.n != 0;
    const uint64_t Kmax = pieces ? std::max<uint64_t>(K, pc.n) : K;
    // replicas of the expected-count array (see estep4_bwd_kernel): up to 256, within 512 MiB
    // (round 3: 2.  The 256 of round 1 kept a handful of very frequent tokens from serialising every wave's atomics; those
    // are summed in the blocks' LDS since round 2, and the remaining memory-side adds are faster on a small array:
    // backward kernel 38.3 ms per GiB with 256 replicas, 36.9 with 4, 36.2 with 2, 35.9 with 1 — profiles/r03/r_*)
    uint32_t n_rep = 2;
    if (const char* e = knob("TGX_ESTEP_REPLICAS")) n_rep = (uint32_t)std::min(256, std::max(1, atoi(e)));
    while (n_rep > 1 && (size_t)n_rep * n_rev * 8 > (512ull << 20)) n_rep >>= 1;
    const size_t abytes = (size_t)(N + Kmax + 128) * 8, ebytes = (size_t)(n_rep + 1) * n_rev * 8 + 256, zbytes = (size_t)Kmax * 8 + 256;
    double *d_alpha = nullptr, *d_exp = nullptr, *d_z = nullptr, *d_zarr = nullptr;
    int32_t* d_aexp = nullptr;  // block exponents of alpha (linear-domain kernels)
    const size_t xbytes = (size_t)((N >> 4) + Kmax + 128) * 4;
    if (pass.alloc(abytes, &d_alpha) != hipSuccess || (linear && pass.alloc(xbytes, &d_aexp) != hipSuccess) ||
        pass.alloc(ebytes, &d_exp) != hipSuccess || pass.alloc(256, &d_z) != hipSuccess || pass.alloc(zbytes, &d_zarr) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (E-step scratch)");
    if (hipMemsetAsync(d_exp, 0, ebytes, m->stream) != hipSuccess ||
        hipMemsetAsync(d_z, 0, 256, m->stream) != hipSuccess ||
        hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "E-step setup copies failed");
    tgx::Estep4Params p{};
    p.text = c->d_text;
    p.soffs = d_soffs;
    p.order = d_order;
    p.n_snips = K;
    p.snip_sample = d_ssample;
    p.snip_base = d_sbase;
    p.trie_fwd = linear ? m->d_trie_w : m->d_trie;
    p.trie_rev = linear ? m->d_trie_rev_w : m->d_trie_rev;
    p.alpha_exp = d_aexp;
    p.root_fwd = m->flat.table[0].base & ~tgx::kTerminalBit;
    p.root_rev = m->flat_rev.table[0].base & ~tgx::kTerminalBit;
    p.alpha = d_alpha;
    p.zarr = d_zarr;
    p.expected_slot = d_exp;
    p.n_slots_rev = (uint32_t)n_rev;
    p.n_replicas = n_rep;
    p.logz_sum = d_z;
    p.err_snip = &m->d_ctrl->err;
    p.queue_fwd = &m->d_ctrl->estep.queue;
    p.queue_bwd = &m->d_ctrl->estep.queue_bwd;
    p.range_flag = &m->d_ctrl->estep.range_flag;
    p.flags = debug_flags();
    p.dropout = dropout;
    p.seed = seed;
    // The linear-domain kernels are tried first; if some position of some snippet has no incoming token
    // (lattice.rs:255's 0.0 case, e.g. a byte that is no token) or a value left the f64 range, the forward
    // kernel says so and the pass is redone with the log-domain kernels.
    // Positions per lane of the linear-domain kernels, chosen per kernel like encode4_kernel's: the longest
    // snippet is a serial chain (forward 14.5 / 11 / 9 ms, backward 29 / 23 / 23.5 ms per 64 KiB at 1 / 2 / 4
    // positions per lane) while more positions per lane cost waves (forward 52 / 48 / 33 GB/s, backward
    // 21 / 16 / 11 GB/s): tools/eppl_sweep.py on 1 x MI355X.  TGX_EPPL overrides both.
    int eppl_fwd = 1, eppl_bwd = 1;
    {
        const double longest = pieces ? (double)pc.longest / 65536.0 : (K ? (double)(soffs[order[0] + 1] - soffs[order[0]]) / 65536.0 : 0.0);
        const double f_gbps[3] = {52.0, 48.0, 33.0}, f_chain[3] = {14.5, 11.0, 9.0};
        // (the backward kernel with 2 positions per lane runs 8 groups of 16 positions per block and sums 8192
        // slots in LDS: tools/bwd_groups_sweep.py)
        const double b_gbps[3] = {21.0, 12.7, 11.0}, b_chain[3] = {29.0, 20.9, 23.5};
        double bf = 0, bb = 0;
        for (int i = 0; i < 3; i++) {
            const double tf = std::max((double)N / (f_gbps[i] * 1e6), longest * f_chain[i]);
            const double tb = std::max((double)N / (b_gbps[i] * 1e6), longest * b_chain[i]);
            if (i == 0 || tf < bf * 0.95) { bf = tf; eppl_fwd = 1 << i; }
            if (i == 0 || tb < bb * 0.95) { bb = tb; eppl_bwd = 1 << i; }
        }
        if (const char* e = knob("TGX_EPPL")) {
            const int v = atoi(e);
            if (v == 1 || v == 2 || v == 4) eppl_fwd = eppl_bwd = v;
        }
    }
    // Forward sweep on the 8-byte ranked records (encode5.hip: estep5_fwd_kernel) where the vocabulary has them; the
    // geometry as for encode5_kernel: every w in LDS with four positions per lane on 16..13 waves, three on 13, two
    // on 16, else three on 16 with the hottest in LDS (COLD build).  TGX_ESTEP_FWD=rows4 keeps estep4l_fwd_kernel.
    bool use5f = false, cold5f = false;
    int ppl5f = 4, waves5f = 16;
    tgx::Encode5Params q5f{};
    uint32_t blocks5f = 1;
    if (linear && !long_tokens && c->max_len < (1ull << 32)) {
        const char* ff = knob("TGX_ESTEP_FWD");
        const char* fp = knob("TGX_PATH");  // (rows4 names the kernels over the 16-byte records, here as for encode)
        if (!(ff && strcmp(ff, "rows4") == 0) && !(fp && strcmp(fp, "rows4") == 0)) {
            // The tables cost ~80 ns of host time per token of the vocabulary, the kernel saves ~4.7 ms per GiB of text:
            // a model that runs ONE pass over a small shard (prune makes a model per EM sub-iteration, src/prune.rs:48)
            // is better off without them; a model's second pass, or a pass over enough text, builds them.
            if (!m->estep_trie8_tried && (m->estep_calls >= 1 || ff != nullptr || (double)N * 4.7e-12 >= (double)m->vocab_size * 80e-9)) {
                const tgx_status est = ensure_estep_trie8(m);
                if (est != TGX_OK) return est;
            }
            use5f = m->have_wvalues;
        }
    }
    if (use5f) {
        const uint32_t budget = 160u * 1024u;
        auto fits = [&](int waves, int ppl) { return m->n_values <= tgx::encode5_max_hot(false, waves, ppl, budget); };
        if (fits(13, 4)) {
            ppl5f = 4;
            waves5f = 16;
            while (!fits(waves5f, 4)) waves5f--;
        } else if (fits(13, 3)) {
            ppl5f = 3;
            waves5f = 13;
        } else if (fits(16, 2)) {
            ppl5f = 2;
            waves5f = 16;
        } else {
            ppl5f = 3;
            waves5f = 16;
        }
        knob_int("TGX_EPPL", 1, 4, &ppl5f);
        uint32_t n_hot = knob_cap_hot("TGX_E5_HOT", std::min(m->n_values, tgx::encode5_max_hot(false, waves5f, ppl5f, budget)));
        cold5f = n_hot < m->n_values;
        int per_simd = 0;
        if (tgx::estep5_waves_per_simd(dropout > 0.0, cold5f, ppl5f, &per_simd) != hipSuccess) return fail(TGX_ERR_DEVICE, "estep5 attribute query failed");
        waves5f = std::max(1, std::min(waves5f, per_simd * 4));
        const uint64_t n_units = pieces ? pc.n : K;
        waves5f = waves_for_units(waves5f, n_units, (uint64_t)m->num_cus);
        n_hot = knob_cap_hot("TGX_E5_HOT", std::min(m->n_values, tgx::encode5_max_hot(false, waves5f, ppl5f, budget)));  // (fewer waves: more room)
        cold5f = n_hot < m->n_values;
        q5f.trie8 = m->d_trie8;
        q5f.trie_bytes = (uint32_t)(m->flat.table.size() * sizeof(tgx::Trie8Rec));
        q5f.values = m->d_wvalues;
        q5f.root_base = m->root_base8;
        q5f.n_values = m->n_values;
        q5f.n_hot = n_hot;
        q5f.claim_chunk = claim_chunk_for(N, n_units);
        const uint64_t rows_per_block = 4ull * (uint64_t)waves5f;
        blocks5f = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_units + rows_per_block - 1) / rows_per_block, (uint64_t)m->num_cus));
    }
    bool use_linear = linear;
    for (;;) {
        p.trie_fwd = use_linear ? m->d_trie_w : m->d_trie;
        p.trie_rev = use_linear ? m->d_trie_rev_w : m->d_trie_rev;
        const bool on_pieces = pieces && use_linear;  // (the log-domain kernels redo a pass on the uncut snippets: cuts.hip)
        p.soffs = on_pieces ? pc.d_offs : d_soffs;
        p.order = on_pieces ? pc.d_order : d_order;
        p.n_snips = on_pieces ? pc.n : K;
        p.snip_sample = on_pieces ? pc.d_sample : d_ssample;
        p.snip_base = on_pieces ? pc.d_base : d_sbase;
        p.err_snip = on_pieces ? &m->d_ctrl->err_piece : &m->d_ctrl->err;  // pieces: z is checked per snippet (launch_piece_z_check)
        if (hipMemsetAsync(&m->d_ctrl->estep, 0x00, sizeof(DeviceCtrl::Estep), m->stream) != hipSuccess ||
            hipMemsetAsync(d_z, 0, 256, m->stream) != hipSuccess ||
            hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step queue reset failed");
        const bool fwd5 = use_linear && use5f;
        time_begin(m, fwd5 ? "estep5_fwd_kernel" : (use_linear ? "estep4l_fwd_kernel" : "estep4_fwd_kernel"));
        if ((fwd5 ? tgx::launch_estep5_fwd(p, q5f, cold5f, ppl5f, waves5f, blocks5f, m->stream)
                  : (use_linear ? tgx::launch_estep4l_fwd(p, eppl_fwd, long_tokens, (uint32_t)m->num_cus, m->stream)
                                : tgx::launch_estep4_fwd(p, (uint32_t)m->num_cus, m->stream))) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step forward launch failed");
        time_end(m);
        if (use_linear) {
            unsigned long long flag = 0;
            if (hipMemcpyAsync(&flag, &m->d_ctrl->estep.range_flag, 8, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
                hipStreamSynchronize(m->stream) != hipSuccess)
                return fail(TGX_ERR_DEVICE, "E-step forward pass failed: %s", hipGetErrorString(hipGetLastError()));
            if (flag != 0) {
                if (long_tokens) {
                    if (fallback) *fallback = true;
                    return pass.done();
                }
                use_linear = false;
                continue;
            }
        }
        time_begin(m, use_linear ? "estep4l_bwd_kernel" : "estep4_bwd_kernel");
        uint32_t bwd_groups = 16;  // groups of 16 positions per block of the backward kernel (estep4l.hip)
        if (const char* e = knob("TGX_BWD_GROUPS")) bwd_groups = (uint32_t)std::max(0, atoi(e));
        if ((use_linear ? tgx::launch_estep4l_bwd(p, eppl_bwd, long_tokens, (uint32_t)m->num_cus, bwd_groups, m->stream)
                        : tgx::launch_estep4_bwd(p, (uint32_t)m->num_cus, m->stream)) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "estep4 backward launch failed");
        time_end(m);
        if (on_pieces && tgx::launch_piece_z_check(d_zarr, pc.d_snip, pc.n, pc.d_zsnip, K, &m->d_ctrl->err, m->stream) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "E-step z check launch failed");
        break;
    }
    double* d_sum = d_exp + (size_t)n_rep * n_rev;  // replica sums
    time_begin(m, "estep4_reduce_kernel");
    if (tgx::launch_estep4_reduce(d_exp, d_sum, (uint32_t)n_rev, n_rep, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "estep4 reduce launch failed");
    time_end(m);
    std::vector<double> h(n_rev);
    double hz = 0.0;
    // The backward kernel of the long-token builds has an overflow list of its own (matches of 17..32 bytes by END
    // position and window; the forward kernel counts them by START position), so it can run out where the forward
    // kernel did not: the flag is read again with the results, and a pass that raised it is discarded.
    unsigned long long flag_bwd = 0;
    tgx_status st = estep_read_back(m, c, d_sum, &h, d_z, &hz, &flag_bwd);
    if (st != TGX_OK) return st;
    if (use_linear && flag_bwd != 0) {  // nothing of this pass reaches `expected`
        if (long_tokens && fallback) {
            *fallback = true;  // the generic kernel redoes it (tgx_estep)
            return pass.done();
        }
        return fail(TGX_ERR_DEVICE, "E-step backward kernel raised range_flag %llu after a clean forward pass", flag_bwd);
    }
    st = estep_z_failure(m, c, ssample.data());
    if (st != TGX_OK) return st;
    add_slot_counts(m, h, expected);
    if (logz_sum) *logz_sum = hz;
    m->estep_calls++;
    return pass.done();
}

// E-step on estep_kernel (estep.hip): the log-domain kernel, one sample per wave, for what the others cannot do (tokens
// of more than 32 bytes, a score that is not finite, a pass the linear-domain kernels handed back, TGX_PATH=fused).
// Caller holds both locks and has built the reversed trie.
static tgx_status estep_generic(tgx_model* m, tgx_corpus* c, uint64_t snippet_len, double dropout, uint64_t seed, double* expected,
                                double* logz_sum) {
    const uint64_t S = c->n_samples, N = c->n_bytes;
    const size_t n_rev = m->flat_rev.table.size();
    uint32_t n_rep = 256;
    while (n_rep > 1 && (size_t)n_rep * n_rev * 8 > (512ull << 20)) n_rep >>= 1;
    const size_t abytes = (size_t)(N + S + 128) * 8, ebytes = (size_t)(n_rep + 1) * n_rev * 8 + 256;
    Pass pass(m);
    double *d_alpha = nullptr, *d_exp = nullptr, *d_z = nullptr;
    if (pass.alloc(abytes, &d_alpha) != hipSuccess || pass.alloc(ebytes, &d_exp) != hipSuccess || pass.alloc(256, &d_z) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "out of device memory (E-step scratch)");
    if (hipMemsetAsync(d_exp, 0, ebytes, m->stream) != hipSuccess ||
        hipMemsetAsync(d_z, 0, 256, m->stream) != hipSuccess ||
        hipMemsetAsync(&m->d_ctrl->err, 0xFF, 8, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "memset failed");
    tgx::EstepParams p{};
    p.text = c->d_text;
    p.offs = c->d_offs;
    p.order = c->d_order;
    p.n_samples = S;
    p.trie_fwd = m->d_trie;
    p.trie_rev = m->d_trie_rev;
    p.root_fwd = m->flat.table[0].base & ~tgx::kTerminalBit;
    p.root_rev = m->flat_rev.table[0].base & ~tgx::kTerminalBit;
    p.lm = m->lm;
    p.snippet_len = snippet_len;
    p.alpha = d_alpha;
    p.expected_slot = d_exp;
    p.n_slots_rev = (uint32_t)n_rev;
    p.n_replicas = n_rep;
    p.logz_sum = d_z;
    p.err_sample = &m->d_ctrl->err;
    p.dropout = dropout;
    p.seed = seed;
    const uint64_t wpb = tgx::estep_waves_per_block(m->lm);
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>((S + wpb - 1) / wpb, (uint64_t)m->num_cus * (uint64_t)m->estep_blocks_per_cu));
    time_begin(m, "estep_kernel");
    if (tgx::launch_estep(p, blocks, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "estep launch failed");
    time_end(m);
    double* d_sum = d_exp + (size_t)n_rep * n_rev;
    if (tgx::launch_estep4_reduce(d_exp, d_sum, (uint32_t)n_rev, n_rep, m->stream) != hipSuccess)
        return fail(TGX_ERR_DEVICE, "estep reduce launch failed");
    std::vector<double> h(n_rev);
    double hz = 0.0;
    tgx_status st = estep_read_back(m, c, d_sum, &h, d_z, &hz, nullptr);
    if (st == TGX_OK) st = estep_z_failure(m, c, nullptr);  // (this kernel's units are the samples)
    if (st != TGX_OK) return st;
    add_slot_counts(m, h, expected);
    if (logz_sum) *logz_sum = hz;
    return pass.done();
}

tgx_status tgx_estep(tgx_model* m, tgx_corpus* c, uint64_t snippet_len, double dropout,
                     uint64_t seed, double* expected, double* logz_sum) {
    if (!m || !c || !expected) return fail(TGX_ERR_INVALID, "tgx_estep: NULL argument");
    if (m->device != c->device) return fail(TGX_ERR_INVALID, "model and corpus on different devices");
    if (snippet_len == 0) snippet_len = TGX_ESTEP_SNIPPET_LEN;
    if (snippet_len >= 0xFFFFFF00ull) return fail(TGX_ERR_UNSUPPORTED, "snippet_len must be below 4 GiB");
    std::lock_guard<std::mutex> lk(m->mu);
    std::lock_guard<std::mutex> lkc(c->mu);
    HIP_TRY(hipSetDevice(m->device));
    m->n_timed = 0;
    tgx_status st = TGX_OK;
    {   // round 4: one walk per position (estep7.hip); TGX_ESTEP=chain / log and TGX_PATH=rows4 / fused keep the older kernels
        const char* force = knob("TGX_PATH");
        const char* fe = knob("TGX_ESTEP");
        if (m->scores_finite && m->lm <= 16 && m->vocab_size && !force && !fe) {
            bool fallback = false;
            st = estep_fused(m, c, snippet_len, dropout, seed, expected, logz_sum, &fallback);
            if (st != TGX_OK || !fallback) return st;
            m->n_timed = 0;
        }
    }
    st = ensure_reverse_trie(m);
    if (st != TGX_OK) return st;
    {
        const char* force = knob("TGX_PATH");
        const bool rows = m->scores_finite && !(force && strcmp(force, "fused") == 0);
        if (rows && m->lm <= 16) return estep_rows4(m, c, snippet_len, dropout, seed, expected, logz_sum, nullptr);
        // tokens of 17..32 bytes (after `merge`): the linear-domain kernels' long-token builds; the generic kernel
        // below where they cannot do the pass
        const char* force_log = knob("TGX_ESTEP");
        if (rows && m->lm <= 32 && m->estep_linear_ok && !(force_log && strcmp(force_log, "log") == 0)) {
            bool fallback = false;
            st = estep_rows4(m, c, snippet_len, dropout, seed, expected, logz_sum, &fallback);
            if (st != TGX_OK || !fallback) return st;
        }
    }
    return estep_generic(m, c, snippet_len, dropout, seed, expected, logz_sum);
}
