// The C ABI's encode pass (include/tgx.h: tgx_encode_corpus, tgx_encode_batch*): the tables a model builds at its first
// encode, the choice among the four kernel families — encode5_kernel / encode6_kernel (encode5.hip), encode4_kernel
// (kernels.hip), encode4l_kernel / encode2_kernel (encode4l.hip, encode2.hip) and the one-sample-per-wave kernel
// (kernels.hip) —, their geometry, the back-trace, and the scan and compaction that end a pass.  It runs on the model's own
// streams under a Pass and takes the knobs and the launch arithmetic from tgx_api.cpp (pass_internal.h); the lattice
// passes (lattice_pass.cpp) and the counting passes (tgx_api.cpp) take the encode parameters, the tables and the end of a
// pass from here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tgx.h"
#include "api_internal.h"
#include "device_internal.h"
#include "pass_internal.h"
#include "kernels.h"
#include "encode_split.h"
#include "ids_in_place.h"
#include "top_table.h"
#include "trie_build.h"

using namespace tgx::host;
using namespace tgx::dev;

namespace {

// encode5_kernel: the depth at which a trip's live walks are compacted (0: never; TGX_E5_COMPACT=off|4..8 overrides)
constexpr int kE5CompactDepth = 5;

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
         tgx::launch_rank_remap(m->d_trie8, (uint32_t)m->flat.table.size(), d_perm, tgx::kTrie8RankMask, m->stream) == hipSuccess &&
         (!m->d_top8 || tgx::launch_rank_remap_top(m->d_top8, d_perm, m->stream) == hipSuccess) &&  // (ranks in both halves of its second words)
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

// Long samples first, four to a block (encode6_kernel: three walker waves per sample ahead of one row of the
// block's relaxing wave), when that shortens the pass.  encode5_kernel takes ~0.104 us per byte of a
// sample's serial chain (6.8 ms per 64 KiB) and ~1 s per 88 GB of batch; encode6_kernel ~0.037 us per byte
// of chain (2.4 ms per 64 KiB) but ~55 GB/s once every CU has its two blocks (eight relaxing rows per CU;
// profiles/r02: e6 shapes).  The two run one after the other, so the split is chosen among the powers of
// two as thresholds by the sum of the two estimates; TGX_LONG_THRESHOLD forces one (0: never).
// Its LDS copy of the value table is what two blocks per CU leave room for (~4 500 values).
struct Encode6Choice {
    int e6_bpc;        // blocks per CU
    uint32_t n_hot6;   // values in the LDS copy
    uint32_t pool6;    // pool entries per ring slot (0: none)
    bool cold6;        // the LDS copy does not hold every value
    bool e6_usable;    // false: the kernel has no build that beats encode5_kernel on this vocabulary
};
Encode6Choice choose_encode6(const tgx_model* m) {
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
    return Encode6Choice{e6_bpc, n_hot6, pool6, cold6, e6_usable};
}

// The samples that go to encode6_kernel and the CUs it gets beside encode5_kernel: the cost model of encode_split.h over
// the batch's lengths, with the knobs parsed here.
tgx::EncodeSplit split_long_samples(const tgx_model* m, const tgx_corpus* c, const Encode6Choice& e6) {
    tgx::EncodeSplitQuery sq{};
    sq.sorted_len = c->h_sorted_len.data();
    sq.sorted_cum = c->h_sorted_cum.data();
    sq.n_samples = c->n_samples;
    sq.n_bytes = c->n_bytes;
    sq.max_len = c->max_len;
    sq.num_cus = m->num_cus;
    sq.cold6 = e6.cold6;
    sq.e6_bpc = e6.e6_bpc;
    sq.values_fit = m->n_values <= tgx::encode5_max_hot(false, 8, 4, 160u * 1024u);
    sq.corun_timeouts = m->corun_wait_timeouts != 0;
    if (const char* e = knob("TGX_LONG_THRESHOLD")) {
        sq.threshold_set = true;
        sq.threshold = (uint64_t)std::max(0ll, atoll(e));
    }
    if (const char* e = knob("TGX_CORUN")) {
        sq.corun_set = true;
        sq.corun = atoi(e);
    }
    return tgx::encode_split(sq);
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
//   * the same with 14 waves in the TOP builds, whose LDS holds no copy of the root's records: up to 9 727 values — the
//     32 000-entry vocabulary's 9 652 —, encode5_kernel 12.1 -> 11.5 ms (profiles/top_table);
//   * three positions per lane with the ~7 800 hottest values in LDS and the others read from L2 by the
//     relaxing lanes (COLD builds; every token its own score: after an M-step or merge), 14.0 ms.
// Fewer waves when the batch has fewer samples than the chip has rows, so that they spread over the CUs.
// Tokens of 17..32 bytes: the LONG build (four positions per lane, a list of long matches per wave).
struct Encode5Geometry {
    int ppl, bpc, waves;  // positions per lane, blocks per CU, waves per block
    int per_simd;         // waves per SIMD that the chosen build's registers allow
    bool cold;            // the LDS copy does not hold every value
    uint32_t n_hot;       // values in the LDS copy
    uint32_t blocks5;
    int compact;          // the build's switches: the depth at which live walks are compacted,
    bool lean, step_ok;   // the lean builds, and with the lean step
    bool in_place;        // the build counts tokens and the trace writes the ids in place (ids_in_place.h)
    bool top;             // the TOP build: a walk's first two levels from the top table, no root copy in LDS
};
// Three positions per lane with every value in LDS runs 14 waves where the values fit beside them without the root copy
// (9 727 at most: the 32 000-entry spec vocabulary has 9 652), else 13 as before: by measurement (profiles/top_table).
constexpr bool kE5Top14Waves = true;
// p: the pass's parameters so far (dropout, flags); n_long, corun_cus: the split; have_result: there is a result to write ids into
tgx_status choose_encode5(const tgx_model* m, const tgx_corpus* c, const tgx::EncodeParams& p, bool long_tokens, uint64_t n_long,
                          uint32_t corun_cus, bool have_result, Encode5Geometry* out) {
    const double dropout = p.dropout;
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
    // the TOP builds (encode5.hip) and their LDS layout without the root copy; TGX_E5_TOP=0: the kernels and the geometry as they were
    bool top = tgx::encode5_has_top(dropout > 0.0, long_tokens) && m->d_top8 != nullptr;
    if (const char* e = knob("TGX_E5_TOP")) top = top && atoi(e) != 0;
    const uint32_t lds_cu = 160u * 1024u;
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
    const bool want_count = have_result && tgx::ids_in_place(iq);
    {
        int ps4 = 0;
        HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, false, 4, long_tokens, compact, lean, step_ok, want_count, top, &ps4));
        hot_waves = std::min(16, ps4 * 4);
        const int least = long_tokens ? 12 : 13;  // (the long-token build has four positions per lane only)
        while (hot_waves >= least && m->n_values > tgx::encode5_max_hot(long_tokens, hot_waves, 4, lds_cu, top)) hot_waves--;
        if (hot_waves < least) {
            hot_waves = 0;  // not with four positions per lane
            if (!long_tokens) {
                // three positions per lane x 13 waves with every value in LDS (up to ~10 100: the 32 000-entry spec
                // vocabulary, 12.5 ms against 12.8 with two positions per lane); two x 16 (up to ~11 900: the
                // 65 536-entry one, 13.0 ms); else three x 16 with the ~7 800 hottest in LDS (every token its own
                // score: 14.0 ms against 14.4 with four positions per lane and 3 712) — profiles/r03/n_e5_ppl3_sweep.txt
                // (TOP: the root copy's 2 KiB are what a fourteenth wave lacked: encode5_kernel 12.00 -> 11.56 ms, profiles/top_table)
                if (top && kE5Top14Waves && m->n_values <= tgx::encode5_max_hot(false, 14, 3, lds_cu, top)) {
                    ppl = 3;
                    hot_waves = 14;
                } else if (m->n_values <= tgx::encode5_max_hot(false, 13, 3, lds_cu, top)) {
                    ppl = 3;
                    hot_waves = 13;
                } else if (m->n_values <= tgx::encode5_max_hot(false, 16, 2, lds_cu, top)) {
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
    HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, false, ppl, long_tokens, compact, lean, step_ok, want_count, top, &per_simd));
    int waves = std::min(16, (per_simd / bpc) * 4);
    if ((ppl == 4 || ppl == 3) && bpc == 1 && hot_waves > 0) waves = std::min(waves, hot_waves);
    if (m->n_values > tgx::encode5_max_hot(long_tokens, waves, ppl, budget, top)) {
        cold = true;
        HIP_TRY(tgx::encode5_waves_per_simd(dropout > 0.0, true, ppl, long_tokens, compact, lean, step_ok, want_count, top, &per_simd));
        waves = std::min(16, (per_simd / bpc) * 4);
    }
    if (balance_waves > 0 && ppl == 4 && bpc == 1) waves = std::min(waves, balance_waves);
    waves = waves_for_units(waves, rest_n, (uint64_t)cus5 * bpc);
    knob_int("TGX_WAVES", 1, 16, &waves);
    while (waves > 1 && tgx::encode5_max_hot(long_tokens, waves, ppl, budget, top) < 16u) waves--;
    uint32_t n_hot = std::min(m->n_values, tgx::encode5_max_hot(long_tokens, waves, ppl, budget, top));
    n_hot = knob_cap_hot("TGX_E5_HOT", n_hot);
    cold = n_hot < m->n_values;
    iq.build_counts = tgx::encode5_counts(dropout > 0.0, cold, ppl, long_tokens);
    const bool in_place = want_count && tgx::ids_in_place(iq);
    const uint64_t rows_per_block = 4 * (uint64_t)waves;
    const uint32_t blocks5 = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>((rest_n + rows_per_block - 1) / rows_per_block, (uint64_t)cus5 * bpc));
    *out = Encode5Geometry{ppl, bpc, waves, per_simd, cold, n_hot, blocks5, compact, lean, step_ok, in_place, top};
    return TGX_OK;
}

// The trace of the rows5 path over every sample of the corpus (p.order and p.n_samples are the whole batch's again).
tgx_status trace_rows5(tgx_model* m, tgx_corpus* c, tgx::EncodeParams& p, bool long_tokens, bool in_place, Pass& pass, tgx_result* r) {
    const uint32_t blocks_t = trace_blocks(m, c->n_samples);
    if (in_place) {
        // the counts are there before the trace: offsets, total (the pass's one wait), the ids buffer, and the trace
        // writes every id where it belongs.  d_ctrl->err is the caller's to read, after the trace.
        const tgx_status st = scan_ids_offsets(m, c, r, "encode", false);
        if (st != TGX_OK) return st;
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
    return TGX_OK;
}

// The rows5 path: encode6_kernel over the long samples (first, or beside encode5_kernel on CUs of its own),
// encode5_kernel over the rest, then the trace over all of them — through `tmp`, or writing r's ids in place.
tgx_status encode_rows5(tgx_model* m, tgx_corpus* c, tgx::EncodeParams& p, bool long_tokens, Pass& pass, tgx_result* r) {
    tgx_status st = ensure_value_ranks(m, c);
    if (st != TGX_OK) return st;
    m->last_redo_samples = 0;
    const Encode6Choice e6 = choose_encode6(m);
    tgx::EncodeSplit split;
    if (c->n_samples && !long_tokens && e6.e6_usable) split = split_long_samples(m, c, e6);  // (encode6_kernel walks 16 bytes)
    const uint64_t n_long = split.n_long;
    const uint32_t corun_cus = split.corun_cus;
    Encode5Geometry g;
    if ((st = choose_encode5(m, c, p, long_tokens, n_long, corun_cus, r != nullptr, &g)) != TGX_OK) return st;
    m->last_n_hot = g.n_hot;
    m->last_encode_top = g.top && c->n_samples - n_long != 0;  // (self-check: what tgx_last_encode_top_table reports)
    if (!g.in_place) {  // the trace writes through `tmp`
        if ((st = ensure_scratch(c, true)) != TGX_OK) return st;
        p.tmp = c->d_tmp;
    }
    // (self-check) the lean items of this pass's kernels: encode5_kernel's in the low byte, encode6_kernel's in the next
    const uint64_t rest_n = c->n_samples - n_long;  // what is left for encode5_kernel
    m->last_lean_items = !g.lean ? 0u : ((rest_n ? (uint32_t)tgx::encode5_lean_items(g.cold, g.ppl, g.step_ok) : 0u) |
                                         (n_long ? (uint32_t)tgx::encode6_lean_items() << 8 : 0u));
    // whole blocks only: a block's waves are dealt round-robin to the SIMDs, ceil(waves / 4) on the fullest
    m->last_encode_waves_per_cu = std::min(g.bpc, g.per_simd / ((g.waves + 3) / 4)) * g.waves;
    tgx::Encode5Params q{};
    q.trie8 = m->d_trie8;
    q.trie_bytes = (uint32_t)(m->flat.table.size() * sizeof(tgx::Trie8Rec));
    q.values = m->d_values;
    q.root_base = m->root_base8;
    q.top = m->d_top8;
    q.n_values = m->n_values;
    q.n_hot = g.n_hot;
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
        blocks6 = (uint32_t)std::min<uint64_t>((n_long + 3) / 4, (uint64_t)(corun_cus ? (int)corun_cus : m->num_cus) * (uint64_t)e6.e6_bpc);
        q6.n_hot = e6.n_hot6;
        q6.pool = e6.cold6 ? e6.pool6 : 0u;
        if (!corun_cus) {
            time_begin(m, "encode6_kernel");
            HIP_TRY(tgx::launch_encode6(p6, q6, e6.cold6, g.lean, blocks6, m->stream));
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
    const Stamps stamps5 = stamps_begin(m, pass, '1', (size_t)g.blocks5 * (size_t)g.waves);
    p.stamps = stamps5.d;
    time_begin(m, "encode5_kernel");
    {
        if (long_tokens) {  // samples whose wave ran out of list entries for long matches go to encode2_kernel
            p.redo_count = &m->d_ctrl->encode_redo;
            p.redo_list = c->d_counts;  // free until the trace writes the token counts
            HIP_TRY(hipMemsetAsync(&m->d_ctrl->encode_redo, 0x00, 8, m->stream));
        }
        // (co-run: more than half of the CU's LDS, so that no block of the long-sample kernel shares the CU)
        const hipError_t le = tgx::launch_encode5(p, q, g.cold, g.ppl, long_tokens, g.compact, g.lean, g.step_ok, g.in_place, g.top, g.waves, g.blocks5, corun_cus && n_long ? 84u * 1024u : 0u, m->stream);
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
            while (*started < g.blocks5 && !(timed_out = std::chrono::steady_clock::now() - t0 >= std::chrono::milliseconds(2))) {
            }
            if (timed_out && *started < g.blocks5) m->corun_wait_timeouts++;
        }
        const hipError_t l6 = tgx::launch_encode6(p6, q6, e6.cold6, g.lean, blocks6, m->stream2);
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
    if (stamps5.d) stamps_report(m, stamps5, g.ppl, "encode5 stamps", "iteration", {"switch", "text+reset", "walk", "relax", "store"});
    p.stamps = nullptr;
    if (long_tokens) {
        const tgx_status rst = redo_long_matches(m, c, p);
        if (rst != TGX_OK) return rst;
    }
    p.order = c->d_order;
    p.n_samples = c->n_samples;
    return trace_rows5(m, c, p, long_tokens, g.in_place, pass, r);
}

// Vocabularies without 8-byte records (more than 65 535 distinct score values): round 1's kernel over the
// 16-byte records, scores through the match buffer.
// `bpc` blocks per CU of `waves` waves each (8 KiB of LDS per wave and position group).
// TGX_PPL (positions per lane: 1, 2, 4), TGX_WAVES, TGX_BPC override the defaults (with TGX_DEBUG=1).
// Two blocks of ten waves per CU (20 x 8 KiB of LDS); rows claim samples dynamically, so the
// geometry only has to fill the CU.
tgx_status encode_rows4(tgx_model* m, tgx_corpus* c, tgx::EncodeParams& p, Pass& pass) {
    const double dropout = p.dropout;
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
    return TGX_OK;
}

// Tokens of 17..32 bytes: the 16-lane rows with an overflow list for the long matches (encode4l.hip);
// samples whose wave ran out of overflow entries are redone two per wave on 32-lane rows (encode2.hip),
// as is the whole batch with TGX_PATH=rows2.
tgx_status encode_rows2(tgx_model* m, tgx_corpus* c, tgx::EncodeParams& p, bool rows2) {
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
    return TGX_OK;
}

// Everything else (tokens of more than 32 bytes, scores that are not finite, TGX_PATH=fused): one sample per wave.
tgx_status encode_fused(tgx_model* m, tgx_corpus* c, const tgx::EncodeParams& p) {
    time_begin(m, "encode_kernel");
    HIP_TRY(tgx::launch_encode(p, grid_blocks(m, c->n_samples), m->stream));
    time_end(m);
    return TGX_OK;
}

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
    m->last_encode_top = false;
    if (use5) return encode_rows5(m, c, p, long_tokens, pass, r);
    if ((st = ensure_scratch(c, true)) != TGX_OK) return st;
    p.tmp = c->d_tmp;
    if (use4) return encode_rows4(m, c, p, pass);
    if (use2) return encode_rows2(m, c, p, force && strcmp(force, "rows2") == 0);
    return encode_fused(m, c, p);
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
        const tgx_status tst = upload_top_table(m, t8.rec.data(), ns, t8.root_base);
        if (tst != TGX_OK) return tst;
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

tgx_status tgx::dev::upload_top_table(tgx_model* m, const tgx::Trie8Rec* rec, size_t n_slots, uint32_t root_base) {
    std::vector<tgx::Trie8Rec> top;
    tgx::build_top_table(rec, n_slots, root_base, &top);
    if (!m->d_top8) HIP_TRY(hipMalloc(&m->d_top8, top.size() * sizeof(tgx::Trie8Rec)));
    HIP_TRY(hipMemcpy(m->d_top8, top.data(), top.size() * sizeof(tgx::Trie8Rec), hipMemcpyHostToDevice));
    return TGX_OK;
}

// ---- encode --------------------------------------------------------------------

// caller holds m->mu
tgx_status tgx::dev::encode_corpus_locked(tgx_model* m, tgx_corpus* c, double dropout, uint64_t seed,
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

// ---- measurement: what the last encode pass of a model chose --------------------------------

uint32_t tgx_last_encode_waves_per_cu(const tgx_model* m) { return m ? (uint32_t)m->last_encode_waves_per_cu : 0u; }
uint64_t tgx_last_encode_redo_samples(const tgx_model* m) { return m ? m->last_redo_samples : 0; }
uint64_t tgx_last_encode_long_samples(const tgx_model* m) { return m ? m->last_long_samples : 0; }
uint32_t tgx_last_encode_corun_cus(const tgx_model* m) { return m ? m->last_corun_cus : 0; }
uint32_t tgx_encode_corun_timeouts(const tgx_model* m) { return m ? m->corun_wait_timeouts : 0; }
uint32_t tgx_last_encode_hot_values(const tgx_model* m) { return m ? m->last_n_hot : 0u; }
int tgx_last_encode_top_table(const tgx_model* m) { return m && m->last_encode_top ? 1 : 0; }
uint32_t tgx_last_encode_lean_items(const tgx_model* m) { return m ? m->last_lean_items : 0u; }
int tgx_last_encode_ids_in_place(const tgx_model* m) { return (m && m->last_ids_in_place) ? 1 : 0; }
