// Device side of `generate` (reference src/generate.rs:54-139, VocabularyGenerator::feed): the DOCUMENT
// frequency of every char-aligned substring of at most max_token_length bytes — in how many samples it occurs
// at least once — over a packed batch.  The reference enumerates the windows per sample on rayon workers into
// a HashSet<&str> and merges per-chunk maps; here
//
//   window kernels : one lane per byte position; a position that starts a character extends a window
//                    character by character, hashing as it goes (FNV-1a 64), and keeps a window with the
//                    seeded insert-probability rule (the reference draws from an unseeded thread RNG,
//                    src/generate.rs:88,112: a counter hash of (seed, sample, window hash) stands in, the same
//                    in the Python mirror).  Pass 1 counts the kept windows per block of 256 positions, an
//                    exclusive scan gives every block its output range, pass 2 writes {hash, sample | position
//                    | length} in position order — hence in ascending sample order.
//   sort           : rocPRIM radix sort of the pairs by hash (stable: samples stay ascending inside a hash run).
//   runs           : a run of equal hashes is one substring; its document frequency is the number of distinct
//                    samples in the run (adjacent duplicates after the stable sort).  Run heads are numbered by
//                    an inclusive scan; every entry compares its window's BYTES with its run's first entry,
//                    so a 64-bit hash collision is detected, never silently merged.
//
// What stays on the host, as in the reference: the split regex (parts arrive as byte ranges), the allow regex
// (a pure function of the candidate: applied to the distinct substrings that come back instead of to every
// window) and the added / suggested tokens.  HBM-bound byte and integer work; no MFMA.
//
// The allow regex as an automaton is served by window kernels of their own (allow.hip, include/tgx_allow.h): the
// checks, the uploads, the scan and everything from the sort on are the functions of generate.h, defined below, which
// both paths call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/tgx.h"
#include "device_internal.h"
#include "generate.h"

tgx_status tgx_set_error(tgx_status st, const char* msg);  // tgx_api.cpp

namespace tgx {

struct WindowParams {
    const uint8_t* text;          // padded: reads up to 32 bytes past a position are safe
    uint64_t n_bytes;
    const uint64_t* part_begin;   // parts (samples, or the split regex's matches) sorted, disjoint
    const uint64_t* part_end;
    const uint32_t* part_sample;
    const uint64_t* part_origin;  // offset in `text` of the first byte of the part's SAMPLE (the keep rule hashes the window's offset in its sample)
    uint64_t n_parts;
    const uint32_t* blk_part;     // per block of 256 positions: first part whose end lies beyond the block's start
    uint32_t max_len;
    double prob;
    uint64_t seed;
    uint64_t salt;                // 0: the sort key is the window's FNV-1a hash; else a second, salted hash of its bytes (the retry
                                  // after two different substrings met in one key)
    uint64_t key_mask;            // ~0; fewer bits only in the forced-collision test
    uint32_t* blk_count;          // pass 1: kept windows per block
    const uint64_t* blk_offs;     // pass 2: exclusive scan of blk_count
    uint64_t* keys;               // pass 2: window hash
    uint64_t* vals;               // pass 2: sample << 37 | position << 5 | (length - 1)
};

template <bool EMIT>
__global__ __launch_bounds__(256) void window_kernel(WindowParams P) {
    __shared__ uint32_t wave_cnt[4];
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t sample = 0;
    uint64_t origin = 0;
    uint64_t end = 0;  // end of this position's part; 0 = the position starts no window
    if (p < P.n_bytes) {
        uint64_t k = P.blk_part[blockIdx.x];
        while (k < P.n_parts && P.part_end[k] <= p) k++;
        if (k < P.n_parts && P.part_begin[k] <= p && (P.text[p] & 0xC0u) != 0x80u) {  // inside a part, at a character start
            end = P.part_end[k];
            sample = P.part_sample[k];
            origin = P.part_origin[k];
        }
    }
    // the windows of this position in ascending length; `emit` is called for the kept ones (src/generate.rs:99-120)
    auto windows = [&](auto emit) {
        uint32_t kept = 0;
        uint64_t h = kFnvOffset, g = kFnvOffset ^ P.salt;
        for (uint32_t len = 1; len <= P.max_len && p + len <= end; ++len) {
            const uint64_t c = (uint64_t)P.text[p + len - 1];
            generate_hash_byte(c, P.salt, h, g);
            const bool boundary = (p + len == end) || (P.text[p + len] & 0xC0u) != 0x80u;
            if (boundary && generate_keep(P.prob, P.seed, sample, p - origin, len)) {
                emit(kept, (P.salt ? g : h) & P.key_mask, len);
                kept++;
            }
        }
        return kept;
    };
    const uint32_t kept = windows([](uint32_t, uint64_t, uint32_t) {});
    // block-level exclusive prefix of `kept` (position order)
    uint32_t incl = kept;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(incl, off);
        if ((int)lane >= off) incl += y;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wave_cnt[w];
    if (!EMIT) {
        if (threadIdx.x == 255) P.blk_count[blockIdx.x] = before + incl;
        return;
    }
    const uint64_t at = P.blk_offs[blockIdx.x] + before + (incl - kept);
    windows([&](uint32_t i, uint64_t h, uint32_t len) {
        P.keys[at + i] = h;
        P.vals[at + i] = generate_value(sample, p, len);
    });
}

// head[i] = 1 where a new hash run starts
__global__ __launch_bounds__(256) void run_heads_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = i ? i - 1 : 0;
    head[i] = ((i == 0) | (keys[i] != keys[j])) ? 1u : 0u;
}

// rep[run] = the run's first entry; df[run] += 1 for every entry that opens a new sample inside its run.
// A run id outside [1, n_runs] cannot come out of an inclusive scan of the heads; it is never used as an index,
// and it is COUNTED (bad_runs): the host fails the call with TGX_ERR_DEVICE instead of returning frequencies with
// entries missing.  (Round 2 met a wild atomic address in an earlier, short-circuit form of this kernel whose
// source was not kept; the reconstructions under profiles/r03/run_count_short_circuit.* do not show a compiler
// defect, so the cause of that fault is NOT established — hence the loud guard.)
__global__ __launch_bounds__(256) void run_count_kernel(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                        const uint32_t* __restrict__ run_id, uint64_t n, uint32_t n_runs,
                                                        uint64_t* __restrict__ rep, uint32_t* __restrict__ df,
                                                        unsigned long long* __restrict__ bad_runs) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = i ? i - 1 : 0;
    const uint64_t k = keys[i], kp = keys[j], v = vals[i], vp = vals[j];
    const uint32_t r = run_id[i] - 1u;
    const bool head = (i == 0) | (k != kp);
    const bool newdoc = head | ((v >> 37) != (vp >> 37));
    if (r >= n_runs) {
        atomicAdd(bad_runs, 1ull);
        return;
    }
    if (head) rep[r] = v;
    if (newdoc) atomicAdd(&df[r], 1u);
}

// every entry's window against its run's representative, byte by byte
__global__ __launch_bounds__(256) void run_check_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ vals,
                                                        const uint32_t* __restrict__ run_id, uint64_t n, uint32_t n_runs,
                                                        const uint64_t* __restrict__ rep, unsigned long long* __restrict__ collisions,
                                                        unsigned long long* __restrict__ bad_runs) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (run_id[i] - 1u >= n_runs) {
        atomicAdd(bad_runs, 1ull);
        return;
    }
    const uint64_t a = vals[i], b = rep[run_id[i] - 1u];
    if (a == b) return;
    const uint32_t la = (uint32_t)(a & 31u) + 1u, lb = (uint32_t)(b & 31u) + 1u;
    bool same = la == lb;
    const uint64_t pa = (a >> 5) & 0xFFFFFFFFull, pb = (b >> 5) & 0xFFFFFFFFull;
    for (uint32_t j = 0; same && j < la; ++j) same = text[pa + j] == text[pb + j];
    if (!same) atomicAdd(collisions, 1ull);
}

// ---- what every path of the pass shares (generate.h) ----------------------------------------------------------------------

void* GenerateScratch::alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
    owned.push_back(p);
    // (these buffers bypass the pool; TGX_POOL_FILL covers them all the same)
    if (tgx::dev::pool_fill(device, p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
    return p;
}

void GenerateScratch::release() {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
}

namespace {

tgx_status generate_fail(GenerateScratch& scratch, tgx_status st, const char* msg) {
    (void)hipDeviceSynchronize();
    scratch.release();
    return tgx_set_error(st, msg);
}

// (TGX_DEBUG as tgx_api.cpp reads it: set, not empty, not "0")
bool generate_debug() {
    const char* dbg_env = getenv("TGX_DEBUG");
    return dbg_env && *dbg_env && *dbg_env != '0';
}

// (expands where `scratch` and `dbg` are visible)
#define G_TRY(expr)                                                       \
    do {                                                                  \
        if (dbg) { fprintf(stderr, "[tgx] generate: %s\n", #expr); fflush(stderr); } \
        if ((expr) != hipSuccess) return generate_fail(scratch, TGX_ERR_DEVICE, "HIP error in tgx_substring_df: " #expr); \
        if (dbg && hipDeviceSynchronize() != hipSuccess) return generate_fail(scratch, TGX_ERR_DEVICE, "HIP error after " #expr); \
    } while (0)

}  // namespace

tgx_status substring_df_check(const GenerateArgs& a, bool* empty) {
    *empty = false;
    if (a.n_distinct) *a.n_distinct = 0;
    if (a.cutoff_df) *a.cutoff_df = 0;
    if (!a.out_pos || !a.out_len || !a.out_df || !a.n_out) return tgx_set_error(TGX_ERR_INVALID, "tgx_substring_df: NULL argument");
    *a.out_pos = nullptr;
    *a.out_len = nullptr;
    *a.out_df = nullptr;
    *a.n_out = 0;
    if (a.n_windows) *a.n_windows = 0;
    if (a.n_collisions) *a.n_collisions = 0;
    if (a.n_parts && (!a.text || !a.part_begin || !a.part_end || !a.part_sample)) return tgx_set_error(TGX_ERR_INVALID, "tgx_substring_df: NULL argument");
    if (const char* why = generate_check_sizes(a.n_bytes, a.max_token_length)) return tgx_set_error(TGX_ERR_UNSUPPORTED, why);
    if (a.n_parts == 0 || a.n_bytes == 0) {
        *empty = true;
        return TGX_OK;
    }
    if (const char* why = generate_check_parts(a.n_bytes, a.part_begin, a.part_end, a.part_sample, a.part_origin, a.n_parts)) return tgx_set_error(TGX_ERR_INVALID, why);
    return TGX_OK;
}

tgx_status substring_df_upload(const GenerateArgs& a, GenerateScratch& scratch, GenerateInput* in) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || a.device < 0 || a.device >= ndev) {
        (void)hipGetLastError();
        return tgx_set_error(TGX_ERR_DEVICE, "no usable HIP device (gfx950 required)");
    }
    scratch.device = a.device;
    const bool dbg = generate_debug();
    G_TRY(hipSetDevice(a.device));
    const uint64_t n_bytes = a.n_bytes, n_parts = a.n_parts, n_blocks = (n_bytes + kGenerateBlock - 1) / kGenerateBlock;
    // first part whose end lies beyond each block's start
    std::vector<uint32_t> blk_part(n_blocks);
    {
        uint64_t k = 0;
        for (uint64_t b = 0; b < n_blocks; b++) {
            while (k < n_parts && a.part_end[k] <= b * kGenerateBlock) k++;
            blk_part[b] = (uint32_t)std::min<uint64_t>(k, 0xFFFFFFFFull);
        }
    }
    uint8_t* d_text = (uint8_t*)scratch.alloc(n_bytes + 64);
    uint64_t* d_pb = (uint64_t*)scratch.alloc(n_parts * 8);
    uint64_t* d_pe = (uint64_t*)scratch.alloc(n_parts * 8);
    uint32_t* d_ps = (uint32_t*)scratch.alloc(n_parts * 4);
    uint32_t* d_bp = (uint32_t*)scratch.alloc(n_blocks * 4);
    unsigned long long* d_ctr = (unsigned long long*)scratch.alloc(64);
    if (!d_text || !d_pb || !d_pe || !d_ps || !d_bp || !d_ctr) return generate_fail(scratch, TGX_ERR_DEVICE, "out of device memory (generate)");
    G_TRY(hipMemset(d_text + n_bytes, 0, 64));
    G_TRY(hipMemcpy(d_text, a.text, n_bytes, hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(d_pb, a.part_begin, n_parts * 8, hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(d_pe, a.part_end, n_parts * 8, hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(d_ps, a.part_sample, n_parts * 4, hipMemcpyHostToDevice));
    uint64_t* d_po = (uint64_t*)scratch.alloc(n_parts * 8);
    if (!d_po) return generate_fail(scratch, TGX_ERR_DEVICE, "out of device memory (generate)");
    G_TRY(hipMemcpy(d_po, a.part_origin ? a.part_origin : a.part_begin, n_parts * 8, hipMemcpyHostToDevice));
    G_TRY(hipMemcpy(d_bp, blk_part.data(), n_blocks * 4, hipMemcpyHostToDevice));
    G_TRY(hipMemset(d_ctr, 0, 64));
    *in = GenerateInput{d_text, d_pb, d_pe, d_po, d_ps, d_bp, n_blocks, d_ctr};
    return TGX_OK;
}

// exclusive scan of the counts (u32 -> u64)
tgx_status substring_df_offsets(GenerateScratch& scratch, const uint32_t* d_count, uint64_t* d_offs, uint64_t n, uint64_t* total) {
    const bool dbg = generate_debug();
    uint32_t* d_bc = const_cast<uint32_t*>(d_count);
    uint64_t* d_bo = d_offs;
    {
        size_t tb = 0;
        G_TRY((rocprim::exclusive_scan(nullptr, tb, d_bc, d_bo, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>())));
        void* tmp = scratch.alloc(tb);
        if (!tmp) return generate_fail(scratch, TGX_ERR_DEVICE, "out of device memory (generate)");
        G_TRY((rocprim::exclusive_scan(tmp, tb, d_bc, d_bo, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>())));
    }
    uint64_t last_off = 0;
    uint32_t last_cnt = 0;
    G_TRY(hipMemcpy(&last_off, d_bo + (n - 1), 8, hipMemcpyDeviceToHost));
    G_TRY(hipMemcpy(&last_cnt, d_bc + (n - 1), 4, hipMemcpyDeviceToHost));
    *total = last_off + last_cnt;
    return TGX_OK;
}

tgx_status substring_df_tail(const GenerateArgs& a, GenerateScratch& scratch, const GenerateInput& in, uint64_t M, const GenerateEmit& emit, GenerateTimer* timer) {
    const bool dbg = generate_debug();
    const uint8_t* d_text = in.text;
    unsigned long long* d_ctr = in.ctr;
    const uint64_t top_k = a.top_k;
    auto fail = [&](tgx_status st, const char* msg) { return generate_fail(scratch, st, msg); };
    auto dalloc = [&](size_t bytes) { return scratch.alloc(bytes); };
    auto stage_begin = [&](int stage) {
        if (timer) timer->begin(stage);
    };
    auto stage_end = [&](int stage) {
        if (timer) timer->end(stage);
    };
    if (a.n_windows) *a.n_windows = M;
    if (M == 0) {
        scratch.release();
        return TGX_OK;
    }
    if (M >= (1ull << 32)) return fail(TGX_ERR_UNSUPPORTED, "tgx_substring_df: more than 2^32 windows in one call: feed smaller batches");
    uint64_t* d_keys = (uint64_t*)dalloc(M * 8);
    uint64_t* d_vals = (uint64_t*)dalloc(M * 8);
    uint64_t* d_keys2 = (uint64_t*)dalloc(M * 8);
    uint64_t* d_vals2 = (uint64_t*)dalloc(M * 8);
    if (!d_keys || !d_vals || !d_keys2 || !d_vals2) return fail(TGX_ERR_DEVICE, "out of device memory (generate: windows)");
    // forced-collision test (TGX_KNOBS=1 TGX_GENERATE_COLLIDE=bits): the first attempt keeps that many key bits only
    uint64_t first_mask = ~0ull;
    {
        const char* kn = getenv("TGX_KNOBS");
        const char* fc = (kn && *kn && *kn != '0') ? getenv("TGX_GENERATE_COLLIDE") : nullptr;
        if (fc && atoi(fc) > 0 && atoi(fc) < 64) first_mask = (1ull << atoi(fc)) - 1ull;
    }
    uint32_t* d_head = reinterpret_cast<uint32_t*>(d_keys);  // (the unsorted key buffer is free once the sort is done)
    uint32_t* d_run = reinterpret_cast<uint32_t*>(d_keys) + M;
    const uint32_t mblocks = (uint32_t)((M + 255) / 256);
    uint64_t* d_rep = d_vals;  // the unsorted values are free after the sort: n_runs <= M
    uint32_t* d_df = nullptr;
    uint32_t n_runs = 0;
    unsigned long long coll_total = 0, coll = 0;
    for (int attempt = 0; attempt < 4; attempt++) {  // (a timed call reports the stages of its last attempt)
        const uint64_t salt = attempt ? 0xD6E8FEB86659FD93ULL * (uint64_t)attempt : 0ull;
        const uint64_t key_mask = attempt ? ~0ull : first_mask;
        G_TRY(hipMemset(d_ctr, 0, 64));
        stage_begin(kGenStageEmit);
        G_TRY(emit(salt, key_mask, d_keys, d_vals));
        stage_end(kGenStageEmit);
        stage_begin(kGenStageSort);
        {
            size_t tb = 0;
            G_TRY(rocprim::radix_sort_pairs(nullptr, tb, d_keys, d_keys2, d_vals, d_vals2, (size_t)M));
            void* tmp = dalloc(tb);
            if (!tmp) return fail(TGX_ERR_DEVICE, "out of device memory (generate: sort)");
            G_TRY(rocprim::radix_sort_pairs(tmp, tb, d_keys, d_keys2, d_vals, d_vals2, (size_t)M));
        }
        stage_end(kGenStageSort);
        stage_begin(kGenStageRuns);
        // run ids: inclusive scan of the run heads
        hipLaunchKernelGGL(run_heads_kernel, dim3(mblocks), dim3(256), 0, 0, d_keys2, M, d_head);
        G_TRY(hipGetLastError());
        {
            size_t tb = 0;
            G_TRY((rocprim::inclusive_scan(nullptr, tb, d_head, d_run, (size_t)M, rocprim::plus<uint32_t>())));
            void* tmp = dalloc(tb);
            if (!tmp) return fail(TGX_ERR_DEVICE, "out of device memory (generate)");
            G_TRY((rocprim::inclusive_scan(tmp, tb, d_head, d_run, (size_t)M, rocprim::plus<uint32_t>())));
        }
        G_TRY(hipMemcpy(&n_runs, d_run + (M - 1), 4, hipMemcpyDeviceToHost));
        if (dbg) fprintf(stderr, "[tgx] generate: attempt %d M=%llu n_runs=%u\n", attempt, (unsigned long long)M, n_runs);
        if (n_runs == 0 || n_runs > M) return fail(TGX_ERR_DEVICE, "tgx_substring_df: inconsistent run count");
        d_df = (uint32_t*)dalloc((size_t)n_runs * 4);
        if (!d_df) return fail(TGX_ERR_DEVICE, "out of device memory (generate)");
        G_TRY(hipMemset(d_df, 0, (size_t)n_runs * 4));
        hipLaunchKernelGGL(run_count_kernel, dim3(mblocks), dim3(256), 0, 0, d_keys2, d_vals2, d_run, M, n_runs, d_rep, d_df, d_ctr + 1);
        G_TRY(hipGetLastError());
        hipLaunchKernelGGL(run_check_kernel, dim3(mblocks), dim3(256), 0, 0, d_text, d_vals2, d_run, M, n_runs, d_rep, d_ctr, d_ctr + 1);
        G_TRY(hipGetLastError());
        stage_end(kGenStageRuns);
        unsigned long long ctr[2] = {0, 0};  // [0] entries that met a foreign run (a key collision), [1] entries whose run id was out of range
        G_TRY(hipMemcpy(ctr, d_ctr, 16, hipMemcpyDeviceToHost));
        if (ctr[1]) return fail(TGX_ERR_DEVICE, "tgx_substring_df: entries with a run id outside [1, n_runs] (run ids corrupt)");
        coll = ctr[0];
        coll_total += coll;
        if (!coll) break;  // every run is one substring: the counts are exact
    }
    if (a.n_collisions) *a.n_collisions = coll_total;
    if (coll) return fail(TGX_ERR_UNSUPPORTED, "tgx_substring_df: different substrings shared a 64-bit key under four independent hashes");
    if (a.n_distinct) *a.n_distinct = n_runs;
    // top_k: only the top_k most frequent substrings leave the device (VocabularyGenerator::generate keeps the most
    // frequent ones, src/generate.rs:150-152, 199-213): a stable descending radix sort of (df, representative) —
    // equal frequencies stay in ascending hash order —, and the frequency of the first substring that is cut off
    uint64_t n_ret = n_runs;
    if (top_k && top_k < n_runs) {
        uint32_t* d_df2 = (uint32_t*)dalloc((size_t)n_runs * 4);
        uint64_t* d_rep2 = (uint64_t*)dalloc((size_t)n_runs * 8);
        if (!d_df2 || !d_rep2) return fail(TGX_ERR_DEVICE, "out of device memory (generate: top-k)");
        stage_begin(kGenStageTop);
        size_t tb = 0;
        G_TRY(rocprim::radix_sort_pairs_desc(nullptr, tb, d_df, d_df2, d_rep, d_rep2, (size_t)n_runs));
        void* tmp = dalloc(tb);
        if (!tmp) return fail(TGX_ERR_DEVICE, "out of device memory (generate: top-k sort)");
        G_TRY(rocprim::radix_sort_pairs_desc(tmp, tb, d_df, d_df2, d_rep, d_rep2, (size_t)n_runs));
        stage_end(kGenStageTop);
        uint32_t cut = 0;
        G_TRY(hipMemcpy(&cut, d_df2 + top_k, 4, hipMemcpyDeviceToHost));
        if (a.cutoff_df) *a.cutoff_df = cut;
        d_df = d_df2;
        d_rep = d_rep2;
        n_ret = top_k;
    }
    n_runs = (uint32_t)n_ret;
    std::vector<uint64_t> rep(n_runs);
    uint64_t* pos = (uint64_t*)malloc(sizeof(uint64_t) * std::max<uint32_t>(n_runs, 1));
    uint32_t* len = (uint32_t*)malloc(sizeof(uint32_t) * std::max<uint32_t>(n_runs, 1));
    uint32_t* df = (uint32_t*)malloc(sizeof(uint32_t) * std::max<uint32_t>(n_runs, 1));
    if (!pos || !len || !df) {
        free(pos);
        free(len);
        free(df);
        return fail(TGX_ERR_INVALID, "tgx_substring_df: out of host memory");
    }
    if (hipMemcpy(rep.data(), d_rep, (size_t)n_runs * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(df, d_df, (size_t)n_runs * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        free(pos);
        free(len);
        free(df);
        return fail(TGX_ERR_DEVICE, "tgx_substring_df: copy of the result failed");
    }
    for (uint32_t r = 0; r < n_runs; r++) {
        pos[r] = (rep[r] >> 5) & 0xFFFFFFFFull;
        len[r] = (uint32_t)(rep[r] & 31u) + 1u;
    }
    scratch.release();
    *a.out_pos = pos;
    *a.out_len = len;
    *a.out_df = df;
    *a.n_out = n_runs;
    return TGX_OK;
}

namespace {

// Document frequencies of the char-aligned substrings of at most max_token_length (<= 32) bytes of the parts
// text[part_begin[k], part_end[k]) (sorted, disjoint; part_sample[k] non-decreasing), every OCCURRENCE kept with probability
// insert_probability (src/generate.rs:84-89, 108-113: a substring with k occurrences in a sample is counted for it with
// probability 1 - (1 - p)^k); part_origin[k]: where the part's sample begins in `text` (NULL: the part is its own sample) —
// the draw of an occurrence is tgx_generate_u01(seed, sample, offset in the sample << 8 | length).  Out: one entry per distinct substring — the position and length
// of one occurrence and the number of samples it occurs in — malloc'd (tgx_free), in ascending order of the
// substrings' sort keys (their FNV-1a hashes).  Two different substrings with one 64-bit key are DETECTED (every entry of
// a run is compared with the run's first, byte by byte) and resolved: the pass is sorted again under a second, salted hash
// of the windows' bytes, up to three times; *n_collisions reports how many entries met a foreign run in the attempts that
// were discarded.  text must be < 4 GiB.
tgx_status substring_df_impl(const GenerateArgs& a) {
    bool empty = false;
    tgx_status st = substring_df_check(a, &empty);
    if (st != TGX_OK || empty) return st;
    GenerateScratch scratch;
    GenerateInput in{};
    if ((st = substring_df_upload(a, scratch, &in)) != TGX_OK) return st;
    const bool dbg = generate_debug();
    uint32_t* d_bc = (uint32_t*)scratch.alloc(in.n_blocks * 4);
    uint64_t* d_bo = (uint64_t*)scratch.alloc((in.n_blocks + 1) * 8);
    if (!d_bc || !d_bo) return generate_fail(scratch, TGX_ERR_DEVICE, "out of device memory (generate)");
    WindowParams P{};
    P.text = in.text;
    P.n_bytes = a.n_bytes;
    P.part_begin = in.part_begin;
    P.part_end = in.part_end;
    P.part_sample = in.part_sample;
    P.part_origin = in.part_origin;
    P.n_parts = a.n_parts;
    P.blk_part = in.blk_part;
    P.max_len = a.max_token_length;
    P.prob = a.insert_probability;
    P.seed = a.seed;
    P.blk_count = d_bc;
    hipLaunchKernelGGL(window_kernel<false>, dim3((uint32_t)in.n_blocks), dim3(256), 0, 0, P);
    G_TRY(hipGetLastError());
    uint64_t M = 0;
    if ((st = substring_df_offsets(scratch, d_bc, d_bo, in.n_blocks, &M)) != TGX_OK) return st;
    P.blk_offs = d_bo;
    return substring_df_tail(a, scratch, in, M, [&](uint64_t salt, uint64_t key_mask, uint64_t* keys, uint64_t* vals) {
        P.salt = salt;
        P.key_mask = key_mask;
        P.keys = keys;
        P.vals = vals;
        hipLaunchKernelGGL(window_kernel<true>, dim3((uint32_t)in.n_blocks), dim3(256), 0, 0, P);
        return hipGetLastError();
    }, nullptr);
}

#undef G_TRY

}  // namespace

}  // namespace tgx

extern "C" {

double tgx_generate_u01(uint64_t seed, uint64_t sample, uint64_t window_hash) { return tgx::generate_u01(seed, sample, window_hash); }

tgx_status tgx_substring_df(int device, const uint8_t* text, uint64_t n_bytes, const uint64_t* part_begin,
                            const uint64_t* part_end, const uint32_t* part_sample, const uint64_t* part_origin, uint64_t n_parts,
                            uint32_t max_token_length, double insert_probability, uint64_t seed, uint64_t** out_pos,
                            uint32_t** out_len, uint32_t** out_df, uint64_t* n_out, uint64_t* n_windows,
                            uint64_t* n_collisions) {
    return tgx::substring_df_impl({device, text, n_bytes, part_begin, part_end, part_sample, part_origin, n_parts, max_token_length, insert_probability, seed, 0,
                                   out_pos, out_len, out_df, n_out, n_windows, n_collisions, nullptr, nullptr});
}

// The same with only the top_k most frequent substrings returned (descending frequency; 0 = all): *n_distinct = the
// number of distinct substrings counted, *cutoff_df = the frequency of the most frequent substring that was NOT
// returned (0 when nothing was cut) — every substring that is not in the output occurs in at most that many
// samples, which is what lets a caller that accumulates several calls decide whether its selection is exact.
tgx_status tgx_substring_df_top(int device, const uint8_t* text, uint64_t n_bytes, const uint64_t* part_begin,
                                const uint64_t* part_end, const uint32_t* part_sample, const uint64_t* part_origin, uint64_t n_parts,
                                uint32_t max_token_length, double insert_probability, uint64_t seed, uint64_t top_k,
                                uint64_t** out_pos, uint32_t** out_len, uint32_t** out_df, uint64_t* n_out,
                                uint64_t* n_windows, uint64_t* n_collisions, uint64_t* n_distinct, uint32_t* cutoff_df) {
    return tgx::substring_df_impl({device, text, n_bytes, part_begin, part_end, part_sample, part_origin, n_parts, max_token_length, insert_probability, seed,
                                   top_k, out_pos, out_len, out_df, n_out, n_windows, n_collisions, n_distinct, cutoff_df});
}

}  // extern "C"
