// Kernel parameter blocks and launchers shared by kernels.hip and the passes (tgx_api.cpp, encode_pass.cpp, estep_pass.cpp,
// lattice_pass.cpp).  The fills of the result- and corpus-side transforms (assemble, fim, select, pack, windows, flat spans,
// decode) share one owner search, tile arithmetic and launch geometry, and fim, select and decode one tile loop and its stores:
// tile_fill.h, which the headers below include.  scan_helpers.h beside it has the block sum and the rocPRIM scans that
// front.hip, norm.hip, fim.hip and select.hip share; only translation units with kernels include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode.h"
#include "encode5_layout.h"
#include "fim.h"
#include "spans.h"

namespace tgx {

// Default stride exponent of the trace kernels' hop stage (trace_body.h: trace_hops; TGX_TRACE_STRIDE overrides it).
constexpr uint32_t kTraceStride = 2;

struct EncodeParams {
    const uint8_t* text;            // u8[N (+ pad)]
    const uint64_t* offs;           // u64[S+1]
    const uint32_t* order;          // u32[S] sample processing order (longest first)
    uint64_t n_samples;
    const void* trie;               // TrieRec[n_slots] (16 B each)
    const uint32_t* tokid;          // u32[n_slots]
    uint32_t root_base;
    uint32_t n_slots;               // trie slots (guards the handle -> id lookup)
    uint32_t lm;                    // max token length rounded up (<= 64)
    uint32_t* bp;                   // u32[N] back-pointer scratch
    uint32_t* tmp;                  // u32[N] right-aligned ids per sample
    uint32_t* counts;               // u32[S] tokens per sample
    uint32_t* status;               // u32[S] 1 = end of sample reachable (encode4 -> trace)
    uint8_t* bp8;                   // u8[N] rows4 back-pointers: len - 1, 0xFF = unreachable
    const void* tokhash;            // TokHashEntry[mask + 1]: token bytes -> id (rows4 trace)
    uint32_t tokhash_mask;
    uint32_t tokhash_seed;
    unsigned long long* err_sample; // min failing sample (init ~0)
    unsigned long long* queue;      // rows4: next unclaimed position of `order` (init 0)
    unsigned long long* redo_count; // encode4l_kernel: samples whose wave ran out of overflow entries (init 0) ...
    uint32_t* redo_list;            // ... and their indices, u32[S]: encode2_kernel redoes exactly those
    double dropout;
    uint64_t seed;
    uint32_t flags;                 // timing experiments only (TGX_FLAGS env): see kernels.hip
    unsigned long long* stamps;     // diagnostic build only (TGX_STAMPS=1): 8 u64 per wave
    uint32_t trace_carry;           // trace kernels: waiting tokens carry over from sample to sample (short samples: trace_body.h)
    uint32_t trace_stride;          // trace kernels: the hop chain visits every 2^trace_stride-th token of a window's path (0 .. 3: trace_body.h)
};

// encode5_kernel / encode6_kernel (encode5.hip): 8-byte label-checked records, score values by rank
struct Encode5Params {
    const void* trie8;              // Trie8Rec[n_slots]
    uint32_t trie_bytes;            // 8 * n_slots
    const double* values;           // f64[n_values + 1]: values[0] = -inf, values[r] = the score value of rank r
    uint32_t root_base;
    uint32_t n_values;              // distinct score values of the vocabulary (<= 65 535)
    uint32_t n_hot;                 // ranks 1..n_hot are copied into the block's LDS; COLD builds read the rest from `values`
    uint32_t claim_chunk;           // consecutive samples of the order a row claims per atomic (>= 1)
    uint32_t list_off, root_off, idx_off;  // LDS layout (set by the launcher)
    uint32_t ctrl_off, ring_off, ring_slots;  // encode6_kernel: control words, ring of match-index buffers
    uint32_t pool;                            // encode6_kernel, COLD builds: pool entries per ring slot for values its walkers fetch (0: none)
    unsigned int* started;                    // encode5_kernel: when not null, every block adds 1 here once it is resident (host-visible memory:
                                              // the co-run launches the long-sample kernel only after all of them are)
    const void* top;                          // encode5_kernel, TOP builds: the top table (top_table.h), Trie8Rec[65 536]
};

struct CompactParams {
    const uint64_t* offs;
    const uint32_t* order;
    uint64_t n_samples;
    const uint32_t* tmp;
    const uint64_t* out_offs;
    uint32_t* ids;
};

struct EstepParams {
    const uint8_t* text;
    const uint64_t* offs;
    const uint32_t* order;
    uint64_t n_samples;
    const void* trie_fwd;           // tokens as written (forward sweep)
    const void* trie_rev;           // reversed tokens (backward sweep)
    uint32_t root_fwd, root_rev;
    uint32_t lm;                    // max token length rounded up (<= 64)
    uint64_t snippet_len;           // 81920 in the reference (prune.rs:75)
    double* alpha;                  // f64[N + S + pad] forward values, sample s at offs[s] + s
    double* expected_slot;          // f64[n_replicas][n_slots_rev] expected counts per reversed-trie slot
    uint32_t n_slots_rev, n_replicas;
    double* logz_sum;
    unsigned long long* err_sample; // min sample whose z is not normal (init ~0)
    double dropout;
    uint64_t seed;
};

hipError_t launch_pair_keys(const uint32_t* ids, const uint64_t* out_offs, uint64_t n_samples, uint32_t shift,
                            unsigned long long sentinel, unsigned long long* keys, uint32_t blocks, hipStream_t stream);
hipError_t pair_sort_temp_bytes(uint64_t n, size_t* bytes);
hipError_t pair_sort(void* temp, size_t temp_bytes, const unsigned long long* in, unsigned long long* out,
                     uint64_t n, unsigned int end_bit, hipStream_t stream);
hipError_t pair_rle_temp_bytes(uint64_t n, size_t* bytes);
hipError_t pair_rle(void* temp, size_t temp_bytes, const unsigned long long* sorted, uint64_t n,
                    unsigned long long* unique_out, unsigned int* counts_out, unsigned int* n_runs_out,
                    hipStream_t stream);

hipError_t pair_count_sort_temp_bytes(uint64_t n, size_t* bytes);
hipError_t pair_count_sort(void* temp, size_t temp_bytes, const unsigned int* counts_in, unsigned int* counts_out,
                           const unsigned long long* keys_in, unsigned long long* keys_out, uint64_t n,
                           hipStream_t stream);
hipError_t launch_pair_expand(const unsigned long long* keys, const unsigned int* cnt, uint64_t n, uint32_t shift,
                              unsigned long long* out_keys, unsigned long long* out_counts, hipStream_t stream);
constexpr uint32_t kHistMaxVocab = 36864;  // ids whose u32 counters fit one block's LDS (144 KiB)
hipError_t launch_ids_histogram(const uint32_t* ids, uint64_t n, uint32_t vocab, unsigned long long* out, uint32_t blocks,
                                hipStream_t stream);
hipError_t ids_sort_temp_bytes(uint64_t n, size_t* bytes);
hipError_t ids_sort(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint64_t n,
                    unsigned int end_bit, hipStream_t stream);
hipError_t ids_rle_temp_bytes(uint64_t n, size_t* bytes);
hipError_t ids_rle(void* temp, size_t temp_bytes, const uint32_t* sorted, uint64_t n, uint32_t* unique_out,
                   unsigned int* counts_out, unsigned int* n_runs_out, hipStream_t stream);

// four-snippets-per-wave E-step (estep4.hip): the work list is the list of snippets
struct Estep4Params {
    const uint8_t* text;            // 256-byte front pad: the backward sweep reads 16 bytes before a position
    const uint64_t* soffs;          // u64[K+1] snippet k = text[soffs[k] .. soffs[k+1])
    const uint32_t* order;          // u32[K] longest first
    uint64_t n_snips;
    const uint32_t* snip_sample;    // u32[K] sample of the snippet        (dropout hash only)
    const uint64_t* snip_base;      // u64[K] its byte offset in the sample (dropout hash only)
    const void* trie_fwd;
    const void* trie_rev;
    uint32_t root_fwd, root_rev;
    double* alpha;                  // f64[N + K + pad]: snippet k's A[0..n] at soffs[k] + k
    double* zarr;                   // f64[K] z = A[n] per snippet
    int32_t* alpha_exp;             // linear-domain kernels (estep4l.hip): power-of-two exponent of each block of 16
                                    // alpha values, snippet k's blocks at (soffs[k] >> 4) + k
    double* expected_slot;          // f64[n_replicas][n_slots_rev]
    uint32_t n_slots_rev, n_replicas;
    uint32_t n_hot;                 // estep4l_bwd_kernel: slots summed in the block's LDS (set by its launcher)
    double* logz_sum;
    unsigned long long* err_snip;   // min snippet whose z is not normal (init ~0)
    uint32_t flags;                 // timing experiments only (TGX_FLAGS with TGX_DEBUG=1): 8 = no cold-slot atomics
    unsigned long long* range_flag; // linear-domain forward kernel: set when the pass needs the log-domain kernels (init 0)
    unsigned long long* queue_fwd;  // next unclaimed position of `order`, forward / backward kernel (init 0)
    unsigned long long* queue_bwd;
    double dropout;
    uint64_t seed;
};
// cuts.hip: positions no token match crosses (the lattice factorises there): long snippets are cut into pieces
struct CutParams {
    const uint8_t* text;
    const uint64_t* soffs;          // u64[K+1] snippets
    const uint32_t* snip_sample;    // u32[K], u64[K]: dropout hash bookkeeping of the snippets
    const uint64_t* snip_base;
    const uint32_t* win_snip;       // u32[W] snippet of window w (windows in text order)
    const uint32_t* win_k;          // u32[W] its number within the snippet; window 0 stands for the snippet's start
    uint64_t n_windows;
    uint32_t window;                // bytes per window
    const void* trie;               // 16-byte records (check, base | terminal << 31, ...)
    uint32_t root;
    uint32_t lmx;                   // longest token, rounded up to 16 or 32
    double dropout;
    uint64_t seed;
    uint64_t* bound;                // out u64[W]: the window's boundary (absolute byte offset) or ~0
    uint32_t* flag;                 // out u32[W]: 1 iff bound[w] != ~0
};
hipError_t launch_cut_windows(const CutParams& p, hipStream_t stream);
hipError_t launch_cut_scatter(const CutParams& p, const uint64_t* pos, uint64_t n_bytes, uint64_t* poffs, uint32_t* psample,
                              uint64_t* pbase, uint32_t* psnip, hipStream_t stream);
hipError_t launch_piece_len(const uint64_t* poffs, const uint64_t* n_pieces, uint32_t* len, uint32_t* idx, unsigned long long* longest,
                            uint64_t cap, hipStream_t stream);
hipError_t piece_sort_temp_bytes(uint64_t n, size_t* bytes);
hipError_t piece_sort(void* temp, size_t temp_bytes, const uint32_t* len_in, uint32_t* len_out, const uint32_t* idx_in, uint32_t* idx_out,
                      uint64_t n, hipStream_t stream);
hipError_t launch_piece_z_check(const double* zarr, const uint32_t* psnip, uint64_t n_pieces, double* zsnip, uint64_t n_snips,
                                unsigned long long* err_snip, hipStream_t stream);

// estep7_kernel (estep7.hip): the E-step with one walk per position — every trip of a row is a lattice of its own
// between two positions no match crosses; match entries are token ranks (trie_build.h: Trie8T)
// (what a row needs once per piece or less often lives behind a pointer, in device memory: as kernel arguments these
// twenty scalar-register pairs pushed the buffer resources of the walk out to spilled lanes — 4 v_readlane and their
// hazard nops per walk level)
struct Estep7Work {
    const uint64_t* soffs;          // u64[K+1] pieces (or snippets): k = text[soffs[k] .. soffs[k+1])
    const uint32_t* order;          // u32[K]
    uint64_t n_snips;
    const uint32_t* snip_sample;    // u32[K], u64[K]: sample and offset in the sample (dropout hash only)
    const uint64_t* snip_base;
    const uint32_t* snip_of;        // u32[K] snippet a piece belongs to (z is summed per snippet); null: k itself
    double* zsnip;                  // f64[snippets] log Z per snippet (sum of its pieces' trips)
    double* logz_sum;
    unsigned long long* range_flag; // 1: a position nothing reaches or a value out of range; 4: redo list full
    unsigned long long* queue;
    unsigned long long* redo_count; // stretches the kernel could not do (no cut within a trip) ...
    uint64_t* redo_offs;            // ... u64[2 cap]: [2 i], [2 i + 1] = begin and end of stretch i
    uint32_t* redo_sample;          // u32[2 cap], u64[2 cap], u32[2 cap]: sample, offset in the sample, snippet (entries 2 i and 2 i + 1 alike)
    uint64_t* redo_base;
    uint32_t* redo_snip;
    uint64_t redo_cap;
};
struct Estep7Params {
    const uint8_t* text;
    const Estep7Work* work;         // device memory (the launcher uploads `host_work` there)
    Estep7Work host_work;           // filled by the caller; not read by the kernel
    const void* trie8t;             // Trie8TRec[n_slots]
    uint32_t n_slots;
    uint32_t root_base;
    const double* wtab;             // f64[n_tok + 1]: [0] = 0, [r] = exp(score of the token of rank r)
    uint32_t n_tok;                 // tokens that can match (ranks 1 .. n_tok)
    uint32_t ovf_limit;             // 16-bit builds: a match of a rank beyond it sends its trip to the redo kernel (0xFFFFFFFF: none can occur)
    uint32_t n_hot;                 // ranks 1 .. n_hot have {sum, w} in the block's LDS
    double* expected;               // f64[n_tok + 1] expected counts by rank
    double dropout;
    uint64_t seed;
    uint32_t claim_chunk;
    uint32_t root_off, zero_off, idx_off;  // LDS layout (set by the launcher)
    uint32_t flags;                 // timing experiments only (TGX_FLAGS with TGX_DEBUG=1): results are WRONG when set
    unsigned long long* stamps;     // diagnostic runs only (TGX_STAMPS=7 with TGX_DEBUG=1): 8 u64 per wave
};
struct Estep7RedoParams {
    const uint8_t* text;
    const uint64_t* redo_offs;      // as written by estep7_kernel
    const uint32_t* redo_sample;
    const uint64_t* redo_base;
    const uint32_t* redo_snip;
    uint64_t n_redo;
    const uint64_t* tbase;          // u64[n_redo]: trips of the stretches before stretch i (the scratch layout)
    const void* trie8t;
    uint32_t n_slots;
    uint32_t root_base;
    const double* wtab;
    uint32_t n_tok, n_hot;
    double* expected;
    double* zsnip;
    double* logz_sum;
    unsigned long long* range_flag;
    unsigned long long* queue;
    double* alpha;                  // f64[16 trips]
    int32_t* aexp;                  // i32[trips]
    unsigned char* mscratch;        // row images of the trips' match entries: trips x 512 (1024) bytes
    double dropout;
    uint64_t seed;
    uint32_t root_off, zero_off, idx_off;  // LDS layout (set by the launcher)
};
uint32_t estep7_redo_max_hot(bool wide);
hipError_t launch_estep7_redo(Estep7RedoParams p, bool wide, uint32_t num_cus, hipStream_t stream);
uint32_t estep7_lds_layout(uint32_t n_hot, bool wide, int waves, int ppl, uint32_t* root_off, uint32_t* zero_off, uint32_t* idx_off);
uint32_t estep7_max_hot(bool wide, int waves, int ppl, uint32_t budget);
hipError_t estep7_waves_per_simd(bool dropout, bool cold, bool wide, int ppl, int* out);
hipError_t launch_estep7(Estep7Params p, bool wide, int ppl, int waves, uint32_t blocks, hipStream_t stream);
// How often every token MATCHES in a sample of the text (chunks of `chunk` bytes every `stride` bytes): counts[rank] += 1
// per position of the sample and token that is a prefix of the text there.  The E-step adds to a token's expected count
// once per match, whatever its score: the ranks that stay in LDS are chosen by these counts (estep_pass.cpp).
hipError_t launch_match_count(const uint8_t* text, uint64_t n_bytes, uint32_t chunk, uint64_t stride, const void* trie8t, uint32_t n_slots,
                              uint32_t root_base, uint32_t n_tok, unsigned int* counts, uint32_t num_cus, hipStream_t stream);
// the same over encode5_kernel's records: counts[rank of the score value] (walks of up to max_len bytes)
hipError_t launch_value_count(const uint8_t* text, uint64_t n_bytes, uint32_t chunk, uint64_t stride, const void* trie8, uint32_t n_slots,
                              uint32_t root_base, uint32_t n_values, uint32_t max_len, unsigned int* counts, uint32_t num_cus, hipStream_t stream);
// rec[t].tok = perm[rec[t].tok] for every slot of the 8-byte E-step records (and encode5_kernel's: the second word is the rank there too)
// rank_mask: the bits of the word that hold the rank (encode5_kernel's records: kTrie8RankMask); the others are dropped
hipError_t launch_rank_remap(void* trie8t, uint32_t n_slots, const uint32_t* perm, uint32_t rank_mask, hipStream_t stream);
// the same for encode5_kernel's top table (top_table.h), whose second words hold a rank in either half
hipError_t launch_rank_remap_top(void* top, const uint32_t* perm, hipStream_t stream);
hipError_t launch_snip_z_check(const double* zsnip, uint64_t n_snips, unsigned long long* err_snip, hipStream_t stream);
hipError_t launch_piece_z_add(const double* zarr, const uint32_t* psnip, const uint32_t* order, uint64_t n_order, double* zsnip, hipStream_t stream);

hipError_t estep4_prepare();
hipError_t launch_estep4_fwd(const Estep4Params& p, uint32_t num_cus, hipStream_t stream);
hipError_t launch_estep4_bwd(const Estep4Params& p, uint32_t num_cus, hipStream_t stream);
hipError_t estep4l_prepare();
hipError_t launch_estep4l_fwd(const Estep4Params& p, int ppl, bool long_tokens, uint32_t num_cus, hipStream_t stream);
hipError_t launch_estep4l_bwd(const Estep4Params& p, int ppl, bool long_tokens, uint32_t num_cus, uint32_t groups_wanted, hipStream_t stream);
hipError_t launch_estep4_reduce(const double* rep, double* out, uint32_t n_slots, uint32_t n_replicas,
                                hipStream_t stream);

uint32_t estep_lds_bytes_per_block(uint32_t lm);
uint32_t estep_waves_per_block(uint32_t lm);
hipError_t estep_max_blocks_per_cu(uint32_t lm, int* out);
hipError_t launch_estep(const EstepParams& p, uint32_t blocks, hipStream_t stream);

uint32_t encode_lds_bytes_per_block(uint32_t lm);
uint32_t encode_waves_per_block(uint32_t lm);
hipError_t encode_max_blocks_per_cu(uint32_t lm, int* out);
hipError_t launch_encode(const EncodeParams& p, uint32_t blocks, hipStream_t stream);
uint32_t encode4_group_bytes();
hipError_t encode4_waves_per_simd(bool dropout, int ppl, bool root, int* out);
hipError_t launch_encode4(const EncodeParams& p, int ppl, int waves, uint32_t blocks, bool root, hipStream_t stream);
uint32_t encode4_lds_bytes(int waves, int ppl, bool root);
hipError_t launch_trace(const EncodeParams& p, uint32_t blocks, hipStream_t stream);
// The trace that writes ids in place (trace_body.h: INPLACE): p.counts holds every sample's token count already
// (encode5_kernel's counting builds) and o.out_offs their scan.  p.tmp is not used.
struct TraceInPlace {
    const uint64_t* out_offs;  // u64[S+1]: the result's offsets
    uint32_t* ids;             // u32[out_offs[S]]: the result's ids
};
hipError_t launch_trace_in_place(const EncodeParams& p, const TraceInPlace& o, uint32_t blocks, hipStream_t stream);
// err_sample code bits of the trace kernels (the plain value: the lowest sample whose end is not reached)
constexpr unsigned long long kErrCorruptBp = 1ULL << 62;      // a back-pointer that names no vocabulary token (low bits: the text byte)
constexpr unsigned long long kErrCountMismatch = 1ULL << 61;  // in place: the trace's token count differs from P.counts (low bits: the sample)
// (encode5_lds_layout, encode5_max_hot: encode5_layout.h)
// lean: the kernels with the lean relaxation step (TGX_E5_LEAN; device_common.h: relax5_lean_step) — the dropout and
// long-token builds have none and run the step as it was (encode5_has_lean)
bool encode5_has_lean(bool dropout, bool long_tokens);
// the items (device_common.h: kLeanStep | kLeanBcast | kLeanFetch) of the lean build of encode5_kernel (hot /
// COLD, positions per lane; step_ok: the scores pass the lean step's gate, else the build without the step) and encode6_kernel
int encode5_lean_items(bool cold, int ppl, bool step_ok);
int encode6_lean_items();
// whether the build of encode5_kernel counts tokens in its relaxation and writes them to P.counts (DESIGN.md section R8;
// decided per build in encode5.hip): the passes of such a build may write ids in place (ids_in_place.h)
bool encode5_counts(bool dropout, bool cold, int ppl, bool long_tokens);
// whether encode5_kernel has a TOP build for these (the first two levels of a walk from the top table,
// no root copy in LDS): every hot and COLD build; the dropout and long-token builds keep their root copy
bool encode5_has_top(bool dropout, bool long_tokens);
// count: ask for the counting build where the geometry has one; top: the TOP build (where encode5_has_top())
hipError_t encode5_waves_per_simd(bool dropout, bool cold, int ppl, bool long_tokens, int compact, bool lean, bool step_ok, bool count, bool top, int* out);
uint32_t encode6_lds_layout(uint32_t n_hot, uint32_t pool, uint32_t* root_off, uint32_t* ctrl_off, uint32_t* ring_off);
uint32_t encode6_max_hot(uint32_t budget, uint32_t pool);
uint32_t encode6_pool_total(uint32_t pool);  // pool entries of a block (index space they take)
// estep5_fwd_kernel (encode5.hip): the E-step's forward sweep over the 8-byte ranked records; q.values = exp(score value) by rank
hipError_t estep5_waves_per_simd(bool dropout, bool cold, int ppl, int* out);
hipError_t launch_estep5_fwd(const struct Estep4Params& p, Encode5Params q, bool cold, int ppl, int waves, uint32_t blocks, hipStream_t stream);
hipError_t launch_encode6(const EncodeParams& p, Encode5Params q, bool cold, bool lean, uint32_t blocks, hipStream_t stream);
// compact: the depth at which the walks of a trip are compacted (0: never; 4 .. 8; encode5.hip: Walk5)
// count: the counting build (an error where encode5_counts() says the build has none)
// top: the TOP build and its LDS layout (an error where encode5_has_top() says the build has none, or without q.top)
hipError_t launch_encode5(const EncodeParams& p, Encode5Params q, bool cold, int ppl, bool long_tokens, int compact, bool lean, bool step_ok, bool count,
                          bool top, int waves, uint32_t blocks, uint32_t min_lds, hipStream_t stream);
hipError_t launch_encode2(const EncodeParams& p, uint32_t num_cus, bool permuted, hipStream_t stream);   // encode2.hip
hipError_t launch_trace32(const EncodeParams& p, uint32_t blocks, bool permuted, hipStream_t stream);
hipError_t launch_encode4l(const EncodeParams& p, uint32_t num_cus, hipStream_t stream);  // encode4l.hip
hipError_t scan_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_scan(uint32_t* counts, uint64_t* offsets, uint64_t n, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_compact(const CompactParams& p, uint32_t blocks, bool rows, hipStream_t stream);

// layout.hip: a result's ids laid out as [S, L] padded rows, a packed stream of [B, L] blocks or [W, L] windows (layout.h has the
// row mapping).  Outputs are caller-owned device memory; any of mask / lengths / doc / pos / counter may be null.
struct LayoutParams {
    const uint32_t* ids;            // u32[T]
    const uint64_t* offs;           // u64[S+1]
    uint64_t n_rows;                // S
    uint32_t len;                   // row_len (padded) or block_len (packed)
    uint32_t pad, bos, eos;         // bos / eos: 0xFFFFFFFF = none
    uint32_t flags;                 // TGX_LAYOUT_*
    void* out;                      // i32 or i64 (TGX_LAYOUT_I64)
    uint8_t* mask;                  // padded: u8[S·L]
    int32_t* lengths;               // padded: i32[S]
    int32_t* doc;                   // packed: i32[n_out]
    int32_t* pos;                   // packed: i32[n_out]
    unsigned long long* counter;    // padded: rows with n_i > L - A are added to it (zeroed by the caller)
};
hipError_t launch_layout_max_row(const uint64_t* offs, uint64_t n_rows, unsigned long long* max_out, hipStream_t stream);
hipError_t launch_layout_pad(const LayoutParams& p, hipStream_t stream);
// n_stream = T + S·A positions hold ids, n_out = n_blocks · block_len elements are written
hipError_t launch_layout_pack(const LayoutParams& p, uint64_t n_stream, uint64_t n_out, hipStream_t stream);
// The windowed layout: base.out / mask / lengths are [W, L] / [W·L] / [W]; base.counter, doc and pos are not used.
struct WindowParams {
    LayoutParams base;
    const uint64_t* wo;             // u64[S+1]: Wo, the rows' first windows (launch_scan over the counts)
    uint32_t stride;                // tokens a window repeats of the one before: < L - A
    int32_t* window_row;            // i32[W] or null: the row a window came from
    int32_t* window_first;          // i32[W] or null: index of its first kept token in that row
};
// counts[i] = the windows of row i (u32[S+1]: the last entry belongs to the scan); the longest row goes to *max_out
// (zeroed by the caller)
hipError_t launch_layout_window_count(const uint64_t* offs, uint64_t n_rows, uint32_t room, uint32_t step, uint32_t* counts,
                                      unsigned long long* max_out, hipStream_t stream);
hipError_t launch_layout_windows(const WindowParams& q, uint64_t n_windows, hipStream_t stream);

// assemble.hip: a sample-level result from the result over the non-special segments and the split plan (assemble.h has
// the index arithmetic).  All pointers are device memory.
struct AssembleParams {
    const uint32_t* ids;            // u32[T]: the segment-level result (not read when no segment is encoded)
    const uint64_t* offs;           // u64[E+1]: its offsets (one zero when no segment is encoded)
    const uint64_t* seg_offs;       // u64[S+1]
    const int32_t* seg_special;     // i32[K+1] (the last entry belongs to the scan)
    uint64_t* rank;                 // u64[K+1]: r_k, written by launch_assemble_ranks
    uint64_t* starts;               // u64[K+1]: D_k, written by assemble_starts_kernel
    uint64_t n_segs, n_samples;     // K, S
    uint64_t n_out;                 // T' = T + (K - E)
    uint32_t vocab_size;            // V: special k gets the id V + k
    uint32_t* out_ids;              // u32[T'], 16-byte aligned
    uint64_t* out_offs;             // u64[S+1]
};
hipError_t assemble_scan_temp_bytes(uint64_t n_segs, size_t* bytes);
hipError_t launch_assemble_ranks(int32_t* seg_special, uint64_t* rank, uint64_t n_segs, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_assemble_starts(const AssembleParams& p, hipStream_t stream);
hipError_t launch_assemble_fill(const AssembleParams& p, hipStream_t stream);

// fim.hip: the rows of a result rearranged for fill-in-the-middle (fim.h has the index arithmetic).  All pointers are
// device memory.
struct FimParams {
    const uint32_t* ids;            // u32[T]: the input result
    const uint64_t* offs;           // u64[S+1]: its offsets
    uint64_t n_rows;                // S
    FimArgs f;                      // seed, first_row, rates and the three sentinel ids
    uint64_t n_out;                 // T' = out_offs[S] (the fill)
    uint32_t* out_ids;              // u32[T'], 16-byte aligned
    uint64_t* out_offs;             // u64[S+1], written by launch_fim_offsets
};
hipError_t fim_scan_temp_bytes(uint64_t n_rows, size_t* bytes);
hipError_t launch_fim_offsets(const FimParams& p, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_fim_fill(const FimParams& p, hipStream_t stream);
// mode u8[S] and cuts u64[2S] (either may be null)
hipError_t launch_fim_info(const FimParams& p, uint8_t* mode, uint64_t* cuts, hipStream_t stream);

// select.hip: rows of a result (u32 ids) or of a corpus (u8 text) selected and reordered through an index (select.h has
// the index arithmetic); the keys and the sort of the seeded permutation.  All pointers are device memory.
struct SelectParams {
    const void* data;               // u32[T] ids or u8[N] text of the source
    const uint64_t* offs;           // u64[S+1]: its offsets
    uint64_t n_src;                 // S
    const int64_t* rows;            // i64[M]: output row k is source row rows[k]
    uint64_t n_rows;                // M
    uint64_t* out_offs;             // u64[M+1], written by launch_select_offsets
    uint64_t n_out;                 // T' = out_offs[M] (the fill)
    void* out;                      // u32[T'] or u8[T'], 16-byte aligned
};
hipError_t select_scan_temp_bytes(uint64_t n_rows, size_t* bytes);
// *bad (set to kSelectNoBad by the caller) = the smallest k whose rows[k] is outside [0, S)
hipError_t launch_select_check(const SelectParams& p, unsigned long long* bad, hipStream_t stream);
hipError_t launch_select_offsets(const SelectParams& p, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_select_fill_ids(const SelectParams& p, hipStream_t stream);
// (the source is a corpus's text: up to 3 bytes on either side of it are read, and lie in the allocation's slack)
hipError_t launch_select_fill_text(const SelectParams& p, hipStream_t stream);
hipError_t launch_select_lengths(const uint64_t* offs, uint64_t n_src, int64_t* lengths, hipStream_t stream);
// the permutation of 0 .. n-1 by (tgx_shuffle_key, index): keys_in, keys_out, vals_in are u64[n] / u64[n] / i64[n] scratch
hipError_t shuffle_sort_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_shuffled_rows(uint64_t n, uint64_t seed, uint64_t* keys_in, uint64_t* keys_out, int64_t* vals_in, int64_t* rows, void* temp,
                                size_t temp_bytes, hipStream_t stream);

// decode.hip: ids decoded to UTF-8 text (decode.h has the index arithmetic).  All pointers are device memory.
struct DecodeParams {
    DecodeTables tab;
    DecodeSrc src;
    uint32_t* meta;                 // u32[N+1]: raw length and class per element (the last entry belongs to the scan)
    uint64_t* starts;               // u64[N+1]: B, the elements' raw byte starts
    uint64_t* specials;             // u64[N+1]: X, live specials before an element; NULL when the stream has none
    unsigned long long* bad_pos;    // lowest stream position of an out-of-bounds element (~0 set by the caller: none)
    unsigned long long* n_replaced; // replacement characters (zeroed by the caller)
    unsigned long long* n_specials_live;  // live special tokens (zeroed by the caller)
    uint64_t n_raw;                 // B[N]
    uint8_t* raw;                   // u8[n_raw rounded up to whole slots, + 16], 16-byte aligned
    uint32_t* flags;                // u32[G]: run starts and verbatim bytes per slot of 16 raw bytes, G = ceil(n_raw / 16)
    uint32_t* codes;                // u32[G+1]: output bytes per raw byte (the last entry belongs to the scan)
    uint64_t* row_offs;             // u64[S+1]: the rows' raw starts, then their final offsets
    uint64_t* gpos;                 // u64[G+1]: the slots' output positions (only after a replacement)
    uint8_t* out;                   // the final bytes (only after a replacement)
};
hipError_t decode_scan_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_decode_meta(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream);      // meta and B
hipError_t launch_decode_specials(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream);  // X
hipError_t launch_decode_fill(const DecodeParams& p, hipStream_t stream);
hipError_t launch_decode_rows(const DecodeParams& p, hipStream_t stream);   // after the fill
hipError_t launch_decode_utf8(const DecodeParams& p, hipStream_t stream);   // after the rows
hipError_t decode_expand_temp_bytes(uint64_t n_groups, size_t* bytes);
hipError_t launch_decode_positions(const DecodeParams& p, void* temp, size_t temp_bytes, hipStream_t stream);
hipError_t launch_decode_expand(const DecodeParams& p, hipStream_t stream);  // the bytes and the rows' final offsets

// spans.hip: the part of its row's text that every token of a result covers, in bytes or characters (spans.h has the
// index arithmetic).  All pointers are device memory.
struct SpanParams {
    SpanTables tab;
    const uint32_t* ids;            // u32[T]
    const uint64_t* offs;           // u64[S+1]
    uint64_t n_rows, n;             // S, T
    uint32_t* vals;                 // u32[T+1]: the elements' value words (the last entry belongs to the scan)
    uint64_t* sums;                 // u64[T+1]: P, the exclusive prefix sums of the values
    unsigned long long* row_max;    // the largest row total (zeroed by the caller)
    uint32_t len;                   // padded: row_len
    uint32_t bos, eos;              // padded: 0xFFFFFFFF = none
    uint32_t flags;                 // TGX_LAYOUT_* | TGX_SPAN_CHARS
    void* out;                      // i32 or i64 (TGX_LAYOUT_I64): [T, 2] or [S, L, 2]
};
hipError_t span_scan_temp_bytes(uint64_t n, size_t* bytes);
hipError_t launch_span_sums(const SpanParams& p, void* temp, size_t temp_bytes, hipStream_t stream);  // vals and P
hipError_t launch_span_row_max(const SpanParams& p, hipStream_t stream);                              // after the sums
hipError_t launch_span_flat(const SpanParams& p, hipStream_t stream);
hipError_t launch_span_pad(const SpanParams& p, hipStream_t stream);
// [W, L, 2] over the windows of WindowParams::wo (p.len = L, p.out = the pairs)
hipError_t launch_span_windows(const SpanParams& p, const uint64_t* wo, uint32_t stride, uint64_t n_windows, hipStream_t stream);

}  // namespace tgx
