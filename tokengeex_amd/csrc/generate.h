// What the two window stages of the document-frequency pass share (generate.hip: every char-aligned window; allow.hip:
// the windows an allow automaton accepts, include/tgx_allow.h): the keep rule's draw, the two hash chains of a window's
// bytes, and everything of a call that is not its windows — the arguments' checks, the upload of the text and the parts,
// the scan of the kept counts and the TAIL: the sort by key, the runs, their document frequencies, the byte-by-byte
// collision check with its salted retries, the top-k selection and the malloc'd outputs.  The draw and the chains are
// host and device code (host_twins.cpp: tgx_allow_masks_host); the rest is defined in generate.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

constexpr uint64_t kFnvOffset = 0xCBF29CE484222325ULL, kFnvPrime = 0x100000001B3ULL;
constexpr uint32_t kGenerateBlock = 256;  // positions of a block: the unit of blk_part

// same function as tgx_generate_u01 (include/tgx.h) and tokengeex_amd/generate.py::_u01
__host__ __device__ inline double generate_u01(uint64_t seed, uint64_t sample, uint64_t h) {
    uint64_t x = seed ^ (sample * 0x9E3779B97F4A7C15ULL) ^ (h * 0xC2B2AE3D27D4EB4FULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}
// one draw per OCCURRENCE (src/generate.rs:84-89, 108-113: `rng.gen_range(0.0..1.0) < insert_probability` inside the loops
// over positions and lengths): the stand-in for the thread RNG hashes (seed, sample, offset in the sample, length)
__host__ __device__ inline bool generate_keep(double prob, uint64_t seed, uint32_t sample, uint64_t offset_in_sample, uint32_t len) {
    return prob >= 1.0 || generate_u01(seed, sample, (offset_in_sample << 8) | len) < prob;
}
// byte c into a window's two chains: h is FNV-1a 64; g, begun at kFnvOffset ^ salt, an unrelated mixing chain under which
// keys that met under h part (the retry after a collision; only followed when salt != 0)
__host__ __device__ inline void generate_hash_byte(uint64_t c, uint64_t salt, uint64_t& h, uint64_t& g) {
    h = (h ^ c) * kFnvPrime;
    if (salt) g = ((g ^ c) * 0x9E3779B97F4A7C15ULL) ^ (g >> 29);
}
// a window's entry: sample << 37 | position << 5 | (length - 1)
__host__ __device__ inline uint64_t generate_value(uint32_t sample, uint64_t pos, uint32_t len) {
    return ((uint64_t)sample << 37) | (pos << 5) | (uint64_t)(len - 1u);
}


// ---- the checks of a call's sizes and parts: NULL, or what is wrong ---------------------------------------------------------
// (windows of up to 32 bytes: the reference's CLI default is 24, src/cli.rs:675; a value carries length - 1 in 5 bits)
inline const char* generate_check_sizes(uint64_t n_bytes, uint32_t max_token_length) {  // TGX_ERR_UNSUPPORTED
    if (max_token_length < 1 || max_token_length > 32) return "tgx_substring_df: max_token_length must be 1..32";
    if (n_bytes >= (1ull << 32)) return "tgx_substring_df: feed at most 4 GiB per call";
    return nullptr;
}
inline const char* generate_check_parts(uint64_t n_bytes, const uint64_t* part_begin, const uint64_t* part_end, const uint32_t* part_sample,
                                        const uint64_t* part_origin, uint64_t n_parts) {  // TGX_ERR_INVALID
    for (uint64_t k = 0; k < n_parts; k++) {
        if (part_origin && part_origin[k] > part_begin[k]) return "tgx_substring_df: a part begins before its sample";
        if (part_end[k] < part_begin[k] || part_end[k] > n_bytes || (k && part_begin[k] < part_end[k - 1]) ||
            (k && part_sample[k] < part_sample[k - 1]) || part_sample[k] >= (1u << 27))
            return "tgx_substring_df: parts must be sorted, disjoint, inside the text, with ascending sample ids below 2^27";
    }
    return nullptr;
}

}  // namespace tgx

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without HIP calls)

#include <functional>
#include <vector>

#include "device_internal.h"

namespace tgx {

// the stages a timed call reports (tgx_allow_last_times): the first two are the caller's, the others the tail's
constexpr int kGenerateStages = 6;
enum { kGenStageCount = 0, kGenStageScan = 1, kGenStageEmit = 2, kGenStageSort = 3, kGenStageRuns = 4, kGenStageTop = 5 };
using GenerateTimer = dev::StageTimer<kGenerateStages>;

// The device buffers of one call: hipMalloc'd past the pool, covered by TGX_POOL_FILL all the same, freed together.
struct GenerateScratch {
    int device = 0;
    std::vector<void*> owned;
    void* alloc(size_t bytes);  // NULL: out of device memory
    void release();             // after the device has finished (or failed): hipFree of everything
};

struct GenerateArgs {  // the arguments tgx_substring_df_top and tgx_substring_df_allow share
    int device;
    const uint8_t* text;
    uint64_t n_bytes;
    const uint64_t *part_begin, *part_end;
    const uint32_t* part_sample;
    const uint64_t* part_origin;
    uint64_t n_parts;
    uint32_t max_token_length;
    double insert_probability;
    uint64_t seed, top_k;
    uint64_t** out_pos;
    uint32_t** out_len;
    uint32_t** out_df;
    uint64_t *n_out, *n_windows, *n_collisions, *n_distinct;
    uint32_t* cutoff_df;
};

struct GenerateInput {  // the call's text and parts on the device
    const uint8_t* text;  // n_bytes and 64 zero bytes
    const uint64_t *part_begin, *part_end, *part_origin;
    const uint32_t *part_sample, *blk_part;  // blk_part[b]: the first part whose end lies beyond position 256 b
    uint64_t n_blocks;
    unsigned long long* ctr;  // 8 words, zero
};

// Clears the outputs and checks the arguments; *empty: a valid call with nothing to count (TGX_OK, nothing more to do).
tgx_status substring_df_check(const GenerateArgs& a, bool* empty);
// the device's check, hipSetDevice, and the uploads
tgx_status substring_df_upload(const GenerateArgs& a, GenerateScratch& scratch, GenerateInput* in);
// offs[i] = the sum of count[0 .. i), u64, of n > 0 counts; *total = their sum
tgx_status substring_df_offsets(GenerateScratch& scratch, const uint32_t* d_count, uint64_t* d_offs, uint64_t n, uint64_t* total);
// pass 2 of a path's windows under (salt, key_mask): the M entries {key, value} in position order
using GenerateEmit = std::function<hipError_t(uint64_t salt, uint64_t key_mask, uint64_t* keys, uint64_t* vals)>;
// Everything after the windows' count M.  Frees the scratch on every path; timer may be NULL.
tgx_status substring_df_tail(const GenerateArgs& a, GenerateScratch& scratch, const GenerateInput& in, uint64_t M, const GenerateEmit& emit, GenerateTimer* timer);

}  // namespace tgx

#endif  // TGX_HOST_ONLY
