// The allow filter inside the document-frequency pass (include/tgx_allow.h: tgx_substring_df_allow): which windows of a
// start byte are KEPT, as a 32-bit mask — bit l - 1 for the window of l bytes.  The kernels of allow.hip and the host twin
// in host_twins.cpp (tgx_allow_masks_host) both go through these functions; the table is find.h's (state, tagged and dead
// in one byte), the draw and the hash chains are generate.h's.  DESIGN.md, section L.24.
//
// The walk.  A start byte p is a character start inside a part that ends at `end`; its walk has limit = min(max_len,
// end - p) bytes.  Trip t fetches byte p + t and does two things with it:
//   settle : a window of t bytes that the automaton accepted at trip t - 1 is PENDING; it is a candidate iff the fetched
//            byte is no continuation byte (the window ends on a character boundary).  A candidate is drawn
//            (generate_keep) and, kept, sets bit t - 1.
//   advance: while t < limit, q = table[b][q].  A dead state ends the walk.  A tagged state makes the window of t + 1
//            bytes pending — or, when it ends at the part's end, a candidate at once.
// So a walk makes at most limit + 1 trips, the last of which only settles, and reads no byte at or past `end` except to
// settle against it, which only happens inside the part.  A start that is no character start, or outside every part,
// has limit 0 and the mask 0.
//
// The geometry.  A CHUNK is 64 positions, a wave's work; four chunks are a block of the parent's blk_part table.  A wave
// takes a run of consecutive chunks.  The kept windows are counted per chunk (not per block: a wave then needs nothing
// from its neighbours, and neither kernel has a barrier after the table's copy); an exclusive scan of the chunks' counts
// gives every chunk its output range, so the entries come out in position order, as the parent's do.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "find.h"
#include "generate.h"

namespace tgx {

constexpr uint32_t kAllowChunk = 64;
constexpr uint32_t kAllowMaxLen = 32;  // a mask's bits; a window and its settling byte lie within a chunk and the 64 bytes behind it
constexpr uint32_t kAllowBlockChunks = kGenerateBlock / kAllowChunk;
static_assert(kAllowChunk + kAllowMaxLen < 2 * kAllowChunk, "byte p + t of a chunk's lane is in the chunk or in the 64 bytes behind it");

__host__ __device__ inline uint64_t allow_chunks(uint64_t n_bytes) { return (n_bytes + kAllowChunk - 1) / kAllowChunk; }

// what a start byte's draws hash
struct AllowDraw {
    double prob;
    uint64_t seed;
    uint32_t sample;
    uint64_t offset;  // of the start byte in its sample
};

struct AllowWalk {
    uint32_t q, mask;
    bool live, pending;
};

__host__ __device__ inline AllowWalk allow_begin(uint32_t start, uint32_t limit) { return {start, 0u, limit != 0, false}; }
__host__ __device__ inline bool allow_busy(const AllowWalk& w) { return w.live || w.pending; }

// trip t of a busy walk: b is byte p + t (any value where the text has ended); ends_part: p + limit is the part's end
__host__ __device__ inline void allow_trip(const uint8_t* table, uint32_t b, uint32_t t, uint32_t limit, bool ends_part, const AllowDraw& d, AllowWalk& w) {
    if (w.pending) {
        if ((b & 0xC0u) != 0x80u && generate_keep(d.prob, d.seed, d.sample, d.offset, t)) w.mask |= 1u << (t - 1);
        w.pending = false;
    }
    if (!w.live) return;
    const uint32_t e = table[b * kDfa64MaxStates + w.q];
    w.q = e & 63u;
    if (e & kFindDead) {
        w.live = false;
        return;
    }
    const bool last = t + 1 == limit;
    if (e & kFindTagged) {
        if (last && ends_part) {
            if (generate_keep(d.prob, d.seed, d.sample, d.offset, t + 1)) w.mask |= 1u << t;
        } else {
            w.pending = true;
        }
    }
    if (last) w.live = false;
}

// the whole walk from p on host memory (the kernel runs the same trips a lane a start, in lockstep)
inline uint32_t allow_mask_host(const uint8_t* table, uint32_t start, const uint8_t* text, uint64_t n_bytes, uint64_t p, uint64_t end, uint32_t max_len,
                                const AllowDraw& d) {
    const uint32_t limit = find_limit(p, end, max_len);
    AllowWalk w = allow_begin(start, limit);
    for (uint32_t t = 0; allow_busy(w); t++) allow_trip(table, p + t < n_bytes ? text[p + t] : 0u, t, limit, p + limit == end, d, w);
    return w.mask;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

struct AllowParams {
    const uint8_t* text;
    uint64_t n_bytes;
    const uint64_t *part_begin, *part_end, *part_origin;
    const uint32_t* part_sample;
    uint64_t n_parts;
    const uint32_t* blk_part;  // per block of 256 positions (four chunks): the first part whose end lies beyond the block's start
    uint32_t max_len, start;
    double prob;
    uint64_t seed;
    const uint8_t* table;  // kFindTableBytes bytes, 16-byte aligned
    uint32_t* mask;        // u32[n_bytes]: allow_mask_kernel writes, allow_emit_kernel reads
    uint32_t* chunk_count;  // u32[allow_chunks(n_bytes)]: the set bits of a chunk's masks
    const uint64_t* chunk_offs;  // their exclusive scan
    uint64_t salt, key_mask;     // the emit's: generate.h's two chains
    uint64_t *keys, *vals;
};

// allow.hip.  All pointers are device memory; n_bytes > 0.
hipError_t launch_allow_mask(const AllowParams& P, hipStream_t stream);
hipError_t launch_allow_emit(const AllowParams& P, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
