// A deterministic automaton of up to 64 states over the bytes of every row of a resident corpus
// (include/tgx_patterns64.h: tgx_corpus_dfa64_hits_device): the check of an automaton, the table a call uploads, the step
// of one state on one byte, the composition of two state maps, the units of the work and the chains that turn maps into
// entry states.  The kernels of dfa64.hip and the host twin in host_twins.cpp (tgx_dfa64_hits_host) both go through
// these functions; the rule of the row sums is textstat_row_inside.  DESIGN.md, section L.21.
//
// The map.  The step of a DFA on byte b is a function from states to states, s -> next[b][s], and so is the run over a
// stretch of bytes.  Here a map is 64 bytes, byte s holding the state reached from s; on the device it is one wave
// register, lane s holding byte s.  `a` then `b` is the map c with c[s] = b[a[s]]: on the device one cross-lane read,
// lane s fetching b from lane a[s].  Composition is associative and not commutative; the identity map, byte s = s, is
// its identity.  A state at or above n_states maps to itself, so every byte of every map is below 64.
//
// Rows need no segmented state.  Every row begins in `start`, so at a row's FIRST byte every run first takes `start`
// and then the byte: the map of that byte is the constant map of dfa.h, which drops whatever precedes the row, in its
// chunk or in the chunks before.  A chunk carries the mask of its row starts, bit j for its byte j.
//
// The units.  The bytes of all rows are laid end to end.  A CHUNK is 64 bytes, a SEGMENT 64 chunks and a GROUP 64
// segments.  The map kernel writes every chunk's map and mask and folds the chunks' maps into their segment's RECORD; a
// chunk past the corpus's end has the identity and an empty mask, so a segment always has 64 maps.  The scan folds the
// segments' records into their group's, chains the groups' records from `start` into every group's entry state, and
// chains every group's segment records from that into every segment's ENTRY state: the exclusive scan of the records
// under composition, of which only the byte at `start` is kept (the corpus's first byte is a row's first byte, so the
// identity in front of segment 0 is harmless).  The replay kernel chains a segment's chunk maps from its entry into
// every chunk's entry and walks each chunk from there, a lane a chunk, storing the tag of every byte's state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"
#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kDfa64MaxStates = 64;  // TGX_DFA64_MAX_STATES
constexpr int kDfa64Stages = 4;
constexpr uint32_t kDfa64Chunk = 64;                                   // bytes: a wave reads it a lane a byte
constexpr uint32_t kDfa64SegChunks = 64;                               // chunks of a segment: the replay's lanes
constexpr uint32_t kDfa64Seg = kDfa64Chunk * kDfa64SegChunks;          // bytes
constexpr uint32_t kDfa64Group = 64;                                   // segments of a group of the scan
constexpr uint32_t kDfa64Map = kDfa64MaxStates;                        // bytes of a map
constexpr uint32_t kDfa64TableBytes = 256 * kDfa64MaxStates + kDfa64MaxStates;  // next as 256 rows of 64 bytes, then the tags
constexpr uint32_t kDfa64TableWords = kDfa64TableBytes / 8;
constexpr uint32_t kDfa64BlockWaves = 4;
constexpr uint32_t kDfa64MinRun = 4;  // segments a wave takes at least, so that a block's copy of the table serves 64 KiB of text
static_assert(kDfa64Chunk == kTextstatChunk, "the count kernel reads the tags on textstat_walk's chunks");

// ---- the automaton's check ------------------------------------------------------------------------------------------
// next: u8[256][64], tag: u8[64] (the fields of tgx_dfa64).  NULL, or what is wrong with it.
inline const char* dfa64_check(uint32_t n_states, uint32_t start, const uint8_t (*next)[kDfa64MaxStates], const uint8_t* tag) {
    if (n_states < 1 || n_states > kDfa64MaxStates) return "n_states is outside 1 .. 64";
    if (start >= n_states) return "start is no state";
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t s = 0; s < n_states; s++)
            if (next[b][s] >= n_states) return "an entry of next is no state";
    if (tag[start] != 0) return "tag[start] is not 0: the pattern matches the empty string";
    return nullptr;
}

// ---- the table of a call --------------------------------------------------------------------------------------------
// kDfa64TableBytes bytes: next[b][s] at b * 64 + s, a state at or above n_states its own successor, then the 64 tags.  A
// block copies them into LDS in this layout.
inline void dfa64_build_table(uint32_t n_states, const uint8_t (*next)[kDfa64MaxStates], const uint8_t* tag, uint8_t* table) {
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t s = 0; s < kDfa64MaxStates; s++) table[b * kDfa64MaxStates + s] = s < n_states ? next[b][s] : (uint8_t)s;
    for (uint32_t s = 0; s < kDfa64MaxStates; s++) table[256 * kDfa64MaxStates + s] = s < n_states ? tag[s] : 0;
}

// ---- steps and maps -------------------------------------------------------------------------------------------------
// the state after byte b in state s; b64 = b * 64, which the map kernel shifts once per lane
__host__ __device__ inline uint32_t dfa64_step_at(const uint8_t* next, uint32_t b64, uint32_t s) { return next[b64 + s]; }
// the same at a byte that may be its row's first: every run takes `start` there first
__host__ __device__ inline uint32_t dfa64_step(const uint8_t* next, uint32_t s, uint32_t b, bool row_first, uint32_t start) {
    return dfa64_step_at(next, b * kDfa64MaxStates, row_first ? start : s);
}
// acc = `acc` then `m`, both maps of 64 bytes (the device: dfa64_then in dfa64.hip, one cross-lane read)
inline void dfa64_fold(uint8_t* acc, const uint8_t* m) {
    for (uint32_t s = 0; s < kDfa64Map; s++) acc[s] = m[acc[s]];
}
inline void dfa64_identity(uint8_t* m) {
    for (uint32_t s = 0; s < kDfa64Map; s++) m[s] = (uint8_t)s;
}
// entry[k] = the state in front of map k of n consecutive maps, e the state in front of the first; -> the state behind
// the last (the device: dfa64_chain in dfa64.hip, 64 dependent lane reads)
inline uint32_t dfa64_chain_host(const uint8_t* maps, uint64_t n, uint32_t e, uint8_t* entry) {
    for (uint64_t k = 0; k < n; k++) {
        entry[k] = (uint8_t)e;
        e = maps[k * kDfa64Map + e];
    }
    return e;
}

// ---- the units ------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t dfa64_segs(uint64_t n_bytes) { return (n_bytes + kDfa64Seg - 1) / kDfa64Seg; }
__host__ __device__ inline uint64_t dfa64_groups(uint64_t n_segs) { return (n_segs + kDfa64Group - 1) / kDfa64Group; }
// the bytes of the chunk at c0 (0 past the corpus's end)
__host__ __device__ inline uint32_t dfa64_chunk_bytes(uint64_t c0, uint64_t n_bytes) {
    return c0 >= n_bytes ? 0u : (n_bytes - c0 < kDfa64Chunk ? (uint32_t)(n_bytes - c0) : kDfa64Chunk);
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// the blocks of the map and replay kernels: a wave takes a run of consecutive segments, kDfa64MinRun at least
inline uint32_t dfa64_grid(uint64_t n_segs, uint64_t cap) { return grid_for(n_segs, (uint64_t)kDfa64BlockWaves * kDfa64MinRun, cap); }

// dfa64.hip.  All pointers are device memory; a corpus of N bytes has n_segs = dfa64_segs(N) segments.
// cmap u8[n_segs * 4096]: the chunks' maps; cmask u64[n_segs * 64]: their row-start masks; srec u8[n_segs * 64]: the
// segments' records.  table: kDfa64TableBytes bytes, 16-byte aligned.
hipError_t launch_dfa64_map(const DedupRows& rows, uint32_t start, const uint8_t* table, uint8_t* cmap, uint64_t* cmask, uint8_t* srec, hipStream_t stream);
// sentry u8[n_segs]: every segment's entry state.  grec u8[n_groups * 64] and gentry u8[n_groups] are the scan's own.
hipError_t launch_dfa64_scan(uint32_t start, const uint8_t* srec, uint64_t n_segs, uint8_t* grec, uint8_t* gentry, uint8_t* sentry, hipStream_t stream);
// tags u8[N]: the tag of the state after every byte
hipError_t launch_dfa64_replay(const DedupRows& rows, uint32_t start, const uint8_t* table, const uint8_t* cmap, const uint64_t* cmask, const uint8_t* sentry,
                               uint8_t* tags, hipStream_t stream);
// count i64[S], pre-set to 0 here: per row its bytes with a non-zero tag.  tags may be NULL when the corpus has no byte.
hipError_t launch_dfa64_count(const DedupRows& rows, const uint8_t* tags, int64_t* count, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
