// The bytes inside a match: a forward and a backward automaton over the bytes of every row and a table over the pairs
// of their states (include/tgx_redact.h: tgx_corpus_dfa_cover_device).  The maps, their composition, the constant map
// and the carry operator are dfa.h's; this header has what the two-sided pass adds: the check, the table a call uploads,
// the mirrored place of a backward record and the state a byte reads off the backward side.  The kernels of cover.hip
// and the host twin in host_twins.cpp (tgx_dfa_cover_host) both go through these functions.  DESIGN.md, section L.19.
//
// Two scans.  f_j, the forward state after byte j, is dfa.h's.  g_j, the backward state BEFORE byte j is consumed, is
// the state after every byte to its right in its row.  A backward automaton consumes the rightmost byte first, so the
// map of the bytes [i, last] of a chunk is "the map of [i + 1, last], then byte i's": dfa_compose(right, mine).  A row's
// LAST byte b has the constant map, every nibble next[b][start], which drops whatever lies to its right by the
// arithmetic that drops what precedes a row's first byte in dfa.h.
//
// The mirrored records.  The backward record of chunk k, the map of all its bytes (lane 0's scanned map), is written at
// index n_chunks - 1 - k.  One EXCLUSIVE scan under DfaCarryOp, the operator and the launcher of the forward side
// unchanged, then leaves at that index the map of everything to the right of chunk k, rightmost chunk first.
//
// g of a lane.  It needs the EXCLUSIVE scanned map: that of lane i + 1, or the identity for the chunk's last lane with a
// byte, applied to the carry's image of start.  On a row's last byte g is start outright (the lane to its right belongs
// to another row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfa.h"

namespace tgx {

constexpr int kCoverStages = 3;

// NULL, or what is wrong with the pair of automata (bwd's tag is not looked at)
inline const char* cover_check(uint32_t f_states, uint32_t f_start, const uint8_t (*f_next)[kDfaMaxStates], const uint8_t* f_tag, uint32_t b_states,
                               uint32_t b_start, const uint8_t (*b_next)[kDfaMaxStates]) {
    const uint8_t no_tag[kDfaMaxStates] = {};
    if (const char* why = dfa_check(f_states, f_start, f_next, f_tag)) return why;
    if (dfa_check(b_states, b_start, b_next, no_tag)) return "the backward automaton: n_states, start or an entry of next is out of range";
    return nullptr;
}

// the place of chunk k's backward record and, after the scan, of its carry
__host__ __device__ inline uint64_t cover_mirror(uint64_t k, uint64_t n_chunks) { return n_chunks - 1 - k; }

// g of a lane: right, the scanned backward map of the lane to its right (anything when there is none); chunk_last: the
// lane holds the chunk's last byte; row_last: its row's last byte; carry: the mirrored carry of its chunk.
template <uint32_t NS>
__host__ __device__ inline uint32_t cover_back_state(DfaMap<NS> right, bool chunk_last, bool row_last, DfaMap<NS> carry, uint32_t start) {
    if (row_last) return start;
    return dfa_state<NS>(chunk_last ? dfa_identity<NS>() : right, carry, start);
}

// ---- the table of a call --------------------------------------------------------------------------------------------
// The forward table (kDfaTableWords<NSF> words, dfa.h), the backward one (kDfaTableWords<NSB>, its tags 0), then the
// pair table: 256 bytes, cover[f][g] at 16 f + g, 0 where f or g is no state.
constexpr uint32_t kCoverPairWords = kDfaMaxStates * kDfaMaxStates / 8;
template <uint32_t NSF, uint32_t NSB>
constexpr uint32_t kCoverTableWords = kDfaTableWords<NSF> + kDfaTableWords<NSB> + kCoverPairWords;
template <uint32_t NSF, uint32_t NSB>
inline void cover_build_table(uint32_t f_states, const uint8_t (*f_next)[kDfaMaxStates], const uint8_t* f_tag, uint32_t b_states,
                              const uint8_t (*b_next)[kDfaMaxStates], const uint8_t (*pair)[kDfaMaxStates], uint64_t* words) {
    const uint8_t no_tag[kDfaMaxStates] = {};
    dfa_build_table<NSF>(f_states, f_next, f_tag, words);
    dfa_build_table<NSB>(b_states, b_next, no_tag, words + kDfaTableWords<NSF>);
    uint8_t* p = reinterpret_cast<uint8_t*>(words + kDfaTableWords<NSF> + kDfaTableWords<NSB>);
    for (uint32_t f = 0; f < kDfaMaxStates; f++)
        for (uint32_t g = 0; g < kDfaMaxStates; g++) p[kDfaMaxStates * f + g] = f < f_states && g < b_states ? pair[f][g] : 0;
}
inline uint32_t cover_table_words(uint32_t wf, uint32_t wb) {
    return (wf == 8 ? kDfaTableWords<8> : kDfaTableWords<16>) + (wb == 8 ? kDfaTableWords<8> : kDfaTableWords<16>) + kCoverPairWords;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// cover.hip.  All pointers are device memory; wf and wb are dfa_width of the two sides.  The scans are dfa.hip's
// launch_dfa_scan, one per side.
// rec_f[n_chunks + 1] and rec_b[n_chunks + 1]: the forward records in order and the backward ones mirrored, each with the
// identity behind its last.  table: kCoverTableWords<wf, wb> words.
hipError_t launch_cover_summary(const DedupRows& rows, uint32_t wf, uint32_t wb, uint32_t f_start, uint32_t b_start, const uint64_t* table, void* rec_f,
                                void* rec_b, hipStream_t stream);
// covered i64[S] (may be NULL; pre-set to 0 here) and mask u8[n_bytes] (may be NULL).  table and the carries may be NULL
// when the corpus has no byte.
hipError_t launch_cover(const DedupRows& rows, uint32_t wf, uint32_t wb, uint32_t f_start, uint32_t b_start, const uint64_t* table, const void* carry_f,
                        const void* carry_b, int64_t* covered, uint8_t* mask, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
