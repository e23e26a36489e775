// Leftmost-first, non-overlapping matches of an automaton over the bytes of every row of a resident corpus, and the most
// frequent distinct matches (include/tgx_find.h: tgx_corpus_find_device, tgx_corpus_mine_device): the table a call
// uploads, the step of one walk, the byte a walk leaves per position, the chunk's skip map by pointer doubling, the
// visited set of a chunk and the order rule of the mined entries.  The kernels of find.hip and the host twins in
// host_twins.cpp (tgx_find_host, tgx_mine_host) both go through these functions; the maps' fold, scan and chain are
// dfa64.h's, the rule of the row sums is textstat_row_inside.  DESIGN.md, section L.23.
//
// The walk.  From a start byte a the automaton runs from `start` over at most `limit` = min(max_len, row_end - a) bytes
// and stops early in a dead state (one from which no tagged state is reachable).  len(a) is the last t + 1 at which the
// state was tagged, trunc(a) says that the walk ran into max_len inside its row while still live.  A position's WALK BYTE
// holds len in its low 7 bits and trunc in bit 7.
//
// The table.  16 384 bytes: entry b * 64 + s is the state t = next[b][s] in its low 6 bits, bit 6 set when t is tagged
// and bit 7 when t is dead, so a step is one lookup.  A state at or above n_states is dead.
//
// The chain.  The successor of position p is p + max(len(p), 1).  With the bytes of all rows laid end to end in dfa64.h's
// chunks of 64, the chain's state at a chunk's first byte is the SKIP, the bytes of a match that began before the chunk
// and still lie in it: 0 .. 63, because a match has at most 64 bytes.  No match crosses a row's end, so a row's first
// byte is always reached with skip 0 and rows need no segmented state.  A chunk's MAP is E[r], the skip that leaves the
// chunk entered with skip r: lane j holds its successor j + step, 1 .. 127, and six rounds of pointer doubling (a lane
// below 64 takes the pointer of the lane it points to) bring every lane past 63; E[r] is lane r's pointer less 64.  Maps
// have dfa64.h's form, 64 bytes below 64, and compose the same way, so the segments' records are scanned by
// launch_dfa64_scan from skip 0.  The replay doubles again, now with the set of lanes passed on the way (a 64-bit mask
// per lane, or-ed under the same reads), and the set of the lane at the entry skip is the chunk's VISITED set.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfa64.h"

namespace tgx {

constexpr uint32_t kFindMaxLen = 64;  // TGX_FIND_MAX_LEN
constexpr int kFindStages = 6;        // walk, scan, replay; the mine's compaction and keys, sort and runs, order
constexpr uint32_t kFindTableBytes = 256 * kDfa64MaxStates;
constexpr uint32_t kFindTableWords = kFindTableBytes / 8;
constexpr uint32_t kFindTagged = 64u, kFindDead = 128u;  // bits of a table entry
constexpr uint32_t kFindTrunc = 128u;                      // bit of a walk byte
constexpr uint32_t kFindDoublings = 6;                     // 2^6 hops of at least one byte leave a chunk
static_assert(kFindMaxLen == kDfa64Chunk && kFindMaxLen < kFindTrunc, "a skip is below a chunk's bytes and a length fits beside the trunc bit");

// ---- the table of a call --------------------------------------------------------------------------------------------
// the states from which no tagged state is reachable, as a mask (states at or above n_states included)
inline uint64_t find_dead_mask(uint32_t n_states, const uint8_t (*next)[kDfa64MaxStates], const uint8_t* tag) {
    uint64_t live = 0;
    for (uint32_t s = 0; s < n_states; s++)
        if (tag[s]) live |= 1ull << s;
    for (bool grown = true; grown;) {
        grown = false;
        for (uint32_t s = 0; s < n_states; s++) {
            if ((live >> s) & 1ull) continue;
            for (uint32_t b = 0; b < 256; b++)
                if ((live >> next[b][s]) & 1ull) {
                    live |= 1ull << s;
                    grown = true;
                    break;
                }
        }
    }
    return ~live;
}
inline void find_build_table(uint32_t n_states, const uint8_t (*next)[kDfa64MaxStates], const uint8_t* tag, uint8_t* table) {
    const uint64_t dead = find_dead_mask(n_states, next, tag);
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t s = 0; s < kDfa64MaxStates; s++) {
            const uint32_t t = s < n_states ? next[b][s] : s;
            table[b * kDfa64MaxStates + s] = (uint8_t)(t | (t < n_states && tag[t] ? kFindTagged : 0u) | (((dead >> t) & 1ull) ? kFindDead : 0u));
        }
}
inline const char* find_check_max_len(uint32_t max_len) { return max_len < 1 || max_len > kFindMaxLen ? "max_len is outside 1 .. 64" : nullptr; }

// ---- the walk -------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t find_limit(uint64_t pos, uint64_t row_end, uint32_t max_len) {
    return row_end - pos < max_len ? (uint32_t)(row_end - pos) : max_len;
}
// One byte of a live walk: byte b is its byte t.  q, len and live are the walk's; -> false once it has stopped.
__host__ __device__ inline bool find_advance(const uint8_t* table, uint32_t b, uint32_t t, uint32_t& q, uint32_t& len) {
    const uint32_t e = table[b * kDfa64MaxStates + q];
    q = e & 63u;
    if (e & kFindDead) return false;
    if (e & kFindTagged) len = t + 1;
    return true;
}
// the walk byte of a walk that stopped after t bytes: still_live, it ran out of its limit and not into a dead state
__host__ __device__ inline uint32_t find_walk_byte(uint32_t len, bool still_live, uint32_t t, uint32_t max_len, uint64_t pos, uint64_t row_end) {
    return len | (still_live && t == max_len && pos + t < row_end ? kFindTrunc : 0u);
}
__host__ __device__ inline uint32_t find_len(uint32_t walk_byte) { return walk_byte & (kFindTrunc - 1u); }
__host__ __device__ inline uint32_t find_hop(uint32_t walk_byte) { return find_len(walk_byte) ? find_len(walk_byte) : 1u; }

// the whole walk from pos on host memory (the kernel runs the same steps a lane a start, in lockstep)
inline uint32_t find_walk_host(const uint8_t* table, uint32_t start, const uint8_t* text, uint64_t pos, uint64_t row_end, uint32_t max_len) {
    const uint32_t limit = find_limit(pos, row_end, max_len);
    uint32_t q = start, len = 0, t = 0;
    bool live = true;
    while (live && t < limit) {
        live = find_advance(table, text[pos + t], t, q, len);
        t++;
    }
    return find_walk_byte(len, live, t, max_len, pos, row_end);
}

// ---- the chunk's map and visited set --------------------------------------------------------------------------------
// One round of the doubling on a chunk's 64 pointers (and sets, when reach != NULL): the device does it with one
// cross-lane read per word, every lane at once, so the host reads a copy of the round's input.
inline void find_double_host(uint32_t* ptr, uint64_t* reach) {
    uint32_t p0[kDfa64Chunk];
    uint64_t r0[kDfa64Chunk];
    for (uint32_t j = 0; j < kDfa64Chunk; j++) {
        p0[j] = ptr[j];
        r0[j] = reach ? reach[j] : 0;
    }
    for (uint32_t j = 0; j < kDfa64Chunk; j++)
        if (p0[j] < kDfa64Chunk) {
            ptr[j] = p0[p0[j]];
            if (reach) reach[j] = r0[j] | r0[p0[j]];
        }
}
// walk: the n_in walk bytes of a chunk (a position past the corpus's end hops one byte).  map: E[r], 64 bytes; visited
// (may be NULL): the set of the lanes passed from the entry skip e on.
inline void find_chunk_host(const uint8_t* walk, uint32_t n_in, uint32_t e, uint8_t* map, uint64_t* visited) {
    uint32_t ptr[kDfa64Chunk];
    uint64_t reach[kDfa64Chunk];
    for (uint32_t j = 0; j < kDfa64Chunk; j++) {
        ptr[j] = j + (j < n_in ? find_hop(walk[j]) : 1u);
        reach[j] = 1ull << j;
    }
    for (uint32_t k = 0; k < kFindDoublings; k++) find_double_host(ptr, visited ? reach : nullptr);
    for (uint32_t j = 0; j < kDfa64Chunk; j++) map[j] = (uint8_t)(ptr[j] - kDfa64Chunk);
    if (visited) *visited = reach[e];
}

// ---- the order of the mined entries ---------------------------------------------------------------------------------
// count descending, then first position ascending: does entry a go before entry b?
__host__ __device__ inline bool find_before(uint64_t count_a, uint64_t pos_a, uint64_t count_b, uint64_t pos_b) {
    return count_a != count_b ? count_a > count_b : pos_a < pos_b;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// find.hip.  All pointers are device memory; a corpus of N bytes has n_segs = dfa64_segs(N) segments.
// walk u8[N]: every position's walk byte; srec u8[n_segs * 64]: the segments' records.  table: kFindTableBytes bytes,
// 16-byte aligned.
hipError_t launch_find_walk(const DedupRows& rows, uint32_t start, uint32_t max_len, const uint8_t* table, uint8_t* walk, uint8_t* srec, hipStream_t stream);
// sentry u8[n_segs]: every segment's entry skip (launch_dfa64_scan from 0).  lens u8[N], count i64[S] and truncated
// i64[S] may each be NULL; the counts are pre-set to 0 here.  lens may be walk itself.
hipError_t launch_find_replay(const DedupRows& rows, const uint8_t* walk, const uint8_t* sentry, uint8_t* lens, int64_t* count, int64_t* truncated,
                              hipStream_t stream);
// the mine: keys[i] = tgx_gram_key of the lens[pos[i]] bytes at pos[i] under seed, of n matches
hipError_t launch_find_keys(const uint8_t* text, const uint8_t* lens, const uint64_t* pos, uint64_t n, uint64_t seed, uint64_t* keys, hipStream_t stream);
// the room of the sorts of n pairs
hipError_t find_sort_bytes(uint64_t n, size_t* bytes);
// (keys, pos) sorted stably by key into (keys_out, pos_out)
hipError_t launch_find_sort(const uint64_t* keys, uint64_t* keys_out, const uint64_t* pos, uint64_t* pos_out, uint64_t n, void* tmp, size_t bytes,
                            hipStream_t stream);
// heads[i] = 1 where sorted key i begins a run
hipError_t launch_find_heads(const uint64_t* keys, uint64_t n, uint8_t* heads, hipStream_t stream);
// run r begins at sorted index head[r]: run_pos[r] = pos[head[r]], its first position, and run_count[r] its length
hipError_t launch_find_runs(const uint64_t* head, uint64_t n_runs, uint64_t n, const uint64_t* pos, uint64_t* run_pos, uint64_t* run_count, hipStream_t stream);
// (run_pos, run_count) into the order of find_before: by position ascending into (pos_tmp, count_tmp), then stably by
// count descending back into (run_pos, run_count)
hipError_t launch_find_order(uint64_t* run_pos, uint64_t* run_count, uint64_t* pos_tmp, uint64_t* count_tmp, uint64_t n_runs, void* tmp, size_t bytes,
                             hipStream_t stream);
// out[3 * i ..] = (run_pos[i], lens[run_pos[i]], run_count[i]) of the first n_top entries
hipError_t launch_find_top(const uint64_t* run_pos, const uint64_t* run_count, const uint8_t* lens, uint64_t n_top, uint64_t* out, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
