// Repeated n-grams within a row (include/tgx.h: tgx_*_repeat_stats_device, tgx_repeat_stats_host): the row key, the
// flag of a sorted slot, the end of a run, the coverage window and the table's layout.  The kernels of repeat.hip and
// the host twin in host_twins.cpp (tgx_repeat_stats_host) both go through these functions; DESIGN.md, section L.14.
//
// The source, the width w, the validity of the gram at element e (gram_valid) and its key(e) (tgx_gram_key of its bytes
// under the seed: gram_walk's loaders and minhash_hash_words) are those of gram.h.  The ROW KEY of a valid gram at
// element e of row i is
//     rkey(e) = dedup_mix(key(e) ^ ((i + 1) · 0x9E3779B97F4A7C15)).
// dedup_mix is a bijection, so for a fixed row rkey is a bijection of key: within a row two grams are EQUAL iff their
// keys are equal, which is probabilistic by the 64-bit key exactly in the sense of gram_hits (different grams may share
// a key; equal keys are not verified against the elements).  Across rows equal grams get different row keys, except by
// a 64-bit collision, so one global sort of the row keys groups every row's grams by themselves.
//
// An OCCURRENCE CLASS is the set of the valid grams of one row with one row key; its first member by position is its
// FIRST occurrence, every other member a REPEAT, and a class of two or more members is MULTI.  The sort of (rkey,
// position) pairs is rocPRIM's radix sort, which is STABLE, and the pairs go in by ascending position: the positions
// inside a class ascend after the sort and the class's first slot is its first occurrence.  This is relied on.
//
// Scratch of a call over G valid grams, n elements and S rows: 24 bytes per gram (two u64 key buffers and two u32
// position buffers, the sort's two sides), 1 byte per element (the flags, unless the caller's mask takes them), 8 (S + 1)
// bytes (g_offs) and rocPRIM's temporaries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram.h"

namespace tgx {

constexpr uint32_t kRepeatN = 6;  // the table's statistics, each i64[S]
enum RepeatStat : uint32_t { kRpGrams = 0, kRpRepeated = 1, kRpMulti = 2, kRpTop = 3, kRpCovered = 4, kRpCoveredAll = 5 };
constexpr uint8_t kRepeatBitRepeat = 1;  // mask bit 0: a repeat begins here
constexpr uint8_t kRepeatBitMulti = 2;   // mask bit 1: a member of a MULTI class begins here
constexpr uint64_t kRepeatMaxElems = 0xFFFFFFFEull;  // positions are u32 and 2^32 - 1 elements are refused
constexpr int kRepeatStages = 4;
static_assert(kMinhashMaxBytes <= kGramChunk, "a gram is at most one chunk wide: the chunk before suffices for the coverage window");

__host__ __device__ inline uint64_t repeat_row_key(uint64_t key, uint64_t row) { return dedup_mix(key ^ ((row + 1) * 0x9E3779B97F4A7C15ULL)); }

// The flag of the gram in sorted slot t: head = t is the first slot of its run of equal row keys, next_same = slot t + 1
// holds the same row key.  Bit 0: not a head, so a repeat.  Bit 1: a repeat, or a head that is followed: its class is MULTI.
__host__ __device__ inline uint8_t repeat_flag(bool head, bool next_same) {
    return (uint8_t)((head ? 0 : kRepeatBitRepeat) | ((!head || next_same) ? kRepeatBitMulti : 0));
}

// The end (one past the last slot) of the run of equal keys that begins at slot t < n of the ascending keys: a gallop
// and then a binary search, so a row of one repeated element, a single run of its whole length, costs its logarithm.
__host__ __device__ inline uint64_t repeat_run_end(const uint64_t* keys, uint64_t n, uint64_t t) {
    const uint64_t k = keys[t];
    uint64_t lo = t, step = 1;  // keys[lo] == k
    while (lo + step < n && keys[lo + step] == k) {
        lo += step;
        step *= 2;
    }
    uint64_t hi = lo + step < n ? lo + step : n;  // keys[hi] != k, or hi == n
    while (lo + 1 < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] == k)
            lo = mid;
        else
            hi = mid;
    }
    return hi;
}

// top[row] before the runs: a row with a gram has a class of one member
__host__ __device__ inline uint64_t repeat_top_preset(uint64_t grams) { return grams < 1 ? grams : 1; }

// The coverage rule.  before / here: one bit per element of the chunk before the lane's and of its own chunk (bit l:
// the flagged gram that begins at element c0 - 64 + l, c0 + l).  Element e = c0 + lane of a row that starts at rs is
// covered iff a bit is set at some p in [max(rs, e - w + 1), e].  w <= 64, so the window is the chunk before at most.
// Two shifts bring the 64 positions that end at e into one word (bit 63 = e), a third keeps the last `back` + 1 of them.
// The cut at rs states the rule "a gram covers elements of its own row only" where it is applied, and is a guard, not a
// correction: a flagged gram is VALID, so p + w <= its row's end <= rs for every flagged p of an earlier row, and such a
// p lies in front of e - w + 1 for every e >= rs.  With flags that repeat_runs_kernel wrote, the cut never changes the
// answer (dropping it in the twin fails no test); with a flag array that broke the validity rule it would.
__host__ __device__ inline bool repeat_covered(uint64_t before, uint64_t here, uint32_t lane, uint64_t e, uint64_t rs, uint32_t w) {
    const uint64_t ending = lane == 63 ? here : (before >> (lane + 1)) | (here << (63 - lane));
    const uint64_t back = e - rs < w - 1 ? e - rs : w - 1;  // elements before e that the window takes: <= 63
    return (ending >> (63 - back)) != 0;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// repeat.hip.  All pointers are device memory.
// the room that the sort of n (key, position) pairs needs
hipError_t repeat_sort_bytes(uint64_t n, size_t* sort_bytes);
// keys_out[g_offs[i] + t] = the row key of gram t of row i, pos_out[the same] = its global element
hipError_t launch_repeat_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, uint32_t* pos_out,
                              hipStream_t stream);
// (keys_in, pos_in) sorted stably by key into (keys_out, pos_out)
hipError_t launch_repeat_sort(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* pos_in, uint32_t* pos_out, uint64_t n, void* sort_tmp,
                              size_t sort_bytes, hipStream_t stream);
// The pre-sets: flag u8[n_elems] = 0, and with a table stats[kRpGrams] = the rows' gram counts, stats[kRpTop] =
// repeat_top_preset of them, the other four 0.  stats may be NULL.
hipError_t launch_repeat_preset(const DedupRows& rows, uint32_t width, int64_t* stats, uint8_t* flag, hipStream_t stream);
// flag[pos[t]] of every sorted slot; with a table the length of every MULTI class maxed onto stats[kRpTop]
hipError_t launch_repeat_runs(const DedupRows& rows, const uint64_t* keys, const uint32_t* pos, uint64_t n, uint8_t* flag, int64_t* stats,
                              hipStream_t stream);
// stats[kRpRepeated], [kRpMulti], [kRpCovered], [kRpCoveredAll] of every row from the flags
hipError_t launch_repeat_cover(const DedupRows& rows, uint32_t width, const uint8_t* flag, int64_t* stats, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
