// Duplicate spans across rows (include/tgx_dupspans.h: tgx_*_dup_spans_device, tgx_dup_spans_host): the masked key, the
// rule by which a sorted slot is a duplicate, the table's layout and the mask's bits.  The kernels of dupspan.hip and the
// host twin in host_twins.cpp (tgx_dup_spans_host) both go through these functions; DESIGN.md, section L.25.
//
// The source, the width w, the validity of the gram at element e (gram_valid) and its key(e) are those of gram.h; the
// elements of all rows are numbered end to end.  The valid gram at element e is a DUPLICATE iff some valid gram at an
// element e' < e, of any row, has the same w elements.  Equality is of the ELEMENTS, compared: the key only brings the
// candidates together, so the answer does not depend on it, and the sort may look at its low key_bits bits alone
// (1 .. 64).  Element e of row i is COVERED iff it lies inside a duplicate gram, which lies inside row i as every valid
// gram does.
//
// The sort of (key, position) pairs is rocPRIM's radix sort over the bits [0, key_bits), which is STABLE, and the pairs
// go in by ascending position: the positions inside a run of equal masked keys ascend after the sort.  This is relied
// on.  Equal elements have equal keys, hence equal masked keys, hence one run; an earlier position is then an earlier
// slot of that run: walking back from a slot to the head of its run meets every earlier gram that can be equal to it.
//
// Scratch of a call over G valid grams, n elements and S rows: 24 bytes per gram (two u64 key buffers and two u32
// position buffers, the sort's two sides), 1 byte per element (the flags, unless the caller's mask takes them), 8 (S + 1)
// bytes (g_offs) and rocPRIM's temporaries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram.h"
#include "repeat.h"  // repeat_covered: the coverage window, here over the one bit

namespace tgx {

constexpr uint32_t kDupspanN = 3;  // the table's statistics, each i64[S]
enum DupspanStat : uint32_t { kDsGrams = 0, kDsDup = 1, kDsCovered = 2 };
constexpr uint8_t kDupspanBitDup = 1;      // mask bit 0: a duplicate gram begins here
constexpr uint8_t kDupspanBitCovered = 2;  // mask bit 1: the element lies inside a duplicate gram
constexpr uint64_t kDupspanMaxElems = kRepeatMaxElems;  // positions are u32 and 2^32 - 1 elements are refused
constexpr int kDupspanStages = 4;

// the bits of the key that the sort looks at, 1 <= key_bits <= 64
__host__ __device__ inline uint64_t dupspan_key_mask(uint32_t key_bits) { return key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1; }

// The rule by which the gram in sorted slot t is a duplicate, in two steps that the kernel and the twin both take.  key
// is slot t's, prev_key and prev_pos are slot t - 1's (the kernel has them from the lane below, the twin from memory;
// prev_key is not looked at when t == 0).  A slot whose predecessor's masked key differs is the head of its run, not a
// CANDIDATE, and compares nothing.
__host__ __device__ inline bool dupspan_candidate(uint64_t t, uint64_t key, uint64_t prev_key, uint64_t key_mask) {
    return t > 0 && ((prev_key ^ key) & key_mask) == 0;
}
// For a candidate only: equal_to_mine(p) compares the w elements at p with slot t's own.  The predecessor is compared
// first, and on a mismatch the walk goes back slot by slot while the masked key stays that of slot t: it stops at the
// first equal gram (a duplicate) or at the run's head (not one).  A run of true duplicates costs each slot one
// comparison; a run that mixes different grams costs a slot up to the run's length, so the pass is quadratic in such a
// run: key_bits far below log2 of the gram count are for tests of small sources only.
template <class Equal>
__host__ __device__ inline bool dupspan_walk_back(const uint64_t* keys, const uint32_t* pos, uint64_t t, uint64_t key, uint64_t key_mask,
                                                  uint32_t prev_pos, Equal equal_to_mine) {
    if (equal_to_mine(prev_pos)) return true;
    for (uint64_t s = t - 1; s > 0 && ((keys[s - 1] ^ key) & key_mask) == 0; s--)
        if (equal_to_mine(pos[s - 1])) return true;
    return false;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// dupspan.hip.  All pointers are device memory.
// the room that the sort of n (key, position) pairs over key_bits bits needs
hipError_t dupspan_sort_bytes(uint64_t n, uint32_t key_bits, size_t* sort_bytes);
// The pre-sets: flag u8[n_elems] = 0, and with a table table[kDsGrams] = the rows' gram counts, the other two 0.
hipError_t launch_dupspan_preset(const DedupRows& rows, uint32_t width, int64_t* table, uint8_t* flag, hipStream_t stream);
// keys_out[g_offs[i] + t] = the key of gram t of row i (no row mix), pos_out[the same] = its global element
hipError_t launch_dupspan_keys(const DedupRows& rows, uint32_t width, uint64_t seed, const uint64_t* g_offs, uint64_t* keys_out, uint32_t* pos_out,
                               hipStream_t stream);
// (keys_in, pos_in) sorted stably by the low key_bits bits of the key into (keys_out, pos_out)
hipError_t launch_dupspan_sort(const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* pos_in, uint32_t* pos_out, uint64_t n, uint32_t key_bits,
                               void* sort_tmp, size_t sort_bytes, hipStream_t stream);
// flag[pos[t]] = kDupspanBitDup for every candidate slot t whose walk back finds an equal gram (the pre-set left the rest 0)
hipError_t launch_dupspan_match(const DedupRows& rows, uint32_t width, const uint64_t* keys, const uint32_t* pos, uint64_t n, uint32_t key_bits,
                                uint8_t* flag, hipStream_t stream);
// table[kDsDup] and [kDsCovered] of every row from the flags (table may be NULL), and with finish_mask kDupspanBitCovered
// OR-ed into flag[e] of every covered element
hipError_t launch_dupspan_cover(const DedupRows& rows, uint32_t width, uint8_t* flag, bool finish_mask, int64_t* table, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
