// Fixed-length sequences of byte classes over the bytes of every row of a resident corpus (include/tgx_shapes.h:
// tgx_corpus_shape_hits_device, tgx_corpus_shape_cover_device): the check of the shapes, the word of position bits, the
// table a call uploads, the doubling step of the window, the ends a byte's word gives and the window of the cover.  The
// kernels of shape.hip and the host twins in host_twins.cpp (tgx_shape_hits_host, tgx_shape_cover_host) both go through
// these functions; the tiling and the masks over a chunk's lanes are textstat.h's, and the rule of the row sums is
// textstat_row_inside.  DESIGN.md, section L.20.
//
// The word.  The patterns are laid end to end and position q of the concatenation is bit q of a word of NW uint64_t:
// NW = 1 when the lengths sum to at most 64, else 2.  A pattern may straddle the two halves.  off(q) is q's offset inside
// its pattern.
//
// The window.  W_1(j) = B[text[j]], the positions that byte j fits.  A step doubles the window:
//     W_2d(j) = W_d(j) & ((W_d(j - d) << d) | Z_d),      d = 1, 2, 4, 8, 16, 32,
// Z_d being the bits q with off(q) < d.  By induction bit q of W_D(j) says that the bytes j - min(off(q), D - 1) .. j fit
// the positions that end at q: where off(q) < d the bit is complete and Z_d keeps it, and elsewhere bit q - d, which
// belongs to the same pattern, brings the d bytes before.  The bit shifted out of a pattern's last position lands on the
// next pattern's first, where every Z_d is 1, so packing needs no other care.  W_64 is Shift-And's state D_j with no
// state older than 63 bytes: a chunk needs the chunk in front of it, the HALO, and nothing else.  A position before the
// corpus's first byte contributes 0 before the OR.
//
// Rows.  D(j) = W_64(j) & ROWOK[min(j - row_begin, 63)], ROWOK[t] being the bits with off(q) <= t: a bit that reaches
// back over its row's first byte is cleared, and the bytes of other rows in the window only ever feed such bits.
//
// Ends.  Bit k of a byte's ends is D(j) at pattern k's last position, less the guards: the before-guard clears it when
// j - row_begin >= len[k] and the byte at j - len[k] is in not_before[k], the after-guard when j + 1 < row_end and the
// byte at j + 1 is in not_after[k].  NB[c] and NA[c] hold bit k for a byte c in pattern k's guard.
//
// Cover.  Byte i lies inside a match of k iff some end of k lies in i .. i + len[k] - 1.  An end in a later row cannot:
// its start would be at or before i.  So a lane reads the window off the ballots of its own and the next chunk's ends.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"

namespace tgx {

constexpr uint32_t kShapesMaxPatterns = 8;  // TGX_SHAPES_MAX_PATTERNS
constexpr uint32_t kShapeMaxLen = 64;       // TGX_SHAPE_MAX_LEN
constexpr uint32_t kShapesMaxBits = 128;    // TGX_SHAPES_MAX_BITS
constexpr uint32_t kShapeSteps = 6;         // d = 1 .. 32
constexpr int kShapeStages = 2;
static_assert(kShapeMaxLen == kTextstatChunk, "the halo is one chunk: no state is older than 63 bytes");

// ---- the shapes' check ----------------------------------------------------------------------------------------------
// len: u32[8], cls: u8[128][32] (the fields of tgx_shapes).  byte b of a set
__host__ __device__ inline bool shape_has(const uint8_t* set, uint32_t b) { return (set[b >> 3] >> (b & 7u)) & 1u; }
// NULL, or what is wrong with them
inline const char* shape_check(uint32_t n_patterns, const uint32_t* len, const uint8_t (*cls)[32]) {
    if (n_patterns < 1 || n_patterns > kShapesMaxPatterns) return "n_patterns is outside 1 .. 8";
    uint32_t total = 0;
    for (uint32_t k = 0; k < n_patterns; k++) {
        if (len[k] < 1 || len[k] > kShapeMaxLen) return "a len is outside 1 .. 64";
        total += len[k];
    }
    if (total > kShapesMaxBits) return "the lengths sum to more than 128";
    for (uint32_t q = 0; q < total; q++) {
        bool any = false;
        for (uint32_t i = 0; i < 32; i++) any = any || cls[q][i] != 0;
        if (!any) return "a class at a used position is empty";
    }
    return nullptr;
}
inline uint32_t shape_total(uint32_t n_patterns, const uint32_t* len) {
    uint32_t total = 0;
    for (uint32_t k = 0; k < n_patterns; k++) total += len[k];
    return total;
}
// the instantiation that serves the shapes: the words of 64 bits
inline uint32_t shape_nw(uint32_t total) { return total <= 64 ? 1u : 2u; }

// ---- words ----------------------------------------------------------------------------------------------------------
template <uint32_t NW>
struct ShapeWord {
    uint64_t w[NW];
};
template <uint32_t NW>
__host__ __device__ inline ShapeWord<NW> shape_zero() {
    ShapeWord<NW> r;
    for (uint32_t i = 0; i < NW; i++) r.w[i] = 0;
    return r;
}
template <uint32_t NW>
__host__ __device__ inline ShapeWord<NW> shape_and(const ShapeWord<NW>& a, const ShapeWord<NW>& b) {
    ShapeWord<NW> r;
    for (uint32_t i = 0; i < NW; i++) r.w[i] = a.w[i] & b.w[i];
    return r;
}
// a << d, 1 <= d <= 32; the bits of the low half cross into the high one
template <uint32_t NW>
__host__ __device__ inline ShapeWord<NW> shape_shl(const ShapeWord<NW>& a, uint32_t d) {
    ShapeWord<NW> r;
    r.w[0] = a.w[0] << d;
    if (NW == 2) r.w[NW - 1] = (a.w[NW - 1] << d) | (a.w[0] >> (64u - d));
    return r;
}
// one doubling step: W_2d(j) of W_d(j) = mine, W_d(j - d) = from and Z_d = z
template <uint32_t NW>
__host__ __device__ inline ShapeWord<NW> shape_step(const ShapeWord<NW>& mine, const ShapeWord<NW>& from, uint32_t d, const ShapeWord<NW>& z) {
    const ShapeWord<NW> s = shape_shl<NW>(from, d);
    ShapeWord<NW> r;
    for (uint32_t i = 0; i < NW; i++) r.w[i] = mine.w[i] & (s.w[i] | z.w[i]);
    return r;
}

// ---- the table of a call --------------------------------------------------------------------------------------------
// A block copies it into LDS word by word in this layout: 2 KiB + 1 112 bytes at NW = 1, 4 KiB + 1 688 bytes at NW = 2.
template <uint32_t NW>
struct ShapeTable {
    ShapeWord<NW> b[256];                  // B[c]: bit q says that c is in cls[q]
    ShapeWord<NW> rowok[kShapeMaxLen];     // ROWOK[t]: the bits with off(q) <= t
    ShapeWord<NW> z[8];                    // Z_d at log2 d, six in use: the bits with off(q) < d
    uint8_t nb[256], na[256];              // bit k: the byte is in pattern k's not_before / not_after
    uint8_t last[kShapesMaxPatterns];      // pattern k's last position
    uint8_t len[kShapesMaxPatterns];       // 1 .. 64
    uint32_t n_patterns;
    uint32_t nb_used;                      // bit k: pattern k has a before-guard
};
template <uint32_t NW>
constexpr uint32_t kShapeTableWords = sizeof(ShapeTable<NW>) / 8;
static_assert(sizeof(ShapeTable<1>) % 8 == 0 && sizeof(ShapeTable<2>) % 8 == 0, "copied as 8-byte words");

// len, cls, not_before, not_after: the fields of tgx_shapes, checked.  words: kShapeTableWords<NW> of them.
template <uint32_t NW>
inline void shape_build_table(uint32_t n_patterns, const uint32_t* len, const uint8_t (*cls)[32], const uint8_t (*not_before)[32],
                              const uint8_t (*not_after)[32], uint64_t* words) {
    for (uint32_t i = 0; i < kShapeTableWords<NW>; i++) words[i] = 0;
    ShapeTable<NW>& t = *reinterpret_cast<ShapeTable<NW>*>(words);
    t.n_patterns = n_patterns;
    uint32_t q = 0;
    for (uint32_t k = 0; k < n_patterns; k++) {
        for (uint32_t off = 0; off < len[k]; off++, q++) {
            const uint64_t bit = 1ull << (q & 63u);
            const uint32_t h = NW == 2 ? q >> 6 : 0;
            for (uint32_t c = 0; c < 256; c++)
                if (shape_has(cls[q], c)) t.b[c].w[h] |= bit;
            for (uint32_t r = off; r < kShapeMaxLen; r++) t.rowok[r].w[h] |= bit;
            for (uint32_t s = 0; s < kShapeSteps; s++)
                if (off < (1u << s)) t.z[s].w[h] |= bit;
        }
        t.last[k] = (uint8_t)(q - 1);
        t.len[k] = (uint8_t)len[k];
        for (uint32_t c = 0; c < 256; c++) {
            if (shape_has(not_before[k], c)) {
                t.nb[c] |= (uint8_t)(1u << k);
                t.nb_used |= 1u << k;
            }
            if (shape_has(not_after[k], c)) t.na[c] |= (uint8_t)(1u << k);
        }
    }
}

// ---- ends -----------------------------------------------------------------------------------------------------------
// bit k: D has pattern k's last position (the guards come after)
template <uint32_t NW>
__host__ __device__ inline uint32_t shape_last_bits(const ShapeWord<NW>& d, const uint8_t* last, uint32_t n_patterns) {
    const uint64_t lo = d.w[0], hi = d.w[NW - 1];  // (scalars before the loop: a word indexed by a run-time half would leave the registers)
    uint32_t e = 0;
    for (uint32_t k = 0; k < n_patterns; k++) {
        const uint32_t q = last[k];
        e |= ((uint32_t)((NW == 2 && (q & 64u) ? hi : lo) >> (q & 63u)) & 1u) << k;
    }
    return e;
}
// the before-guard of pattern k applies at a byte `in_row` bytes after its row's first: the match's start is not the row's
__host__ __device__ inline bool shape_guarded_before(uint64_t in_row, uint32_t len) { return in_row >= len; }

// ---- cover ----------------------------------------------------------------------------------------------------------
// own, next: the lanes of a chunk and of the chunk after it at which a match of one pattern ends.  Is `lane` of the first
// chunk inside a match, that is, does an end lie in lane .. lane + len - 1?
__host__ __device__ inline bool shape_covered(uint64_t own, uint64_t next, uint32_t lane, uint32_t len) {
    const uint64_t from_lane = lane ? (own >> lane) | (next << (64u - lane)) : own;
    return (from_lane & textstat_below(len)) != 0;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// shape.hip.  All pointers but len are device memory; nw is shape_nw of the lengths' sum and table kShapeTableWords<nw>
// words.  count i64[S] (may be NULL; pre-set to 0 here) and ends u8[n_bytes] (may be NULL).  table may be NULL when the
// corpus has no byte.
hipError_t launch_shape_ends(const DedupRows& rows, uint32_t nw, const uint64_t* table, int64_t* count, uint8_t* ends, hipStream_t stream);
// covered i64[S] (may be NULL; pre-set to 0 here) and mask u8[n_bytes] (may be NULL) of ends u8[n_bytes], from any source
// (NULL when the corpus has no byte); len: the n_patterns lengths, host memory, which travel as kernel arguments.
hipError_t launch_shape_cover(const DedupRows& rows, uint32_t n_patterns, const uint32_t* len, const uint8_t* ends, int64_t* covered, uint8_t* mask,
                              hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
