// A deterministic automaton over the bytes of every row of a resident corpus (include/tgx_patterns.h:
// tgx_corpus_dfa_hits_device): the check of an automaton, a byte's state map, the composition of two maps, the table a
// call uploads, and the operator that turns the chunks' records into each chunk's carry.  The kernels of dfa.hip and the
// host twin in host_twins.cpp (tgx_dfa_hits_host) both go through these functions; the tiling and the masks over a
// chunk's lanes are textstat.h's, and the rule of the row sums is textstat_row_inside.  DESIGN.md, section L.18.
//
// The map.  The step of a DFA on byte b is a function from states to states, s -> next[b][s].  It is kept as a word of
// NS nibbles, nibble s holding next[b][s]: NS = 16 in a uint64_t, and NS = 8 in a uint32_t for an automaton of at most
// eight states.  A nibble at or above n_states holds its own index, so the identity is 0xFEDCBA9876543210 (its low half
// at NS = 8).  `a` then `b` is the map c with c[s] = b[a[s]]: dfa_compose<NS>(a, b).  Composition of functions is
// associative and not commutative; the identity map is its identity.
//
// Rows need no segmented state.  Every row begins in `start`, so the map of a row's FIRST byte b is taken to be the
// CONSTANT map, every nibble next[b][start].  Composing anything with a constant map on its right gives that constant
// map, c[s] = b[a[s]] = b's one value, so whatever precedes a row, in its chunk or in the chunks before, drops out by
// arithmetic: no reset ballot, no reach, no flag in the record.  A match cut by a row boundary ("a" then "b" under `ab`)
// is the case that holds it.
//
// The scan.  Lane i starts with its byte's map and takes six steps d = 1, 2, 4 .. 32; in step d a lane i >= d composes
// the map of lane i - d in front of its own.  After the steps lane i holds the map of the chunk's bytes up to and
// including its own.  The chunk's RECORD is the map of its last byte; one exclusive scan of the records under
// DfaCarryOp gives every chunk its CARRY, the map of everything in front of it (the corpus's first byte is a row's first
// byte, so the identity in front of chunk 0 is harmless).  The state after a byte is nibble carry[start] of its map.
//
// The composition by byte permutes.  Sixteen variable shifts of a 64-bit word are what the definition asks for.
// Instead the nibbles of b are spread into bytes, the even ones in one pair of words and the odd ones in another, and a
// byte permute (v_perm_b32 on the device, __builtin_amdgcn_perm; the same selection in plain C++ on the host) looks up
// four of a's nibbles at a time in each: selector x >> 1 picks the byte, and x & 1 picks between the even and the odd
// table.  Four lookups of four serve NS = 16, two serve NS = 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"

namespace tgx {

constexpr uint32_t kDfaMaxStates = 16;  // TGX_DFA_MAX_STATES
constexpr int kDfaStages = 3;

// ---- the automaton's check ------------------------------------------------------------------------------------------
// next: u8[256][16], tag: u8[16] (the fields of tgx_dfa).  NULL, or what is wrong with it.
inline const char* dfa_check(uint32_t n_states, uint32_t start, const uint8_t (*next)[kDfaMaxStates], const uint8_t* tag) {
    if (n_states < 1 || n_states > kDfaMaxStates) return "n_states is outside 1 .. 16";
    if (start >= n_states) return "start is no state";
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t s = 0; s < n_states; s++)
            if (next[b][s] >= n_states) return "an entry of next is no state";
    if (tag[start] != 0) return "tag[start] is not 0: the pattern matches the empty string";
    return nullptr;
}
// the instantiation that serves an automaton
__host__ __device__ inline uint32_t dfa_width(uint32_t n_states) { return n_states <= 8 ? 8u : 16u; }

// ---- maps -----------------------------------------------------------------------------------------------------------
template <uint32_t NS>
struct DfaMapOf;
template <>
struct DfaMapOf<8> {
    using type = uint32_t;
};
template <>
struct DfaMapOf<16> {
    using type = uint64_t;
};
template <uint32_t NS>
using DfaMap = typename DfaMapOf<NS>::type;

template <uint32_t NS>
__host__ __device__ constexpr DfaMap<NS> dfa_identity() {
    return (DfaMap<NS>)0xFEDCBA9876543210ull;
}
// nibble s of m
template <uint32_t NS>
__host__ __device__ inline uint32_t dfa_at(DfaMap<NS> m, uint32_t s) {
    return (uint32_t)(m >> (4 * s)) & 15u;
}
// every nibble v
template <uint32_t NS>
__host__ __device__ inline DfaMap<NS> dfa_constant(uint32_t v) {
    return (DfaMap<NS>)0x1111111111111111ull * (DfaMap<NS>)v;
}

// bytes 0 .. 3 of the result: byte (sel >> 8 i) & 7 of the eight bytes hi:lo.  (Every selector here is below 8.)
__host__ __device__ inline uint32_t dfa_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 4; i++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
#endif
}
// Four lookups: x holds a nibble index per byte; e1:e0 the table's even entries, a byte each, o1:o0 its odd ones.
__host__ __device__ inline uint32_t dfa_lookup4(uint32_t x, uint32_t e0, uint32_t e1, uint32_t o0, uint32_t o1) {
    const uint32_t sel = (x >> 1) & 0x07070707u;
    const uint32_t odd = (x & 0x01010101u) * 0xFFu;  // 0xFF in the bytes whose index is odd
    return (dfa_perm(o1, o0, sel) & odd) | (dfa_perm(e1, e0, sel) & ~odd);
}

// `a` then `b`: c[s] = b[a[s]]
template <uint32_t NS>
__host__ __device__ inline DfaMap<NS> dfa_compose(DfaMap<NS> a, DfaMap<NS> b);
template <>
__host__ __device__ inline uint32_t dfa_compose<8>(uint32_t a, uint32_t b) {
    const uint32_t e = b & 0x0F0F0F0Fu, o = (b >> 4) & 0x0F0F0F0Fu;
    return dfa_lookup4(a & 0x0F0F0F0Fu, e, 0, o, 0) | (dfa_lookup4((a >> 4) & 0x0F0F0F0Fu, e, 0, o, 0) << 4);
}
template <>
__host__ __device__ inline uint64_t dfa_compose<16>(uint64_t a, uint64_t b) {
    constexpr uint64_t low = 0x0F0F0F0F0F0F0F0Full;
    const uint64_t be = b & low, bo = (b >> 4) & low, ae = a & low, ao = (a >> 4) & low;
    const uint32_t e0 = (uint32_t)be, e1 = (uint32_t)(be >> 32), o0 = (uint32_t)bo, o1 = (uint32_t)(bo >> 32);
    const uint64_t ce = dfa_lookup4((uint32_t)ae, e0, e1, o0, o1) | ((uint64_t)dfa_lookup4((uint32_t)(ae >> 32), e0, e1, o0, o1) << 32);
    const uint64_t co = dfa_lookup4((uint32_t)ao, e0, e1, o0, o1) | ((uint64_t)dfa_lookup4((uint32_t)(ao >> 32), e0, e1, o0, o1) << 32);
    return ce | (co << 4);
}

// The map a lane starts with: its byte's, or at a row's first byte the constant map of next[b][start].
template <uint32_t NS>
__host__ __device__ inline DfaMap<NS> dfa_lane_map(DfaMap<NS> of_byte, bool row_first, uint32_t start) {
    return row_first ? dfa_constant<NS>(dfa_at<NS>(of_byte, start)) : of_byte;
}
// The state after a byte: m the byte's scanned map, carry the map in front of its chunk.
template <uint32_t NS>
__host__ __device__ inline uint32_t dfa_state(DfaMap<NS> m, DfaMap<NS> carry, uint32_t start) {
    return dfa_at<NS>(m, dfa_at<NS>(carry, start));
}

// b after a.  Associative, not commutative; dfa_identity is its identity.
template <uint32_t NS>
struct DfaCarryOp {
    __host__ __device__ DfaMap<NS> operator()(const DfaMap<NS>& a, const DfaMap<NS>& b) const { return dfa_compose<NS>(a, b); }
};

// ---- the table of a call --------------------------------------------------------------------------------------------
// kDfaTableWords<NS> 8-byte words: the 256 maps, then the 16 tags.  A block copies them into LDS in this layout.
template <uint32_t NS>
constexpr uint32_t kDfaMapWords = 256 * sizeof(DfaMap<NS>) / 8;
template <uint32_t NS>
constexpr uint32_t kDfaTableWords = kDfaMapWords<NS> + kDfaMaxStates / 8;
template <uint32_t NS>
inline void dfa_build_table(uint32_t n_states, const uint8_t (*next)[kDfaMaxStates], const uint8_t* tag, uint64_t* words) {
    DfaMap<NS>* maps = reinterpret_cast<DfaMap<NS>*>(words);
    for (uint32_t b = 0; b < 256; b++) {
        DfaMap<NS> m = dfa_identity<NS>();
        for (uint32_t s = 0; s < n_states; s++) m = (m & ~((DfaMap<NS>)15 << (4 * s))) | ((DfaMap<NS>)next[b][s] << (4 * s));
        maps[b] = m;
    }
    uint8_t* tags = reinterpret_cast<uint8_t*>(words + kDfaMapWords<NS>);
    for (uint32_t s = 0; s < kDfaMaxStates; s++) tags[s] = s < n_states ? tag[s] : 0;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// dfa.hip.  All pointers are device memory; a corpus of n_bytes has n_chunks = ceil(n_bytes / 64) chunks, and width is
// dfa_width(n_states): 8 or 16, the maps being u32 or u64.
// the room that the scan of n_recs records needs
hipError_t dfa_scan_bytes8(uint64_t n_recs, size_t* scan_bytes);
hipError_t dfa_scan_bytes16(uint64_t n_recs, size_t* scan_bytes);
// rec[n_chunks + 1]: the records of the corpus's chunks, then the identity.  table: kDfaTableWords<width> words.
hipError_t launch_dfa_summary(const DedupRows& rows, uint32_t width, uint32_t start, const uint64_t* table, void* rec, hipStream_t stream);
// carry[n_recs] = the exclusive scan of the records under DfaCarryOp
hipError_t launch_dfa_scan(uint32_t width, const void* rec, void* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// count i64[S] (may be NULL; pre-set to 0 here) and ends u8[n_bytes] (may be NULL).  table and carry may be NULL when the
// corpus has no byte.
hipError_t launch_dfa(const DedupRows& rows, uint32_t width, uint32_t start, const uint64_t* table, const void* carry, int64_t* count, uint8_t* ends,
                      hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
