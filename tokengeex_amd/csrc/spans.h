// Index arithmetic of the token spans (include/tgx.h: tgx_result_spans_device, tgx_result_pad_spans_device,
// tgx_result_window_spans_device).  The kernels of spans.hip and the host twins in host_twins.cpp (tgx_spans_host,
// tgx_window_spans_host) both go through these functions, so a machine without a GPU checks the kernels' arithmetic: the
// packed word of a token, an element's value in the chosen unit, the span of an element from the scanned values, and
// the walks of the writers (the padded one through pad_row of layout.h, the windowed one through win_row, the flat
// one through the row cursor of the packed layout with A = 0).
//
// Element j of T has the value u_j in the chosen unit: len(x[j]) bytes, or leads(x[j]) characters.  P = the exclusive
// 64-bit prefix sums of u over the whole stream (P[T] = the total), so inside row i, which starts at element o[i],
// c(b_j) = P[j] - P[o[i]] and c(e_j) = P[j+1] - P[o[i]]: the character unit needs no byte positions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace tgx {

constexpr uint32_t kSpanChars = 8u;  // TGX_SPAN_CHARS

// A base token's word: bits 0..6 len (<= TGX_MAX_TOKEN_LEN = 64), bits 7..13 leads, bit 14 cont.
constexpr uint32_t kSpanWordLeadsShift = 7, kSpanWordCont = 1u << 14, kSpanWordMask = 0x7Fu;
// A special token's word (its length is below 2^31): bits 0..30 len, bits 31..61 leads, bit 62 cont.
constexpr uint32_t kSpanSpLeadsShift = 31;
constexpr uint64_t kSpanSpCont = 1ull << 62, kSpanSpMask = 0x7FFFFFFFull;
// An element's value word: bits 0..30 u_j, bit 31 cont (character unit only).
constexpr uint32_t kSpanValCont = 0x80000000u;

__host__ __device__ inline bool span_is_cont(uint8_t c) { return (c & 0xC0u) == 0x80u; }

// leads and cont of n bytes; *cont = 0 for n = 0
__host__ inline uint64_t span_leads(const uint8_t* bytes, uint64_t n, uint32_t* cont) {
    uint64_t leads = 0;
    for (uint64_t k = 0; k < n; k++) leads += span_is_cont(bytes[k]) ? 0u : 1u;
    *cont = n && span_is_cont(bytes[0]) ? 1u : 0u;
    return leads;
}
__host__ inline uint16_t span_word(const uint8_t* bytes, uint32_t n) {  // n <= 64
    uint32_t cont;
    const uint32_t leads = (uint32_t)span_leads(bytes, n, &cont);
    return (uint16_t)(n | (leads << kSpanWordLeadsShift) | (cont ? kSpanWordCont : 0u));
}
// bytes == NULL: the byte unit, which reads only the length
__host__ inline uint64_t span_special_word(const uint8_t* bytes, uint64_t n) {
    uint32_t cont = 0;
    const uint64_t leads = bytes ? span_leads(bytes, n, &cont) : 0;
    return n | (leads << kSpanSpLeadsShift) | (cont ? kSpanSpCont : 0ull);
}

// the words of the vocabulary and of the special tokens (device memory for the kernels, host memory for the twin)
struct SpanTables {
    const uint16_t* words;     // u16[V]
    const uint64_t* sp_words;  // u64[n_specials]
    uint32_t vocab_size, n_specials;
};

// the value word of id x; *oob: x is neither a token nor a special token (its value is 0)
__host__ __device__ inline uint32_t span_val(const SpanTables& t, uint32_t x, bool chars, bool* oob) {
    *oob = false;
    if (x < t.vocab_size) {
        const uint32_t w = t.words[x];
        if (!chars) return w & kSpanWordMask;
        return ((w >> kSpanWordLeadsShift) & kSpanWordMask) | ((w & kSpanWordCont) ? kSpanValCont : 0u);
    }
    const uint32_t k = x - t.vocab_size;
    if (k < t.n_specials) {
        const uint64_t w = t.sp_words[k];
        if (!chars) return (uint32_t)(w & kSpanSpMask);
        return (uint32_t)((w >> kSpanSpLeadsShift) & kSpanSpMask) | ((w & kSpanSpCont) ? kSpanValCont : 0u);
    }
    *oob = true;
    return 0;
}

struct SpanPair {
    int64_t start, end;
};

// the span of element j of the row that starts at element row0: val = j's value word, of which only the cont bit is
// looked at (the writers pass vals == NULL in the byte unit, where it is never set, and read nothing for it)
__host__ __device__ inline SpanPair span_of(const uint64_t* P, uint64_t row0, uint64_t j, uint32_t val) {
    const uint64_t base = P[row0];
    SpanPair s;
    s.start = (int64_t)(P[j] - base) - (int64_t)(val >> 31);
    s.end = (int64_t)(P[j + 1] - base);
    return s;
}

// the row's total in the chosen unit: what the int32 check takes the maximum of
__host__ __device__ inline uint64_t span_row_total(const uint64_t* P, const uint64_t* offs, uint64_t i) { return P[offs[i + 1]] - P[offs[i]]; }

// ---- padded: pair e = i·L + c of [S, L, 2], through the row mapping of the padded layout -------------------------
// (0, 0) on bos, eos and padding
__host__ __device__ inline SpanPair span_pad_at(const LayoutSeq& seq, const uint64_t* offs, const uint64_t* P, const uint32_t* vals, uint32_t L,
                                                uint32_t flags, uint64_t e) {
    const uint64_t i = e / L;
    const uint32_t c = (uint32_t)(e - i * L);
    const PadRow r = pad_row(offs, i, L, seq, flags);
    const uint32_t k = c - r.col0 - seq.has_bos;  // wraps to a large value left of the kept tokens
    SpanPair s = {0, 0};
    if (k < r.keep) s = span_of(P, offs[i], r.src + k, vals ? vals[r.src + k] : 0u);
    return s;
}

// ---- windows: pair e = w·L + c of [W, L, 2], through the window mapping of layout.h -----------------------------------
// The row that owns window w is the largest i with Wo[i] <= w (pack_find_row over Wo with A = 0).  A kept token gets
// the span it has in its whole row, so the pairs index the sample's text whichever window they stand in.
__host__ __device__ inline SpanPair span_window_at(const LayoutSeq& seq, const uint64_t* offs, const uint64_t* Wo, uint64_t n_rows, const uint64_t* P,
                                                   const uint32_t* vals, uint32_t L, uint32_t stride, uint32_t flags, uint64_t e) {
    const uint64_t w = e / L;
    const uint32_t c = (uint32_t)(e - w * L);
    const uint64_t i = pack_find_row(Wo, 0, 0, n_rows - 1, w);
    const WinRow r = win_row(offs, Wo, i, w, L, seq, stride, flags);
    const uint32_t k = c - r.p.col0 - seq.has_bos;  // wraps to a large value left of the kept tokens
    SpanPair s = {0, 0};
    if (k < r.p.keep) s = span_of(P, offs[i], r.p.src + k, vals ? vals[r.p.src + k] : 0u);
    return s;
}

// ---- flat: element j of [T, 2], in tiles of kSpanTile consecutive elements ------------------------------------------
// The row that owns element j is the largest i with offs[i] <= j: pack_find_row / pack_advance of layout.h with A = 0.
constexpr uint32_t kSpanGroup = 4;             // consecutive elements of a thread slot: 32 bytes of i32 pairs, 64 of i64
constexpr uint32_t kSpanTile = kPackTile;      // elements per tile: the kernel's block of 256 threads x 4 elements

// A thread slot's walk: v[k] = the span of element e0 + k for k < n_in <= kSpanGroup.  lo / hi: the rows that own the
// first and last element of the slot's tile.  Every sum is read once (an element's end is the next one's start) and the
// row's base only when the row changes.
__host__ __device__ inline void span_group(const uint64_t* offs, const uint64_t* P, const uint32_t* vals, uint64_t lo, uint64_t hi, uint64_t e0,
                                           uint32_t n_in, SpanPair (&v)[kSpanGroup]) {
    PackCursor cur;
    uint64_t row = ~0ull, base = 0, at = P[e0];
#pragma unroll
    for (uint32_t k = 0; k < kSpanGroup; k++) {
        if (k < n_in) {
            const uint64_t j = e0 + k;
            const uint64_t i = pack_advance(cur, offs, 0, lo, hi, j);
            if (i != row) {
                row = i;
                base = P[offs[i]];
            }
            const uint64_t next = P[j + 1];
            v[k].start = (int64_t)(at - base) - (int64_t)((vals ? vals[j] : 0u) >> 31);
            v[k].end = (int64_t)(next - base);
            at = next;
        }
    }
}

}  // namespace tgx
