// Per-row word statistics of a resident corpus: the counts of the Gopher quality rules (include/tgx_words.h:
// tgx_corpus_word_stats_device): what a word, its length, a bullet line and an ellipsis are, the summary of a chunk with
// its two carried states, the operator that turns the summaries into each chunk's carry, and the match of a word against
// the caller's stop table.  The kernels of wordstat.hip and the host twin in host_twins.cpp (tgx_word_stats_host) both
// go through these functions; the tiling, the masks over a chunk's lanes and the rule of the row sums are textstat.h's.
// DESIGN.md, section L.15.
//
// Row i is the bytes text[offs[i] .. offs[i+1]).  Everything is defined by bytes alone, on invalid UTF-8 too.
//   SPACE: textstat_is_space (0x20, 0x09 .. 0x0D), the bytes Python's bytes.split() splits on.  Non-ASCII spaces are
//     ordinary bytes.
//   WORD: a maximal run of non-space bytes of one row.  p is a WORD START iff text[p] is no space and p is its row's
//     first byte or text[p - 1] is a space; a WORD END iff text[p] is no space and p is its row's last byte or text[p + 1]
//     is a space.  A word's length is its units: bytes, or under kWordstatChars characters (textstat_is_char).
//   LINE, line start, line end: textstat.h's.  A line's CONTENT is the line without its '\n'.
//   tail(p): the eight bytes text[p - 7 .. p], and prev(p) = text[p - 8]; any of them in front of the row's first byte
//     reads as 0x20.  Here tail(p) is a word whose byte j (bits 8j .. 8j + 7) is text[p - j]: byte 0 is text[p] itself.
//     Every look-around of the statistics is backwards and at most nine bytes.
//   nsb(p): the number of non-space bytes of p's line in front of p, saturated at 3.
//
// The carry.  A word end whose word start lies in its own chunk gets its length and its two flags (a letter, a byte >=
// 0x80) from one popcount each; any other needs what the word holds between its start and the chunk's first byte.  nsb
// is the same question about the line.  So a chunk's SUMMARY holds two segmented states with reset points of their own:
// the WORD state (reset: a space byte or a row's first byte; the units of non-space bytes, a letter seen, a byte >= 0x80
// seen, each since the last reset, the reset's own byte included) and the LINE state (reset: a line start; the non-space
// bytes since, the start's own byte included, saturated at 3).  One exclusive scan under WordstatCarryOp gives every
// chunk its CARRY: both states as they stand in front of its first byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"

namespace tgx {

constexpr uint32_t kWordstatN = 14;      // TGX_WORDSTAT_N
constexpr int kWordstatStages = 3;
constexpr uint32_t kWordstatChars = 1u;  // TGX_WORDSTAT_CHARS
constexpr uint32_t kWordstatFold = 2u;   // TGX_WORDSTAT_FOLD
constexpr uint32_t kWordstatMaxStop = 63;
constexpr uint32_t kWordstatMaxStopLen = 8;

// the statistics' places in the table (include/tgx_words.h)
enum : uint32_t {
    kWsWords = 0, kWsWordUnits = 1, kWsMaxWord = 2, kWsLongWords = 3, kWsAlphaWords = 4, kWsAlphaWideWords = 5, kWsHash = 6,
    kWsEllipsis = 7, kWsLines = 8, kWsBulletLines = 9, kWsEllipsisLines = 10, kWsPunctLines = 11, kWsStopWords = 12, kWsStopMask = 13,
};
// the bits of a byte's mark
enum : uint32_t { kWordMarkStart = 1u, kWordMarkEnd = 2u, kWordMarkStop = 4u, kWordMarkBullet = 8u };

// ---- bytes ----------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool wordstat_is_wide(uint8_t b) { return b >= 0x80u; }
// A-Z lowered, every other byte as it is ('@' and '[' stay)
__host__ __device__ inline uint8_t wordstat_fold(uint8_t b) { return (uint8_t)(b - 'A') < 26u ? (uint8_t)(b | 0x20u) : b; }
__host__ __device__ inline uint8_t wordstat_tail_byte(uint64_t tail, uint32_t j) { return (uint8_t)(tail >> (8 * j)); }

// ---- what a chunk's lanes are, as masks (textstat.h: a bit a lane) ------------------------------------------------------
struct WordMasks {
    uint64_t resets;    // the WORD state's reset points: a space byte or a row's first byte
    uint64_t units;     // the units of non-space bytes
    uint64_t alpha;     // A-Z, a-z
    uint64_t wide;      // bytes >= 0x80
    uint64_t nonspace;  // bytes that are no space
    uint64_t starts;    // the LINE state's reset points: line starts
};

// ---- the summary and the carry --------------------------------------------------------------------------------------
constexpr uint64_t kWordReset = 1ull << 63;   // the chunk holds a reset point of the WORD state
constexpr uint64_t kLineReset = 1ull << 62;   // the chunk holds a line start
constexpr uint64_t kWordAlpha = 1ull << 61;   // a letter since the WORD state's last reset
constexpr uint64_t kWordWide = 1ull << 60;    // a byte >= 0x80 since
constexpr uint32_t kLineNsbShift = 58;        // two bits: the non-space bytes since the last line start, saturated at 3
constexpr uint64_t kLineNsb = 3ull << kLineNsbShift;
constexpr uint64_t kWordUnits = (1ull << 40) - 1;  // the units since the WORD state's last reset (a row is shorter than 2^32)
constexpr uint64_t kWordPart = kWordReset | kWordAlpha | kWordWide | kWordUnits, kLinePart = kLineReset | kLineNsb;

__host__ __device__ inline uint64_t wordstat_sat3(uint64_t n) { return n < 3 ? n : 3; }
__host__ __device__ inline uint64_t wordstat_carry_units(uint64_t carry) { return carry & kWordUnits; }
__host__ __device__ inline uint64_t wordstat_carry_nsb(uint64_t carry) { return (carry & kLineNsb) >> kLineNsbShift; }

__host__ __device__ inline uint64_t wordstat_summary(const WordMasks& m) {
    const uint64_t w = m.resets ? ~textstat_below(textstat_top(m.resets)) : ~0ull;  // the lanes from the last reset on
    const uint64_t l = m.starts ? ~textstat_below(textstat_top(m.starts)) : ~0ull;
    return (m.resets ? kWordReset : 0) | (m.starts ? kLineReset : 0) | ((m.alpha & w) ? kWordAlpha : 0) | ((m.wide & w) ? kWordWide : 0) |
           (wordstat_sat3(textstat_popc(m.nonspace & l)) << kLineNsbShift) | textstat_popc(m.units & w);
}

// b after a, per state: b where b has a reset, else a combined with b (the units: sum; the flags: or; nsb: the
// saturating sum).  Each state's operator is a segmented one and associative; the two states share no bit, so the
// product is associative too, and 0 is its identity.  Not commutative.
struct WordstatCarryOp {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const {
        const uint64_t word = (b & kWordReset) ? (b & kWordPart) : ((a | b) & (kWordReset | kWordAlpha | kWordWide)) | ((a & kWordUnits) + (b & kWordUnits));
        const uint64_t line = (b & kLineReset) ? (b & kLinePart) : (a & kLineReset) | (wordstat_sat3(wordstat_carry_nsb(a) + wordstat_carry_nsb(b)) << kLineNsbShift);
        return word | line;
    }
};

// ---- a lane's word and line, from the chunk's masks and its carry ---------------------------------------------------
// The word that holds `lane` (a non-space byte), from its start up to the lane: its units, and whether a letter or a byte
// >= 0x80 was seen.  The carry is used only by a word that began before the chunk.
struct WordSoFar {
    uint64_t units;
    bool alpha, wide;
};
__host__ __device__ inline WordSoFar wordstat_word(const WordMasks& m, uint32_t lane, uint64_t carry) {
    const uint64_t upto = textstat_below(lane + 1), r = m.resets & upto;
    if (r) {
        const uint64_t span = upto & ~textstat_below(textstat_top(r));
        return {textstat_popc(m.units & span), (m.alpha & span) != 0, (m.wide & span) != 0};
    }
    return {wordstat_carry_units(carry) + textstat_popc(m.units & upto), (carry & kWordAlpha) || (m.alpha & upto), (carry & kWordWide) || (m.wide & upto)};
}
// nsb of the byte at `lane`
__host__ __device__ inline uint32_t wordstat_nsb(const WordMasks& m, uint32_t lane, uint64_t carry) {
    const uint64_t before = textstat_below(lane), s = m.starts & textstat_below(lane + 1);
    const uint64_t n = s ? textstat_popc(m.nonspace & before & ~textstat_below(textstat_top(s))) : wordstat_carry_nsb(carry) + textstat_popc(m.nonspace & before);
    return (uint32_t)wordstat_sat3(n);
}

// ---- what the tail says ---------------------------------------------------------------------------------------------
// the three bytes text[p - 2 - back .. p - back] are a, b, c
__host__ __device__ inline bool wordstat_three(uint64_t tail, uint32_t back, uint8_t a, uint8_t b, uint8_t c) {
    return ((tail >> (8 * back)) & 0xFFFFFFull) == (((uint64_t)a << 16) | ((uint64_t)b << 8) | c);
}
__host__ __device__ inline bool wordstat_is_word_start(uint64_t tail) {
    return !textstat_is_space(wordstat_tail_byte(tail, 0)) && textstat_is_space(wordstat_tail_byte(tail, 1));
}
// a run of three or more dots, counted once at its third dot, or the last byte of U+2026
__host__ __device__ inline bool wordstat_is_ellipsis(uint64_t tail) {
    return (wordstat_three(tail, 0, '.', '.', '.') && wordstat_tail_byte(tail, 3) != '.') || wordstat_three(tail, 0, 0xE2, 0x80, 0xA6);
}
// the last byte of a line-leading bullet: '-' or '*' as the line's first non-space byte, or the last byte of U+2022 as
// its first three
__host__ __device__ inline bool wordstat_is_bullet(uint64_t tail, uint32_t nsb) {
    const uint8_t b = wordstat_tail_byte(tail, 0);
    return ((b == '-' || b == '*') && nsb == 0) || (wordstat_three(tail, 0, 0xE2, 0x80, 0xA2) && nsb == 2);
}
// at a line end (is_nl: the end is a '\n', which is no content): the content ends in "..." or U+2026
__host__ __device__ inline bool wordstat_ellipsis_line(uint64_t tail, bool is_nl) {
    const uint32_t back = is_nl ? 1u : 0u;
    return wordstat_three(tail, back, '.', '.', '.') || wordstat_three(tail, back, 0xE2, 0x80, 0xA6);
}
// at a line end: the content's last byte is one of . ! ? "  (an empty content has the byte before the line, which is a
// '\n' or in front of the row)
__host__ __device__ inline bool wordstat_punct_line(uint64_t tail, bool is_nl) {
    const uint8_t b = wordstat_tail_byte(tail, is_nl ? 1u : 0u);
    return b == '.' || b == '!' || b == '?' || b == '"';
}

// ---- the stop table -------------------------------------------------------------------------------------------------
// An entry of n bytes (1 .. 8) is two words: its bytes laid as a tail's are (byte j is entry[n - 1 - j]), and n.  A word
// end matches it iff the n low bytes of the (folded) tail equal the entry and the byte before them, the tail's byte n or
// prev when n = 8, is a space: the word is the entry, not a longer word that ends in it.
constexpr uint32_t kWordstatStopWords = 2;  // u64 per entry
__host__ __device__ inline bool wordstat_matches(uint64_t tail, uint8_t prev, uint64_t entry, uint64_t n) {
    const uint64_t low = n >= 8 ? ~0ull : (1ull << (8 * n)) - 1;
    const uint8_t before = n >= 8 ? prev : wordstat_tail_byte(tail, (uint32_t)n);
    return (tail & low) == entry && textstat_is_space(before);
}

// tail(p) and prev(p) of the byte at p of the row that begins at row_begin, read plainly (the twin; the kernel shuffles)
inline uint64_t wordstat_tail_of(const uint8_t* text, uint64_t p, uint64_t row_begin, bool fold, uint8_t* prev) {
    uint64_t tail = 0;
    for (uint32_t j = 0; j <= 8; j++) {
        uint8_t b = p - row_begin >= j ? text[p - j] : 0x20u;
        if (fold) b = wordstat_fold(b);
        if (j < 8)
            tail |= (uint64_t)b << (8 * j);
        else
            *prev = b;
    }
    return tail;
}

// The caller's table (host memory) -> table u64[2 * n_stop] as above, or the reason it is refused: more than 63
// entries, an entry that is empty, longer than 8 bytes or holds a space byte, one that holds A-Z under kWordstatFold
// (it could never match), or two equal entries.
inline const char* wordstat_pack_table(const uint8_t* stop_bytes, const uint64_t* stop_offs, uint32_t n_stop, uint32_t flags, uint64_t* table) {
    if (n_stop > kWordstatMaxStop) return "more than 63 stop words";
    if (n_stop && !stop_offs) return "stop_offs is NULL";
    for (uint32_t k = 0; k < n_stop; k++) {
        if (stop_offs[k + 1] < stop_offs[k] || stop_offs[k + 1] - stop_offs[k] > kWordstatMaxStopLen) return "a stop word is longer than 8 bytes (or stop_offs descends)";
        const uint64_t n = stop_offs[k + 1] - stop_offs[k];
        if (n == 0) return "a stop word is empty";
        if (!stop_bytes) return "stop_bytes is NULL";
        uint64_t e = 0;
        for (uint64_t j = 0; j < n; j++) {
            const uint8_t b = stop_bytes[stop_offs[k] + n - 1 - j];
            if (textstat_is_space(b)) return "a stop word holds a space byte";
            if ((flags & kWordstatFold) && (uint8_t)(b - 'A') < 26u) return "a stop word holds A-Z under TGX_WORDSTAT_FOLD";
            e |= (uint64_t)b << (8 * j);
        }
        for (uint32_t q = 0; q < k; q++)
            if (table[kWordstatStopWords * q] == e && table[kWordstatStopWords * q + 1] == n) return "a stop word occurs twice";
        table[kWordstatStopWords * k] = e;
        table[kWordstatStopWords * k + 1] = n;
    }
    return nullptr;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// wordstat.hip.  All pointers are device memory.
// the room that the scan of n_chunks summaries needs
hipError_t wordstat_scan_bytes(uint64_t n_chunks, size_t* scan_bytes);
// summary u64[n_chunks] of the corpus's chunks
hipError_t launch_wordstat_summary(const DedupRows& rows, uint32_t flags, uint64_t* summary, hipStream_t stream);
// carry u64[n_chunks] = the exclusive scan of the summaries under WordstatCarryOp
hipError_t launch_wordstat_scan(const uint64_t* summary, uint64_t* carry, uint64_t n_chunks, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// stats i64[kWordstatN, S] (may be NULL; pre-set to 0 here) and marks u8[n_bytes] (may be NULL); table u64[2 * n_stop]
hipError_t launch_wordstat(const DedupRows& rows, uint64_t word_limit, uint32_t flags, const uint64_t* table, uint32_t n_stop, const uint64_t* carry,
                           int64_t* stats, uint8_t* marks, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
