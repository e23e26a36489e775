// The words of a resident corpus as rows of a result, one id per white-space word (include/tgx_word_ids.h:
// tgx_corpus_words): a word's digits, polynomial, key and id, the segmented state of a stretch of bytes with the doubling
// step of the in-wave scan, the record of a chunk, the operator that turns the records into each chunk's carry, the emit
// rule and the rule of the row offsets.  The kernels of words.hip and the host twin in host_twins.cpp (tgx_words_host) both
// go through these functions; the tiling and the masks over a chunk's lanes are textstat.h's, and space, word, word start,
// word end and the WORD state's reset points are wordstat.h's.  DESIGN.md, section L.17.
//
//   DIGIT of a byte b: b + 1 (1 .. 256); under kWordsFold b goes through wordstat_fold first (A-Z lowered, nothing else).
//   POLYNOMIAL of a word with the bytes b_0 .. b_{n-1}: P = sum_j digit(b_j) * M^(n-1-j) mod 2^64, M = kWordsM (odd).
//   KEY: dedup_mix(P ^ dedup_mix(t + n)), t = dedup_mix(seed + M), n the word's length in bytes.  ID: key >> 33.
//
// The state.  A stretch of bytes is (h, pow): h its polynomial, a space byte counting as the digit 0, and pow = M^len.
// `a` then `b` is (a.h * b.pow + b.h, a.pow * b.pow), which is associative.  A RESET point, a space byte or a row's first
// byte, drops what precedes it: the state of a stretch with a reset is that of its bytes from the last reset on.  A space
// is its own reset and holds 0, so the state at a word's last byte is the word's polynomial.
//
// The in-wave scan.  Lane i starts with its own digit and takes six steps d = 1, 2, 4 .. 32; in step d it adds
// h[i - d] * M^d iff no reset lies in the lanes (i - d, i].  Before step d such a lane holds exactly the d bytes
// (i - d, i], so the multiplier is the constant M^d; lane i - d holds the bytes from its own reach up to i - d.  After the
// steps lane i holds the state of the bytes from the last reset at or below it, or from lane 0, up to i.
//
// The carry.  A word end whose word began in its chunk has its polynomial already; any other needs the state in front of
// the chunk's first byte.  A first pass writes one RECORD per chunk: the state that is open at its end, the non-space
// bytes since the last reset (the word's length so far), whether it holds a reset, and its number of word ends.  One
// exclusive scan under WordsCarryOp gives every chunk its CARRY; one more record behind the last chunk's, the identity,
// takes the totals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textstat.h"
#include "wordstat.h"

namespace tgx {

constexpr uint32_t kWordsFold = 1u;              // TGX_WORDS_FOLD
constexpr uint32_t kWordsVocabSize = 0x80000000u;  // TGX_WORDS_VOCAB_SIZE: every id is below it
constexpr uint64_t kWordsMaxWords = 0xFFFFFFFEull;  // 2^32 - 1 words are refused, as 2^32 - 1 lines are
constexpr int kWordsStages = 4;
constexpr uint64_t kWordsM = 0x9E3779B97F4A7C15ULL;

// ---- a word's digits, key and id ------------------------------------------------------------------------------------
// M^e mod 2^64
__host__ __device__ constexpr uint64_t words_pow(uint64_t e) {
    uint64_t r = 1, b = kWordsM;
    for (; e; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}
__host__ __device__ inline uint64_t words_digit(uint8_t b, bool fold) { return (uint64_t)(fold ? wordstat_fold(b) : b) + 1; }
__host__ __device__ inline uint64_t words_seed(uint64_t seed) { return dedup_mix(seed + kWordsM); }
// t = words_seed(seed)
__host__ __device__ inline uint64_t words_key(uint64_t poly, uint64_t n_bytes, uint64_t t) { return dedup_mix(poly ^ dedup_mix(t + n_bytes)); }
__host__ __device__ inline uint32_t words_id(uint64_t key) { return (uint32_t)(key >> 33); }
// the key of n bytes taken as one word, by the definition (tgx_word_key)
inline uint64_t words_key_of(const uint8_t* bytes, uint64_t n, bool fold, uint64_t seed) {
    uint64_t poly = 0;
    for (uint64_t j = 0; j < n; j++) poly = poly * kWordsM + words_digit(bytes[j], fold);
    return words_key(poly, n, words_seed(seed));
}

// ---- the in-wave scan -----------------------------------------------------------------------------------------------
// How far below itself a lane may reach: the lanes between it and the last reset at or below it (resets: the chunk's
// mask), or all the lanes below it without one.  Step d of the scan adds iff d <= reach.
__host__ __device__ inline uint32_t words_reach(uint64_t resets, uint32_t lane) {
    const uint64_t r = resets & textstat_below(lane + 1);
    return r ? lane - textstat_top(r) : lane;
}
// step D of lane i: mine is the lane's h, below that of lane i - D (anything when i < D: reach < D there)
template <uint32_t D>
__host__ __device__ inline uint64_t words_step(uint64_t mine, uint64_t below, uint32_t reach) {
    constexpr uint64_t m = words_pow(D);
    return D <= reach ? mine + below * m : mine;
}

// ---- the record and the carry ---------------------------------------------------------------------------------------
constexpr uint64_t kWordsReset = 1ull << 63;  // of `open`: the stretch holds a reset
struct WordsRec {
    uint64_t h, pow;  // the state from the last reset on (of the whole stretch without one)
    uint64_t ends;    // word ends
    uint64_t open;    // the non-space bytes from the last reset on (a row is shorter than 2^32), and kWordsReset
};
__host__ __device__ inline WordsRec words_identity() { return {0, 1, 0, 0}; }
__host__ __device__ inline uint64_t words_open_bytes(uint64_t open) { return open & ~kWordsReset; }

// The record of a chunk of n_in bytes: resets, nonspace and ends are its masks, h_last the scanned h of its last lane.
__host__ __device__ inline uint32_t words_open_lanes(uint64_t resets, uint32_t n_in) { return resets ? n_in - textstat_top(resets) : n_in; }
// pow: M^words_open_lanes
__host__ __device__ inline WordsRec words_record(uint64_t resets, uint64_t nonspace, uint64_t ends, uint64_t h_last, uint64_t pow) {
    const uint64_t from = resets ? ~textstat_below(textstat_top(resets)) : ~0ull;  // the lanes from the last reset on
    return {h_last, pow, textstat_popc(ends), (resets ? kWordsReset : 0) | textstat_popc(nonspace & from)};
}

// b after a: the segmented state and length (b's where b has a reset) and the plain sum of the word ends.  Each part is
// associative and they share no field, so the product is; words_identity is its identity.  Not commutative.
struct WordsCarryOp {
    __host__ __device__ WordsRec operator()(const WordsRec& a, const WordsRec& b) const {
        if (b.open & kWordsReset) return {b.h, b.pow, a.ends + b.ends, b.open};
        return {a.h * b.pow + b.h, a.pow * b.pow, a.ends + b.ends, a.open + b.open};
    }
};

// ---- the emit rule --------------------------------------------------------------------------------------------------
// The key of the word that ends at `lane`: h the lane's scanned h, pow_lane = M^(lane + 1).  A word that began before the
// chunk (no reset at or below the lane) takes the carry's state in front of its own and the carry's bytes into its length.
__host__ __device__ inline uint64_t words_end_key(uint64_t resets, uint64_t nonspace, uint32_t lane, uint64_t h, uint64_t pow_lane, const WordsRec& carry,
                                                  uint64_t t) {
    const uint64_t upto = textstat_below(lane + 1), r = resets & upto;
    if (r) return words_key(h, textstat_popc(nonspace & upto & ~textstat_below(textstat_top(r))), t);
    return words_key(carry.h * pow_lane + h, words_open_bytes(carry.open) + textstat_popc(nonspace & upto), t);
}
// its place among the ids
__host__ __device__ inline uint64_t words_end_place(uint64_t ends, uint32_t lane, const WordsRec& carry) {
    return carry.ends + textstat_popc(ends & textstat_below(lane));
}

// ---- the row offsets ------------------------------------------------------------------------------------------------
// out_offs[k], k = 0 .. S: the word ends in front of byte offs[k] (a row's end always ends a word, so that is the words of
// the rows before k).  carry: rec[n_chunks + 1], the scanned records with the totals last.  p = offs[k] < N lies in chunk
// p / 64, whose carry counts the ends before the chunk; the ends of its bytes in front of p are rebuilt from those bytes,
// the byte after each and the rows' ends.  Empty rows and several rows that begin at one byte are no special case.
__host__ __device__ inline uint64_t words_row_offset(const uint8_t* text, const uint64_t* offs, uint64_t k, uint64_t n_bytes, const WordsRec* carry) {
    const uint64_t p = n_bytes ? offs[k] : 0;
    if (p >= n_bytes) return n_bytes ? carry[(n_bytes + kTextstatChunk - 1) / kTextstatChunk].ends : 0;
    const uint64_t c0 = p & ~(uint64_t)(kTextstatChunk - 1);
    uint64_t n = carry[c0 / kTextstatChunk].ends;
    if (c0 == p) return n;
    uint64_t i = pack_find_row(offs, 0, 0, k, c0), end = offs[i + 1];  // the row of the byte at q and its end (offs[k] = p > q)
    for (uint64_t q = c0; q < p; q++) {
        if (q >= end) {
            i = pack_find_row(offs, 0, i + 1, k, q);
            end = offs[i + 1];
        }
        if (!textstat_is_space(text[q]) && (q + 1 == end || textstat_is_space(text[q + 1]))) n++;  // (q + 1 <= p < N)
    }
    return n;
}

#ifndef TGX_HOST_ONLY  // (host_twins.cpp: nothing below is for a translation unit without kernels)

// words.hip.  All pointers are device memory; a corpus of n_bytes has n_chunks = ceil(n_bytes / 64) chunks.
// the room that the scan of n_recs records needs
hipError_t words_scan_bytes(uint64_t n_recs, size_t* scan_bytes);
// rec[n_chunks + 1]: the records of the corpus's chunks, then the identity
hipError_t launch_words_summary(const DedupRows& rows, uint32_t flags, WordsRec* rec, hipStream_t stream);
// carry[n_recs] = the exclusive scan of the records under WordsCarryOp
hipError_t launch_words_scan(const WordsRec* rec, WordsRec* carry, uint64_t n_recs, void* scan_tmp, size_t scan_bytes, hipStream_t stream);
// ids u32[n_words], n_words = carry[n_chunks].ends
hipError_t launch_words_emit(const DedupRows& rows, uint32_t flags, uint64_t seed, const WordsRec* carry, uint32_t* ids, uint64_t n_words, hipStream_t stream);
// out_offs u64[S + 1]; carry may be NULL when the corpus has no byte
hipError_t launch_words_offsets(const DedupRows& rows, const WordsRec* carry, uint64_t* out_offs, hipStream_t stream);

#endif  // TGX_HOST_ONLY

}  // namespace tgx
