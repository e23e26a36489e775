// Index arithmetic of the device front end (include/tgx.h: tgx_corpus_split_specials): a resident corpus split at special
// tokens, the segments between them packed back to back with the CRLF pass applied.  The kernels of front.hip and the
// host twin in host_twins.cpp (tgx_front_host) both go through these functions, so a machine without a GPU checks the
// kernels' index arithmetic.
//
// The text is walked in tiles of kFrontTile consecutive bytes, a thread slot owning kFrontGroup of them.
//   mark      per slot a 16-bit hit mask (a special token fits at that byte: the first in list order that does, bounded
//             by the sample's end) and a 16-bit mask of "\r\n" pairs; the hits become candidates (pos, end, special,
//             sample) in position order.
//   resolve   candidates overlap (special "aa" on "aaaaa"); the rule is sequential: accept iff pos >= cursor, then
//             cursor = end.  A candidate whose pos is >= every earlier end is accepted whatever came before (ends never
//             pass their sample's end, so this also covers the reset at a sample's start): it heads a run, and one
//             thread walks each run.
//   segments  an accepted candidate gives its special's segment, and one in front of it when the gap is not empty; a
//             sample gives one more for a non-empty tail.
//   pack      keep(p) = p lies in an encoded segment and is not the '\r' of a "\r\n" whose '\n' lies in the same segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kFrontGroup = 16;    // consecutive bytes of a thread slot: one 16-byte load
constexpr uint32_t kFrontTile = 4096;   // bytes per tile: the kernel's block of 256 threads x 16 bytes
constexpr uint32_t kFrontFirstBytes = 4;  // up to this many distinct first bytes of specials are looked for a word at a time
constexpr uint32_t kFrontMaxSpecials = 4096;           // more special tokens: TGX_ERR_UNSUPPORTED
constexpr uint64_t kFrontMaxSpecialBytes = 64u << 10;  // more bytes of special tokens: TGX_ERR_UNSUPPORTED

// The special tokens as the kernels read them.  The specials that start with byte b are by_first[first_start[b] ..
// first_start[b + 1]), in list order.
struct FrontTables {
    const uint32_t* first_mask;   // u32[8]: bit b is set when a special starts with byte b (the kernels keep it in LDS)
    const uint32_t* first_start;  // u32[257]
    const uint32_t* by_first;     // u32[n_specials]
    const uint32_t* sp_offs;      // u32[n_specials + 1], from 0
    const uint8_t* sp_bytes;
    uint32_t n_first;                       // distinct first bytes of the specials ...
    uint8_t first_bytes[kFrontFirstBytes];  // ... and which, when there are at most kFrontFirstBytes: a slot without one has no hit
};

// not 0 when a byte of w may be b (never 0 when one is)
__host__ __device__ inline uint32_t front_has_byte(uint32_t w, uint32_t b) {
    const uint32_t z = w ^ (b * 0x01010101u);
    return (z - 0x01010101u) & ~z & 0x80808080u;
}

// The sample that owns byte p < N is the LARGEST i with offs[i] <= p (pack_find_row of tile_fill.h with A = 0), so empty
// samples are stepped over; a tile's last byte is tile_last(t0, kFrontTile, n).

// a walk over ascending bytes of one tile, whose first and last byte belong to samples lo and hi
struct FrontCursor {
    uint64_t i = 0, end = 0;  // the current sample and its end
    bool have = false;
};
__host__ __device__ inline void front_advance(FrontCursor& cur, const uint64_t* offs, uint64_t lo, uint64_t hi, uint64_t p) {
    if (cur.have && p < cur.end) return;
    cur.i = pack_find_row(offs, 0, cur.have ? cur.i + 1 : lo, hi, p);
    cur.end = offs[cur.i + 1];
    cur.have = true;
}

// The special token at p: the first in list order that starts with text[p], fits before `end` and is there; -1: none.
__host__ __device__ inline int32_t front_match(const FrontTables& t, const uint8_t* text, uint64_t p, uint64_t end, uint32_t* len) {
    const uint32_t b = text[p];
    for (uint32_t j = t.first_start[b]; j < t.first_start[b + 1]; j++) {
        const uint32_t k = t.by_first[j];
        const uint32_t o = t.sp_offs[k], l = t.sp_offs[k + 1] - o;
        if (l > end - p) continue;
        uint32_t q = 1;
        while (q < l && text[p + q] == t.sp_bytes[o + q]) q++;
        if (q == l) {
            *len = l;
            return (int32_t)k;
        }
    }
    return -1;
}

// A slot's masks.  v: the slot's bytes (0 past the text's end), next: the byte after them (0 past the end).  Returns the
// hit mask; *crlf: bit q is set when byte q is '\r' and the byte after it '\n', wherever samples and segments end.
__host__ __device__ inline uint32_t front_mark_slot(const FrontTables& t, const uint8_t* text, const uint64_t* offs, uint64_t lo, uint64_t hi,
                                                    uint64_t p0, uint32_t n_in, const uint8_t (&v)[kFrontGroup], uint8_t next, uint32_t* crlf) {
    uint32_t hits = 0, cr = 0;
    // most slots hold neither a special's first byte nor a '\r': four words are asked instead of sixteen bytes
    uint32_t any_first = t.n_first > kFrontFirstBytes ? 1u : 0u, any_cr = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFrontGroup; j += 4) {
        const uint32_t w = (uint32_t)v[j] | (uint32_t)v[j + 1] << 8 | (uint32_t)v[j + 2] << 16 | (uint32_t)v[j + 3] << 24;
        any_cr |= front_has_byte(w, '\r');
#pragma unroll
        for (uint32_t f = 0; f < kFrontFirstBytes; f++)
            if (f < t.n_first) any_first |= front_has_byte(w, t.first_bytes[f]);
    }
    *crlf = 0;
    if (!any_first && !any_cr) return 0;
    FrontCursor cur;
#pragma unroll
    for (uint32_t q = 0; q < kFrontGroup; q++) {
        const uint32_t b = v[q];
        const uint32_t nb = q + 1 < kFrontGroup ? v[(q + 1) % kFrontGroup] : next;
        if (b == '\r' && nb == '\n') cr |= 1u << q;
        if (any_first && q < n_in && ((t.first_mask[b >> 5] >> (b & 31)) & 1u)) {
            front_advance(cur, offs, lo, hi, p0 + q);
            uint32_t len;
            if (front_match(t, text, p0 + q, cur.end, &len) >= 0) hits |= 1u << q;
        }
    }
    *crlf = cr;
    return hits;
}

// The slot's candidates, written in position order from index at: pos, end, special and sample of every hit.
__host__ __device__ inline void front_write_slot(const FrontTables& t, const uint8_t* text, const uint64_t* offs, uint64_t lo, uint64_t hi,
                                                 uint64_t p0, uint32_t hits, uint64_t at, uint64_t* cand_pos, uint64_t* cand_end,
                                                 uint32_t* cand_special, uint32_t* cand_sample) {
    FrontCursor cur;
    for (uint32_t q = 0; q < kFrontGroup; q++) {
        if (!((hits >> q) & 1u)) continue;
        front_advance(cur, offs, lo, hi, p0 + q);
        uint32_t len = 0;
        const int32_t k = front_match(t, text, p0 + q, cur.end, &len);
        cand_pos[at] = p0 + q;
        cand_end[at] = p0 + q + len;
        cand_special[at] = (uint32_t)k;
        cand_sample[at] = (uint32_t)cur.i;
        at++;
    }
}

// pm[c]: the largest end of candidates 0..c.  Candidate c heads a run when no earlier candidate reaches past its start.
__host__ __device__ inline bool front_is_head(const uint64_t* cand_pos, const uint64_t* pm, uint64_t c) { return c == 0 || cand_pos[c] >= pm[c - 1]; }

// The run that candidate c heads: acc_end[x] = the end of an accepted candidate x, 0 for a rejected one.
__host__ __device__ inline void front_resolve_run(const uint64_t* cand_pos, const uint64_t* cand_end, const uint64_t* pm, uint64_t n_cand, uint64_t c,
                                                  uint64_t* acc_end) {
    uint64_t cursor = cand_end[c];
    acc_end[c] = cursor;
    for (uint64_t x = c + 1; x < n_cand && cand_pos[x] < pm[x - 1]; x++) {
        const bool take = cand_pos[x] >= cursor;
        if (take) cursor = cand_end[x];
        acc_end[x] = take ? cursor : 0;
    }
}

// la[c]: the largest acc_end of candidates 0..c.  Where the text that no special has claimed yet starts in front of
// candidate c of a sample that starts at `begin`: the end of the accepted candidate before it in the same sample (an
// end of an earlier sample is <= begin), else the sample's start.
__host__ __device__ inline uint64_t front_cursor_before(const uint64_t* la, uint64_t c, uint64_t begin) {
    const uint64_t e = c ? la[c - 1] : 0;
    return e > begin ? e : begin;
}

// segments of candidate c: 0 when rejected, else its special's and one more for a non-empty gap in front of it
__host__ __device__ inline uint32_t front_cand_segs(const uint64_t* cand_pos, const uint64_t* acc_end, const uint64_t* la, const uint32_t* cand_sample,
                                                    const uint64_t* offs, uint64_t c) {
    if (!acc_end[c]) return 0;
    return cand_pos[c] > front_cursor_before(la, c, offs[cand_sample[c]]) ? 2u : 1u;
}

// the first candidate at or after byte p
__host__ __device__ inline uint64_t front_first_cand(const uint64_t* cand_pos, uint64_t n_cand, uint64_t p) {
    uint64_t lo = 0, hi = n_cand;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (cand_pos[mid] < p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Sample i's segments: those of its candidates [first[i], first[i + 1]) (seg_sum: the exclusive sums of front_cand_segs)
// and its tail.  *tail_begin: where the tail starts (== offs[i + 1]: none).
__host__ __device__ inline uint64_t front_sample_segs(const uint64_t* offs, const uint64_t* first, const uint64_t* seg_sum, const uint64_t* la, uint64_t i,
                                                      uint64_t* tail_begin) {
    const uint64_t t = front_cursor_before(la, first[i + 1], offs[i]);
    *tail_begin = t;
    return seg_sum[first[i + 1]] - seg_sum[first[i]] + (t < offs[i + 1] ? 1u : 0u);
}

// The first encoded segment in [lo, hi) that ends after byte p (hi: none of them).
__host__ __device__ inline uint64_t front_first_enc(const uint64_t* enc_end, uint64_t lo, uint64_t hi, uint64_t p) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (enc_end[mid] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// A slot's keep mask.  e_lo, e_hi: the first encoded segments that end after the tile's first and last byte (the slot's
// lies between them; n_enc: none).  *begins: bit
// q is set when an encoded segment starts at byte q; those segments are *first_begin, *first_begin + 1, ... in order.
__host__ __device__ inline uint32_t front_keep_slot(const uint64_t* enc_begin, const uint64_t* enc_end, uint64_t n_enc, uint64_t e_lo, uint64_t e_hi,
                                                    uint64_t p0, uint32_t n_in, uint32_t crlf_mask, bool crlf, uint32_t* begins, uint64_t* first_begin) {
    uint32_t keep = 0, bg = 0;
    uint64_t e = front_first_enc(enc_end, e_lo, e_hi, p0), fb = 0;
    uint64_t b = e < n_enc ? enc_begin[e] : ~0ull, en = e < n_enc ? enc_end[e] : ~0ull;
    for (uint32_t q = 0; q < n_in && e < n_enc; q++) {
        const uint64_t p = p0 + q;
        if (p >= en) {  // segments are not empty and do not overlap: the next one ends after p
            e++;
            if (e >= n_enc) break;
            b = enc_begin[e];
            en = enc_end[e];
        }
        if (p < b) continue;
        if (p == b) {
            if (!bg) fb = e;
            bg |= 1u << q;
        }
        if (crlf && ((crlf_mask >> q) & 1u) && p + 1 < en) continue;
        keep |= 1u << q;
    }
    *begins = bg;
    *first_begin = fb;
    return keep;
}

__host__ __device__ inline uint32_t front_popc(uint32_t x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (((x + (x >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

// Where the slot's encoded segments start inside their tile's output: prefix = kept bytes of the tile before the slot.
__host__ __device__ inline void front_slot_begins(uint32_t keep, uint32_t begins, uint64_t first_begin, uint32_t prefix, uint32_t* enc_local) {
    for (uint32_t q = 0; begins >> q; q++)
        if ((begins >> q) & 1u) enc_local[first_begin++] = prefix + front_popc(keep & ((1u << q) - 1u));
}

// ---- launchers (front.hip) ------------------------------------------------------------------------------------------

struct FrontParams {
    const uint8_t* text;   // N bytes, 16-byte aligned, readable (as zeros) up to the next multiple of 16 and one byte on
    const uint64_t* offs;  // u64[S + 1]
    uint64_t n_bytes, n_samples;
    FrontTables tab;       // first_mask: device memory here, copied to LDS by the kernels
    uint16_t* hit_mask;    // u16[slots]
    uint16_t* crlf_mask;   // u16[slots]
    uint16_t* keep_mask;   // u16[slots]
    uint64_t *tile_count, *tile_base;  // u64[tiles + 1]: hits per tile and their exclusive sums (mark), then the same for kept bytes (pack)
    // candidates
    uint64_t n_cand;
    uint64_t *cand_pos, *cand_end, *pm, *acc_end, *la, *seg_sum;  // u64[C] ... seg_sum u64[C + 1]
    uint32_t *cand_special, *cand_sample, *cand_segs;              // u32[C] ... cand_segs u32[C + 1]
    // samples and segments
    uint64_t *first, *sample_segs, *seg_offs;  // u64[S + 1] each
    uint64_t n_segs, n_enc;
    uint64_t *seg_begin, *seg_end, *rank;  // u64[K], u64[K], u64[K + 1]
    int32_t* seg_special;                  // i32[K + 1]
    uint64_t *enc_begin, *enc_end;         // u64[E]
    uint32_t* enc_local;                   // u32[E]
    uint64_t* out_offs;                    // u64[E + 1]
    uint8_t* out;                          // the packed segments
    uint32_t crlf;
};

hipError_t front_scan_temp_bytes(uint64_t n, size_t* bytes);  // for every scan below over up to n elements
hipError_t launch_front_mark(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream);      // masks, tile_count
hipError_t launch_front_candidates(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream);  // candidates .. seg_offs
hipError_t launch_front_segments(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream);    // seg_*, rank
hipError_t launch_front_keep(const FrontParams& p, void* temp, size_t temp_bytes, hipStream_t stream);        // enc_*, keep_mask, out_offs
hipError_t launch_front_pack(const FrontParams& p, hipStream_t stream);                                       // out

}  // namespace tgx
