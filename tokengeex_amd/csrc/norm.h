// Unicode normalisation of a resident corpus (include/tgx.h: tgx_corpus_normalize): every row replaced by what
// tgx_normalize_segments makes of it, in HBM.  The kernels of norm.hip and the host twin in host_twins.cpp
// (tgx_normalize_host) both go through these functions, so a machine without a GPU checks the decoder, the property
// lookup, the stream machine and the index arithmetic.
//
// A row is a sequence of units (norm_next: a scalar value, or an offending byte that travels alone).  A unit is active
// under a form when it can change or can change its neighbour (norm_active); almost all text is inert.  A piece is a head
// (an inert unit in front of an active one, or an active unit that starts its row) and the active units behind it; the
// bytes outside pieces are copied, every piece is normalised on its own by one thread (NormStream).
//   mark     per slot of front.h's tiles a 16-bit mask of the bytes that pieces cover and a 16-bit mask of the heads
//   pieces   (begin, row) of every piece in position order
//   length   the bytes every piece turns into, and the lowest row whose window overflows
//   places   the copied bytes and the heads of a tile in front of every slot; with the tiles' sums every copied byte, every
//            head and every row's first byte has its place in the output
//   write    the copied bytes, and the pieces once more with the machine writing
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "front.h"

namespace tgx {

constexpr uint32_t kNormWindow = 32;          // scalars of a stream window: a starter and 31 non-starters
constexpr uint32_t kNormRaw = 0x80000000u;    // an offending byte b travels as kNormRaw | b
constexpr uint32_t kNormStage1 = 0x1100;      // cp >> 8 of the scalar values up to 0x10FFFF
constexpr uint64_t kNormNoRow = ~0ull;        // no row's window has overflowed

// The normaliser's data as the kernels read it (unicode_tables.h) and the activity of every scalar value: bit f of
// stage2[stage1[cp >> 8] * 256 + (cp & 255)] is set when cp is active under form f.  Block 0 is "all inert".
struct NormTables {
    const uint16_t* stage1;  // u16[kNormStage1]
    const uint8_t* stage2;   // u8[blocks * 256]
    const uint32_t* ccc_cp;
    const uint8_t* ccc_val;
    const uint32_t *canon_cp, *canon_off, *canon_seq;
    const uint8_t* canon_len;
    const uint32_t *compat_cp, *compat_off, *compat_seq;
    const uint8_t* compat_len;
    const uint32_t *pair_first, *pair_second, *pair_composite;
    uint32_t ccc_n, canon_n, compat_n, pair_n;
};

namespace norm_hangul {
constexpr uint32_t S_BASE = 0xAC00, L_BASE = 0x1100, V_BASE = 0x1161, T_BASE = 0x11A7;
constexpr uint32_t L_COUNT = 19, V_COUNT = 21, T_COUNT = 28, N_COUNT = V_COUNT * T_COUNT, S_COUNT = L_COUNT * N_COUNT;
}  // namespace norm_hangul

// The unit at s[i] of a row that ends at `end` (i < end), strict UTF-8 as unicode_norm.cpp's next_cp: no overlong forms,
// no surrogates, <= 0x10FFFF, and no continuation byte is looked for at or after `end`.
__host__ __device__ inline uint32_t norm_next(const uint8_t* s, uint64_t end, uint64_t& i) {
    const uint32_t b0 = s[i];
    if (b0 < 0x80) {
        i++;
        return b0;
    }
    const uint32_t b1 = i + 1 < end ? s[i + 1] : 0u, c1 = (b1 & 0xC0u) == 0x80u;
    if (b0 >= 0xC2 && b0 <= 0xDF && c1) {
        i += 2;
        return ((b0 & 0x1Fu) << 6) | (b1 & 63u);
    }
    const uint32_t b2 = c1 && i + 2 < end ? s[i + 2] : 0u, c2 = (b2 & 0xC0u) == 0x80u;
    if (b0 >= 0xE0 && b0 <= 0xEF && c2) {
        const uint32_t cp = ((b0 & 0x0Fu) << 12) | ((b1 & 63u) << 6) | (b2 & 63u);
        if (cp >= 0x800 && !(cp >= 0xD800 && cp <= 0xDFFF)) {
            i += 3;
            return cp;
        }
    }
    const uint32_t b3 = c2 && i + 3 < end ? s[i + 3] : 0u, c3 = (b3 & 0xC0u) == 0x80u;
    if (b0 >= 0xF0 && b0 <= 0xF4 && c3) {
        const uint32_t cp = ((b0 & 0x07u) << 18) | ((b1 & 63u) << 12) | ((b2 & 63u) << 6) | (b3 & 63u);
        if (cp >= 0x10000 && cp <= 0x10FFFF) {
            i += 4;
            return cp;
        }
    }
    i++;
    return kNormRaw | b0;
}

// Raw bytes and ASCII are inert; a scalar of an "all inert" block is answered by the first stage alone.
__host__ __device__ inline bool norm_active(const NormTables& t, uint32_t form, uint32_t cp) {
    if (cp < 0x80 || (cp & kNormRaw)) return false;
    const uint32_t b = t.stage1[cp >> 8];
    return b && ((t.stage2[b * 256u + (cp & 255u)] >> form) & 1u);
}

// index of cp in the ascending cps[0 .. n), or -1
__host__ __device__ inline int32_t norm_find(const uint32_t* cps, uint32_t n, uint32_t cp) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (cps[mid] < cp)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && cps[lo] == cp ? (int32_t)lo : -1;
}

__host__ __device__ inline uint32_t norm_ccc(const NormTables& t, uint32_t cp) {
    if (cp < 0x300 || (cp & kNormRaw)) return 0;
    const int32_t i = norm_find(t.ccc_cp, t.ccc_n, cp);
    return i < 0 ? 0u : t.ccc_val[i];
}

// a scalar's full decomposition: n scalars, read one at a time with norm_decomp_at
struct NormDecomp {
    const uint32_t* seq;  // the tables' sequence, or NULL: a Hangul syllable (n > 1) or cp itself
    uint32_t n, cp;
};
__host__ __device__ inline NormDecomp norm_decompose(const NormTables& t, uint32_t cp, bool compat) {
    using namespace norm_hangul;
    if (cp < 0xA0 || (cp & kNormRaw)) return {nullptr, 1, cp};
    if (cp >= S_BASE && cp < S_BASE + S_COUNT) return {nullptr, (cp - S_BASE) % T_COUNT ? 3u : 2u, cp};
    const int32_t i = compat ? norm_find(t.compat_cp, t.compat_n, cp) : norm_find(t.canon_cp, t.canon_n, cp);
    if (i < 0) return {nullptr, 1, cp};
    return compat ? NormDecomp{t.compat_seq + t.compat_off[i], t.compat_len[i], cp} : NormDecomp{t.canon_seq + t.canon_off[i], t.canon_len[i], cp};
}
__host__ __device__ inline uint32_t norm_decomp_at(const NormDecomp& d, uint32_t k) {
    using namespace norm_hangul;
    if (d.seq) return d.seq[k];
    if (d.n == 1) return d.cp;
    const uint32_t si = d.cp - S_BASE;
    return k == 0 ? L_BASE + si / N_COUNT : k == 1 ? V_BASE + (si % N_COUNT) / T_COUNT : T_BASE + si % T_COUNT;
}

// the primary composite of a and b, or 0 (unicode_norm.cpp's compose_pair)
__host__ __device__ inline uint32_t norm_compose_pair(const NormTables& t, uint32_t a, uint32_t b) {
    using namespace norm_hangul;
    if ((a | b) & kNormRaw) return 0;
    if (a >= L_BASE && a < L_BASE + L_COUNT && b >= V_BASE && b < V_BASE + V_COUNT) return S_BASE + ((a - L_BASE) * V_COUNT + (b - V_BASE)) * T_COUNT;
    if (a >= S_BASE && a < S_BASE + S_COUNT && (a - S_BASE) % T_COUNT == 0 && b > T_BASE && b < T_BASE + T_COUNT) return a + (b - T_BASE);
    uint32_t lo = 0, hi = t.pair_n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (t.pair_first[mid] < a || (t.pair_first[mid] == a && t.pair_second[mid] < b))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < t.pair_n && t.pair_first[lo] == a && t.pair_second[lo] == b ? t.pair_composite[lo] : 0u;
}

// ---- the stream machine: one piece normalised by one thread ----------------------------------------------------------

// The decomposed stream since the last starter: a starter (or, at a row's start, none) and the non-starters behind it.
// Element k of the window is cp[k * stride] / cc[k * stride]: the kernels keep a block's windows interleaved in LDS.
struct NormStream {
    uint32_t* cp;
    uint8_t* cc;
    uint32_t stride;
    uint8_t* out;  // where the piece's bytes go; NULL: they are only counted
    uint32_t n = 0;
    uint64_t produced = 0;
    bool overflow = false;  // the window had no room for a non-starter: the piece's output is not to be used
};

__host__ __device__ inline void norm_emit(NormStream& s, uint32_t cp) {
    uint8_t b[4];
    uint32_t l;
    if (cp < 0x80 || (cp & kNormRaw)) {
        b[0] = (uint8_t)cp;
        l = 1;
    } else if (cp < 0x800) {
        b[0] = (uint8_t)(0xC0 | (cp >> 6));
        b[1] = (uint8_t)(0x80 | (cp & 63));
        l = 2;
    } else if (cp < 0x10000) {
        b[0] = (uint8_t)(0xE0 | (cp >> 12));
        b[1] = (uint8_t)(0x80 | ((cp >> 6) & 63));
        b[2] = (uint8_t)(0x80 | (cp & 63));
        l = 3;
    } else {
        b[0] = (uint8_t)(0xF0 | (cp >> 18));
        b[1] = (uint8_t)(0x80 | ((cp >> 12) & 63));
        b[2] = (uint8_t)(0x80 | ((cp >> 6) & 63));
        b[3] = (uint8_t)(0x80 | (cp & 63));
        l = 4;
    }
    if (s.out) {
        s.out[s.produced] = b[0];
        if (l > 1) s.out[s.produced + 1] = b[1];
        if (l > 2) s.out[s.produced + 2] = b[2];
        if (l > 3) s.out[s.produced + 3] = b[3];
    }
    s.produced += l;
}

// canonical order of the window's marks (a stable insertion sort by class), then the composition loop of
// unicode_norm.cpp's normalize_segment over the window; a window that starts with a mark composes nothing
__host__ __device__ inline void norm_finalize(const NormTables& t, NormStream& s, bool compose) {
    const uint32_t st = s.stride, first = s.n && s.cc[0] == 0 ? 1u : 0u;
    for (uint32_t x = first + 1; x < s.n; x++) {
        const uint32_t cv = s.cp[x * st];
        const uint8_t cc = s.cc[x * st];
        uint32_t y = x;
        while (y > first && s.cc[(y - 1) * st] > cc) {
            s.cp[y * st] = s.cp[(y - 1) * st];
            s.cc[y * st] = s.cc[(y - 1) * st];
            y--;
        }
        s.cp[y * st] = cv;
        s.cc[y * st] = cc;
    }
    if (!compose || s.n < 2 || !first) return;
    uint32_t starter = s.cp[0], last = 0, w = 1;
    for (uint32_t k = 1; k < s.n; k++) {
        const uint32_t ch = s.cp[k * st], cc = s.cc[k * st];
        const uint32_t comp = (last < cc || last == 0) ? norm_compose_pair(t, starter, ch) : 0u;
        if (comp) {
            starter = comp;
            continue;
        }
        last = cc;
        s.cp[w * st] = ch;
        s.cc[w * st] = (uint8_t)cc;
        w++;
    }
    s.cp[0] = starter;
    s.n = w;
}

__host__ __device__ inline void norm_flush(NormStream& s) {
    for (uint32_t k = 0; k < s.n; k++) norm_emit(s, s.cp[k * s.stride]);
    s.n = 0;
}

// one scalar of the decomposed stream
__host__ __device__ inline void norm_feed(const NormTables& t, NormStream& s, uint32_t x, bool compose) {
    const uint32_t cc = norm_ccc(t, x);
    if (cc) {
        if (s.n == kNormWindow) {
            s.overflow = true;
            return;
        }
        s.cp[s.n * s.stride] = x;
        s.cc[s.n * s.stride] = (uint8_t)cc;
        s.n++;
        return;
    }
    norm_finalize(t, s, compose);
    if (compose && s.n == 1 && s.cc[0] == 0) {  // a starter that took all its marks may take the next starter too
        const uint32_t comp = norm_compose_pair(t, s.cp[0], x);
        if (comp) {
            s.cp[0] = comp;
            return;
        }
    }
    norm_flush(s);
    s.cp[0] = x;
    s.cc[0] = 0;
    s.n = 1;
}

// The piece headed at `begin` of a row that ends at row_end: the head and the active units behind it go through the
// machine.  Returns where the piece ends.
__host__ __device__ inline uint64_t norm_run_piece(const NormTables& t, uint32_t form, const uint8_t* text, uint64_t begin, uint64_t row_end, NormStream& s) {
    const bool compose = form & 1u, compat = form & 2u;
    uint64_t i = begin;
    while (i < row_end) {
        uint64_t j = i;
        const uint32_t cp = norm_next(text, row_end, j);
        if (i != begin && !norm_active(t, form, cp)) break;
        i = j;
        const NormDecomp d = norm_decompose(t, cp, compat);
        for (uint32_t k = 0; k < d.n; k++) norm_feed(t, s, norm_decomp_at(d, k), compose);
    }
    norm_finalize(t, s, compose);
    norm_flush(s);
    return i;
}

// ---- index arithmetic ---------------------------------------------------------------------------------------------------

// A slot's masks: bits 0..15 the bytes that pieces cover, bits 16..31 the first bytes of heads.  v: the slot's bytes (0
// past the text's end), next: the byte after them (0 past the end).  lo, hi: the rows of the tile's first and last byte.
// Nothing at or after the end of a row is read for that row, so nothing at or after n_bytes is read at all.
__host__ __device__ inline uint32_t norm_mark_slot(const NormTables& t, uint32_t form, const uint8_t* text, const uint64_t* offs, uint64_t lo, uint64_t hi,
                                                   uint64_t p0, uint32_t n_in, const uint8_t (&v)[kFrontGroup], uint8_t next) {
    // most slots are ASCII and so is the byte behind them: no unit in them is active or stands in front of an active one
    uint32_t high = next & 0x80u;
#pragma unroll
    for (uint32_t j = 0; j < kFrontGroup; j += 4) high |= ((uint32_t)v[j] | (uint32_t)v[j + 1] | (uint32_t)v[j + 2] | (uint32_t)v[j + 3]) & 0x80u;
    if (!high) return 0;
    FrontCursor cur;
    front_advance(cur, offs, lo, hi, p0);
    // where the row's units are in step with the slot: p0, or the lead byte of the sequence that p0 lies inside (a byte
    // that is no continuation byte always starts a unit)
    uint64_t pos = p0;
    if ((v[0] & 0xC0u) == 0x80u) {
        const uint64_t begin = offs[cur.i];
        for (uint32_t k = 1; k <= 3 && p0 >= begin + k; k++)
            if ((text[p0 - k] & 0xC0u) != 0x80u) {
                uint64_t j = p0 - k;
                norm_next(text, cur.end, j);
                if (j > p0) pos = p0 - k;
                break;
            }
    }
    uint32_t cov = 0, head = 0;
    const uint64_t stop = p0 + n_in;
    bool carried = false, c_act = false;  // the unit behind the last one, when it lies in the same row
    uint64_t c_end = 0;
    while (pos < stop) {
        front_advance(cur, offs, lo, hi, pos);
        uint64_t a_end = pos;
        bool a_act = c_act;
        if (carried)
            a_end = c_end;
        else
            a_act = norm_active(t, form, norm_next(text, cur.end, a_end));
        carried = a_end < cur.end;
        if (carried) {
            c_end = a_end;
            c_act = norm_active(t, form, norm_next(text, cur.end, c_end));
        }
        const bool is_head = a_act ? pos == offs[cur.i] : (carried && c_act);
        if (a_act || is_head) {
            const uint32_t q0 = pos > p0 ? (uint32_t)(pos - p0) : 0u, q1 = (uint32_t)((a_end < stop ? a_end : stop) - p0);
            cov |= ((1u << q1) - 1u) & ~((1u << q0) - 1u);
            if (is_head && pos >= p0) head |= 1u << (pos - p0);
        }
        pos = a_end;
    }
    return cov | head << 16;
}

// the slot's bytes that are copied
__host__ __device__ inline uint32_t norm_verbatim(uint32_t mask, uint32_t n_in) { return ~mask & ((1u << n_in) - 1u); }

// The slot's pieces, written in position order from index at: where each begins and its row.
__host__ __device__ inline void norm_write_pieces(const uint64_t* offs, uint64_t lo, uint64_t hi, uint64_t p0, uint32_t heads, uint64_t at, uint64_t* piece_begin,
                                                  uint64_t* piece_row) {
    FrontCursor cur;
    for (uint32_t q = 0; heads >> q; q++) {
        if (!((heads >> q) & 1u)) continue;
        front_advance(cur, offs, lo, hi, p0 + q);
        piece_begin[at] = p0 + q;
        piece_row[at] = cur.i;
        at++;
    }
}

// What the places need: mask u32[slots] (norm_mark_slot), slot_pre u32[slots] (the copied bytes, bits 0..15, and the heads,
// bits 16..31, of the slot's tile in front of the slot), tile_base u64[tiles + 1] (pieces headed before each tile),
// piece_sum u64[P + 1] (bytes of the pieces before each) and tile_place u64[tiles + 1] (output bytes before each tile).
struct NormPlaces {
    const uint32_t *mask, *slot_pre;
    const uint64_t *tile_base, *piece_sum, *tile_place;
};

// what a tile turns into: its copied bytes and the bytes of the pieces headed in it
__host__ __device__ inline uint64_t norm_tile_bytes(const uint64_t* tile_base, const uint64_t* piece_sum, uint64_t tile, uint32_t copied) {
    return copied + (piece_sum[tile_base[tile + 1]] - piece_sum[tile_base[tile]]);
}

// Where byte p < N goes when it is copied or starts a head: behind what its tile's earlier copied bytes and earlier
// pieces turn into.  A row's first byte is always one of the two, as pieces do not cross rows.
__host__ __device__ inline uint64_t norm_place(const NormPlaces& pl, uint64_t p) {
    const uint64_t tile = p / kFrontTile, slot = p / kFrontGroup, pb = pl.tile_base[tile];
    const uint32_t m = pl.mask[slot], pre = pl.slot_pre[slot], below = (1u << (p % kFrontGroup)) - 1u;
    const uint32_t copied = (pre & 0xFFFFu) + front_popc(~m & below), heads = (pre >> 16) + front_popc((m >> 16) & below);
    return pl.tile_place[tile] + copied + (pl.piece_sum[pb + heads] - pl.piece_sum[pb]);
}

// the slot's copied bytes to their places
__host__ __device__ inline void norm_copy_slot(const NormPlaces& pl, uint64_t p0, uint32_t n_in, const uint8_t (&v)[kFrontGroup], uint8_t* out) {
    const uint64_t tile = p0 / kFrontTile, slot = p0 / kFrontGroup, pb = pl.tile_base[tile];
    const uint32_t m = pl.mask[slot], pre = pl.slot_pre[slot], copy = norm_verbatim(m, n_in);
    if (!copy) return;
    uint64_t heads = pb + (pre >> 16);
    uint64_t at = pl.tile_place[tile] + (pre & 0xFFFFu) + (pl.piece_sum[heads] - pl.piece_sum[pb]);
#pragma unroll
    for (uint32_t q = 0; q < kFrontGroup; q++) {
        if ((m >> (16 + q)) & 1u) {  // the bytes behind a head also stand behind its piece
            at += pl.piece_sum[heads + 1] - pl.piece_sum[heads];
            heads++;
        }
        if ((copy >> q) & 1u) out[at++] = v[q];
    }
}

// ---- launchers (norm.hip) -----------------------------------------------------------------------------------------------

struct NormParams {
    const uint8_t* text;   // as FrontParams::text
    const uint64_t* offs;  // u64[S + 1]
    uint64_t n_bytes, n_rows;
    uint32_t form;
    NormTables tab;        // device memory
    uint32_t *mask, *slot_pre;            // u32[slots] each
    uint64_t *tile_count, *tile_base;     // u64[tiles + 1]: heads per tile and their exclusive sums; tile_base[tiles] = P
    uint64_t *tile_bytes, *tile_place;    // u64[tiles + 1]: output bytes per tile and their exclusive sums
    uint64_t n_pieces;
    uint64_t *piece_begin, *piece_row;    // u64[P]
    uint64_t *piece_len, *piece_sum;      // u64[P + 1]: bytes every piece turns into (entry P is 0) and their exclusive sums
    uint64_t* overflow_row;               // u64[1]: the lowest row whose window overflowed, or kNormNoRow
    uint64_t* out_offs;                   // u64[S + 1]
    uint8_t* out;
};

hipError_t norm_scan_temp_bytes(uint64_t n, size_t* bytes);  // for every scan below over up to n elements
hipError_t launch_norm_mark(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream);    // mask, tile_base
hipError_t launch_norm_pieces(const NormParams& p, hipStream_t stream);                                  // piece_begin, piece_row
hipError_t launch_norm_length(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream);  // piece_len, piece_sum, overflow_row
hipError_t launch_norm_places(const NormParams& p, void* temp, size_t temp_bytes, hipStream_t stream);  // slot_pre, tile_place, out_offs
hipError_t launch_norm_write(const NormParams& p, hipStream_t stream);                                   // out

}  // namespace tgx
