// Index arithmetic of the decode of ids to UTF-8 text (include/tgx.h: tgx_decode_result, tgx_decode_padded).  The kernels
// of decode.hip and the host twin in host_twins.cpp (tgx_decode_rows_host) both go through these functions, so a machine
// without a GPU checks the kernels' arithmetic: liveness and classes of an element, the walk of a thread slot over the
// elements that cover its 16 output bytes, and String::from_utf8_lossy as a rule that looks at most 3 bytes to either
// side of a byte inside its run.
//
// Element j of N owns the raw bytes [B[j], B[j+1]): a base token's bytes, a special token's (when they are included) or
// none (not live, an empty token, an excluded special).  X[j] = live specials before j, so element j is a special iff
// X[j+1] != X[j] and a special lies in [j', j) iff X[j] != X[j'] (X == NULL: the stream has no live special, and nothing
// is read for it).  Per 16 raw bytes one flag word: bit q = a run of
// base tokens (or a special token) starts at byte q, bit 16 + q = byte q is a special token's and goes out verbatim.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kDecodeGroup = 16;    // consecutive raw bytes of a thread slot: one 16-byte store
constexpr uint32_t kDecodeTile = 4096;   // raw bytes per tile: the fill kernel's block of 256 threads x 16 bytes
constexpr uint32_t kDecodeSlotLen = 16;  // tokens of up to this many bytes are read from their 16-byte slot
constexpr uint32_t kDecodeSpecial = 0x80000000u;  // meta word: the element is a live special token (low 31 bits: raw length)
constexpr uint32_t kDecodeU32 = 0, kDecodeI32 = 1, kDecodeI64 = 2;  // element types

struct alignas(16) DecodeSlot {
    uint64_t lo, hi;  // a token's bytes, first byte lowest
};

// the vocabulary and the special tokens (device memory for the kernels, host memory for the twin)
struct DecodeTables {
    const uint8_t* tok_len;    // u8[V]
    const DecodeSlot* slots;   // [V]: the bytes of tokens of <= kDecodeSlotLen bytes
    const uint8_t* bytes;      // the tokens back to back ...
    const uint64_t* offs;      // ... u64[V+1]
    const uint8_t* sp_bytes;   // the special tokens back to back ...
    const uint64_t* sp_offs;   // ... u64[n_specials+1]
    uint32_t vocab_size, n_specials;
    int include_special;
};

// the id stream: S rows, in the offsets form (offs != NULL: u32 ids, row i = [offs[i], offs[i+1])) or the padded form
// (row i = [i·row_len, (i+1)·row_len), liveness by mask / lengths / skip_id)
struct DecodeSrc {
    const void* ids;
    const uint64_t* offs;
    const uint8_t* mask;
    const int32_t* lengths;
    uint64_t n_rows, row_len, n;  // n: elements
    uint32_t kind;                // kDecodeU32 / kDecodeI32 / kDecodeI64
    uint32_t skip_id;             // 0xFFFFFFFF: none
};

__host__ __device__ inline int64_t decode_elem(const DecodeSrc& s, uint64_t j) {
    if (s.kind == kDecodeI64) return static_cast<const int64_t*>(s.ids)[j];
    if (s.kind == kDecodeI32) return static_cast<const int32_t*>(s.ids)[j];
    return static_cast<const uint32_t*>(s.ids)[j];
}

__host__ __device__ inline bool decode_live(const DecodeSrc& s, uint64_t j, int64_t x) {
    if (s.offs) return true;
    if (s.mask && s.mask[j] == 0) return false;
    if (s.lengths) {
        const uint64_t i = j / s.row_len;
        const int32_t n = s.lengths[i];
        if (n <= 0 || j - i * s.row_len >= (uint64_t)n) return false;
    }
    return s.skip_id == 0xFFFFFFFFu || x != (int64_t)s.skip_id;
}

// the meta word of a live element of value x: its raw length, with kDecodeSpecial for a special token; *oob: x is neither
__host__ __device__ inline uint32_t decode_meta(const DecodeTables& t, int64_t x, bool* oob) {
    *oob = false;
    if (x >= 0 && x < (int64_t)t.vocab_size) return t.tok_len[x];
    const int64_t k = x - (int64_t)t.vocab_size;
    if (x >= 0 && k < (int64_t)t.n_specials)
        return kDecodeSpecial | (t.include_special ? (uint32_t)(t.sp_offs[k + 1] - t.sp_offs[k]) : 0u);
    *oob = true;
    return 0;
}

// the first element of row i <= S
__host__ __device__ inline uint64_t decode_row_first(const DecodeSrc& s, uint64_t i) { return s.offs ? s.offs[i] : i * s.row_len; }

// The element that owns raw byte b is the LARGEST j with B[j] <= b (pack_find_row of tile_fill.h over B with A = 0), so
// elements without bytes are stepped over.

// the owner of byte b >= B[j+1], which is the next element whenever that one has bytes
__host__ __device__ inline uint64_t decode_step(const uint64_t* B, uint64_t j, uint64_t hi, uint64_t b) {
    return B[j + 2] > b ? j + 1 : pack_find_row(B, 0, j + 2, hi, b);
}

// The owners that bound the searches of a tile are those of the byte before it and of its last byte (tile_first with
// kDecodeBack, tile_last): a slot asks who owns the byte before its first one.
constexpr uint32_t kDecodeBack = 1;

// the element a slot's walk stands on
struct DecodeCursor {
    uint64_t j, start, next;  // the element and its raw bytes [start, next)
    uint64_t x;               // X[j]
    bool special;
    const uint8_t* ptr;       // its bytes when they are not in `slot`
    DecodeSlot slot;
};

__host__ __device__ inline void decode_enter(DecodeCursor& c, const DecodeTables& t, const DecodeSrc& s, const uint64_t* B, const uint64_t* X,
                                             uint64_t j) {
    c.j = j;
    c.start = B[j];
    c.next = B[j + 1];
    c.x = X ? X[j] : 0;
    c.special = X ? X[j + 1] != c.x : false;
    const uint64_t id = (uint64_t)decode_elem(s, j);  // an element with bytes is live and in range
    c.ptr = nullptr;
    c.slot.lo = c.slot.hi = 0;
    if (c.special)
        c.ptr = t.sp_bytes + t.sp_offs[id - t.vocab_size];
    else if (c.next - c.start <= kDecodeSlotLen)
        c.slot = t.slots[id];
    else
        c.ptr = t.bytes + t.offs[id];
}

__host__ __device__ inline uint8_t decode_byte(const DecodeCursor& c, uint64_t b) {
    const uint64_t k = b - c.start;
    if (c.ptr) return c.ptr[k];
    return (uint8_t)(k < 8 ? c.slot.lo >> (8 * k) : c.slot.hi >> (8 * (k - 8)));
}

// A thread slot's walk: v[q] = raw byte e0 + q for q < n_in <= kDecodeGroup -> the slot's flag word.  lo / hi: the owners
// of tile_first (kDecodeBack) / tile_last of the slot's tile.
__host__ __device__ inline uint32_t decode_group(const DecodeTables& t, const DecodeSrc& s, const uint64_t* B, const uint64_t* X, uint64_t lo,
                                                 uint64_t hi, uint64_t e0, uint32_t n_in, uint8_t (&v)[kDecodeGroup]) {
    DecodeCursor c;
    decode_enter(c, t, s, B, X, pack_find_row(B, 0, lo, hi, e0));
    // X of the owner of the byte before the one looked at: a special in between (or that owner itself) ends a run
    uint64_t xprev = c.x;
    if (X && e0 == c.start && e0 > 0) xprev = X[pack_find_row(B, 0, lo, c.j - 1, e0 - 1)];
    uint32_t flags = 0;
#pragma unroll
    for (uint32_t q = 0; q < kDecodeGroup; q++) {
        if (q < n_in) {
            const uint64_t b = e0 + q;
            if (b >= c.next) {
                xprev = c.x;
                decode_enter(c, t, s, B, X, decode_step(B, c.j, hi, b));
            }
            if (b == c.start && (c.special || c.x != xprev || b == 0)) flags |= 1u << q;
            if (c.special) flags |= 0x10000u << q;
            v[q] = decode_byte(c, b);
        }
    }
    return flags;
}

// ---- String::from_utf8_lossy, byte by byte -------------------------------------------------------------------------
// A window of kDecodeWindow bytes: w[3 + q] = raw byte e0 + q of a slot, three bytes to either side.  `start`: bit i =
// a run starts at w[i] (the end of the text counts as one), so nothing is read across such a bit and a byte outside
// the text is never looked at.

constexpr uint32_t kDecodeWindow = kDecodeGroup + 6;

// the window's bytes in three words (registers on the device: a byte array indexed by a variable would live in scratch)
struct DecodeWin {
    uint64_t a = 0, b = 0, c = 0;  // w[0..8), w[8..16), w[16..22)
    __host__ __device__ uint8_t operator[](uint32_t i) const {
        return (uint8_t)(i < 8 ? a >> (8 * i) : i < 16 ? b >> (8 * (i - 8)) : c >> (8 * (i - 16)));
    }
    // own: the slot's 16 bytes (first byte lowest), before / after: the three bytes to either side (first byte lowest)
    __host__ __device__ static DecodeWin of(uint32_t before, uint64_t own_lo, uint64_t own_hi, uint32_t after) {
        DecodeWin w;
        w.a = (uint64_t)(before & 0xFFFFFFu) | (own_lo << 24);
        w.b = (own_lo >> 40) | (own_hi << 24);
        w.c = (own_hi >> 40) | ((uint64_t)(after & 0xFFFFFFu) << 24);
        return w;
    }
};

__host__ __device__ inline bool decode_is_cont(uint8_t c) { return (c & 0xC0u) == 0x80u; }

// sub(q) of a byte that is no continuation byte: the bytes it consumes; *valid: they are one well-formed character
__host__ __device__ inline uint32_t decode_sub(const DecodeWin& w, uint32_t start, uint32_t q, bool* valid) {
    const uint8_t c = w[q];
    *valid = c < 0x80u;
    if (c < 0xC2u || c > 0xF4u) return 1;  // ASCII; C0, C1, F5..FF
    const uint32_t need = c < 0xE0u ? 2 : c < 0xF0u ? 3 : 4;
    uint8_t lo2 = 0x80u, hi2 = 0xBFu;
    if (c == 0xE0u) lo2 = 0xA0u;
    if (c == 0xEDu) hi2 = 0x9Fu;
    if (c == 0xF0u) lo2 = 0x90u;
    if (c == 0xF4u) hi2 = 0x8Fu;
    uint32_t k = 1;
    for (; k < need; k++) {
        if ((start >> (q + k)) & 1u) break;
        const uint8_t d = w[q + k];
        if (k == 1 ? (d < lo2 || d > hi2) : !decode_is_cont(d)) break;
    }
    *valid = k == need;
    return k;
}

// output bytes of w[i], 3 <= i < 3 + kDecodeGroup: 0, 1 or 3 (the replacement character)
__host__ __device__ inline uint32_t decode_contrib(const DecodeWin& w, uint32_t start, uint32_t i) {
    bool valid;
    if (!decode_is_cont(w[i])) {
        decode_sub(w, start, i, &valid);
        return valid ? 1 : 3;
    }
    for (uint32_t d = 1; d <= 3; d++) {
        if ((start >> (i - d + 1)) & 1u) break;  // w[i - d] belongs to another run
        if (decode_is_cont(w[i - d])) continue;
        if (decode_sub(w, start, i - d, &valid) > d) return valid ? 1 : 0;
        break;
    }
    return 3;  // a stray continuation byte
}

// the slot's code word: 2 bits per byte, its output bytes.  verbatim: bit q = byte q is a special token's.
__host__ __device__ inline uint32_t decode_utf8_group(const DecodeWin& w, uint32_t start, uint32_t verbatim, uint32_t n_in) {
    uint32_t code = 0;
#pragma unroll
    for (uint32_t q = 0; q < kDecodeGroup; q++)
        if (q < n_in) code |= ((verbatim >> q) & 1u ? 1u : decode_contrib(w, start, 3 + q)) << (2 * q);
    return code;
}

__host__ __device__ inline uint32_t decode_popc(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
// output bytes of the first r <= 16 bytes of a slot / replacement characters of a slot
__host__ __device__ inline uint32_t decode_code_bytes(uint32_t code, uint32_t r) {
    if (r < kDecodeGroup) code &= (1u << (2 * r)) - 1u;
    return decode_popc(code & 0x55555555u) + 2 * decode_popc(code & 0xAAAAAAAAu);
}
__host__ __device__ inline uint32_t decode_code_replaced(uint32_t code) { return decode_popc(code & 0xAAAAAAAAu); }

// the start bits of a slot's window from the flag words of the slot before it, its own and the one after it (0 where
// there is none), with the end of the text: e0 = the slot's first raw byte, n_raw = the text's length
__host__ __device__ inline uint32_t decode_window_starts(uint32_t f_prev, uint32_t f_own, uint32_t f_next, uint64_t e0, uint64_t n_raw) {
    uint32_t start = ((f_prev >> 13) & 7u) | ((f_own & 0xFFFFu) << 3) | ((f_next & 7u) << 19);
    if (n_raw - e0 < kDecodeGroup + 3) start |= 1u << (uint32_t)(n_raw - e0 + 3);
    return start;
}

// the 16 bytes of the slot at p (16-byte aligned; the buffer is padded to whole slots), first byte lowest
__host__ __device__ inline void decode_load_slot(const uint8_t* p, uint64_t* lo, uint64_t* hi) {
    uint64_t w[2];
    __builtin_memcpy(w, __builtin_assume_aligned(p, 16), 16);
    *lo = w[0];
    *hi = w[1];
}

// The code word of slot g of the raw text: its window is put together from the text and the flag words, unless all of its
// bytes are ASCII, which go out as they are whatever surrounds them.
__host__ __device__ inline uint32_t decode_utf8_slot(const uint8_t* raw, const uint32_t* flags, uint64_t n_raw, uint64_t g) {
    const uint64_t e0 = g * kDecodeGroup, n_groups = (n_raw + kDecodeGroup - 1) / kDecodeGroup;
    const uint32_t n_in = n_raw - e0 < kDecodeGroup ? (uint32_t)(n_raw - e0) : kDecodeGroup;
    uint64_t lo, hi;
    decode_load_slot(raw + e0, &lo, &hi);
    if (n_in < kDecodeGroup) {  // what lies behind the text is not looked at, but may be anything
        if (n_in <= 8) {
            hi = 0;
            if (n_in < 8) lo &= (1ull << (8 * n_in)) - 1ull;
        } else {
            hi &= (1ull << (8 * (n_in - 8))) - 1ull;
        }
    }
    if (((lo | hi) & 0x8080808080808080ull) == 0) return (n_in < kDecodeGroup ? (1u << (2 * n_in)) - 1u : ~0u) & 0x55555555u;
    uint32_t before = 0, after = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        if (e0) before |= (uint32_t)raw[e0 - 3 + k] << (8 * k);
        if (e0 + kDecodeGroup + k < n_raw) after |= (uint32_t)raw[e0 + kDecodeGroup + k] << (8 * k);
    }
    const DecodeWin w = DecodeWin::of(before, lo, hi, after);
    const uint32_t f_own = flags[g];
    const uint32_t start = decode_window_starts(g ? flags[g - 1] : 0, f_own, g + 1 < n_groups ? flags[g + 1] : 0, e0, n_raw);
    return decode_utf8_group(w, start, f_own >> 16, n_in);
}

// final position of raw byte r <= n_raw: gpos = the scanned output bytes of the slots (gpos[G] = all of them)
__host__ __device__ inline uint64_t decode_final_pos(const uint64_t* gpos, const uint32_t* codes, uint64_t r, uint64_t n_raw) {
    if (r >= n_raw) return gpos[(n_raw + kDecodeGroup - 1) / kDecodeGroup];
    return gpos[r / kDecodeGroup] + decode_code_bytes(codes[r / kDecodeGroup], (uint32_t)(r % kDecodeGroup));
}

// the output of slot g: its raw bytes with code word `code`, written from out[pos] on
__host__ __device__ inline void decode_expand_slot(const uint8_t* raw, uint64_t n_raw, uint64_t g, uint32_t code, uint8_t* out, uint64_t pos) {
    const uint64_t e0 = g * kDecodeGroup;
    const uint32_t n_in = n_raw - e0 < kDecodeGroup ? (uint32_t)(n_raw - e0) : kDecodeGroup;
    uint64_t lo, hi;
    decode_load_slot(raw + e0, &lo, &hi);
    for (uint32_t q = 0; q < n_in; q++) {
        const uint32_t c = (code >> (2 * q)) & 3u;
        if (c == 1) {
            out[pos++] = (uint8_t)(q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8)));
        } else if (c == 3) {
            out[pos++] = 0xEFu;
            out[pos++] = 0xBFu;
            out[pos++] = 0xBDu;
        }
    }
}

}  // namespace tgx
