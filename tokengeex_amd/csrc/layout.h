// Row mapping of the padded, packed and windowed layouts of a result (include/tgx.h: tgx_result_pad_device,
// tgx_result_pack_device, tgx_result_window_pad_device).  The kernels of layout.hip and the host twins in host_twins.cpp
// (tgx_layout_pad_host, tgx_layout_pack_host, tgx_layout_windows_host) both go through these functions, so a machine
// without a GPU checks the kernels' index arithmetic.
//
// Row i has the tokens ids[offs[i] .. offs[i+1]); offs[0] = 0.  A = how many of bos / eos are present.  A written
// sequence is [bos] + kept tokens + [eos].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_fill.h"

namespace tgx {

constexpr uint32_t kLayoutNoId = 0xFFFFFFFFu;    // TGX_NO_ID
constexpr uint32_t kLayoutPadLeft = 1u;          // TGX_LAYOUT_PAD_LEFT
constexpr uint32_t kLayoutTruncLeft = 2u;        // TGX_LAYOUT_TRUNC_LEFT
constexpr uint32_t kLayoutI64 = 4u;              // TGX_LAYOUT_I64

struct LayoutSeq {
    uint32_t bos, eos, pad;
    uint32_t has_bos;  // 0 / 1
    uint32_t extra;    // A
};

__host__ __device__ inline LayoutSeq layout_seq(uint32_t bos, uint32_t eos, uint32_t pad) {
    LayoutSeq s;
    s.bos = bos;
    s.eos = eos;
    s.pad = pad;
    s.has_bos = bos != kLayoutNoId ? 1u : 0u;
    s.extra = s.has_bos + (eos != kLayoutNoId ? 1u : 0u);
    return s;
}

// element q of [bos] + ids[src .. src + keep) + [eos], q < keep + A
__host__ __device__ inline uint32_t layout_seq_at(const LayoutSeq& s, const uint32_t* ids, uint64_t src, uint64_t keep, uint64_t q) {
    if (s.has_bos && q == 0) return s.bos;
    const uint64_t k = q - s.has_bos;
    return k < keep ? ids[src + k] : s.eos;
}

// ---- padded: out[i, c], c < L ------------------------------------------------------------------------------
struct PadRow {
    uint64_t src;    // first kept token in ids
    uint32_t keep;   // kept tokens: min(n_i, L - A)
    uint32_t len;    // keep + A
    uint32_t col0;   // column of the sequence's first element
    uint32_t truncated;
};

// L >= 1 and L >= A (checked by the callers)
__host__ __device__ inline PadRow pad_row(const uint64_t* offs, uint64_t i, uint32_t L, const LayoutSeq& s, uint32_t flags) {
    const uint64_t b = offs[i], n = offs[i + 1] - b;
    const uint32_t room = L - s.extra;
    PadRow r;
    r.keep = n < room ? (uint32_t)n : room;
    r.src = b + ((flags & kLayoutTruncLeft) ? n - r.keep : 0);
    r.len = r.keep + s.extra;
    r.col0 = (flags & kLayoutPadLeft) ? L - r.len : 0;
    r.truncated = n > room ? 1u : 0u;
    return r;
}

// the id at column c of the row; returns the mask bit (1 on the sequence, 0 on padding)
__host__ __device__ inline uint32_t pad_at(const LayoutSeq& s, const PadRow& r, const uint32_t* ids, uint32_t c, uint32_t* id) {
    const uint32_t q = c - r.col0;  // wraps to a large value left of the sequence
    if (q >= r.len) {
        *id = s.pad;
        return 0;
    }
    *id = layout_seq_at(s, ids, r.src, r.keep, q);
    return 1;
}

// A thread slot's walk: n_in <= kLayoutGroup consecutive elements of the flat [S, L] output from element e0 on, which
// may run over the end of a row into the next ones.  v[k] gets the id of element e0 + k, the return value its mask
// bit in byte k.  The slot that holds a row's first column speaks for the row: it writes lengths[i] (when wanted)
// and adds the row to *truncated.
constexpr uint32_t kLayoutGroup = 4;
__host__ __device__ inline uint32_t pad_group(const LayoutSeq& s, const uint32_t* ids, const uint64_t* offs, uint32_t L, uint32_t flags,
                                              uint64_t e0, uint32_t n_in, int32_t* lengths, uint32_t (&v)[kLayoutGroup],
                                              unsigned long long* truncated) {
    uint64_t i = e0 / L;
    uint32_t c = (uint32_t)(e0 - i * L);
    PadRow row = pad_row(offs, i, L, s, flags);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLayoutGroup; k++) {
        if (k < n_in) {
            if (c == 0) {
                if (lengths) lengths[i] = (int32_t)row.len;
                *truncated += row.truncated;
            }
            m |= pad_at(s, row, ids, c, &v[k]) << (8 * k);
            if (++c == L) {
                c = 0;
                i++;
                if (k + 1 < n_in) row = pad_row(offs, i, L, s, flags);
            }
        }
    }
    return m;
}

// ---- packed: stream position j < n_stream = T + S·A -----------------------------------------------------------
// row i starts at P_i = offs[i] + i·A (P_S = n_stream): pack_row_start and pack_find_row of tile_fill.h

// A walk over ascending stream positions that all lie between the positions owned by rows lo and hi (a tile's first
// and last): the first position searches [lo, hi], a later one stays on its row until the next row's start and then
// searches from the row after it.
constexpr uint32_t kPackTile = 1024;  // positions per tile: the kernel's block of 256 threads x 4 elements
struct PackCursor {
    uint64_t i = 0, next = 0;  // the current row and P_{i+1}
    bool have = false;
};
__host__ __device__ inline uint64_t pack_advance(PackCursor& cur, const uint64_t* offs, uint64_t A, uint64_t lo, uint64_t hi, uint64_t j) {
    if (!cur.have || j >= cur.next) {
        cur.i = pack_find_row(offs, A, cur.have ? cur.i + 1 : lo, hi, j);
        cur.next = pack_row_start(offs, A, cur.i + 1);
        cur.have = true;
    }
    return cur.i;
}

// the id at stream position j, which row i owns; *pos = j - P_i
__host__ __device__ inline uint32_t pack_at(const LayoutSeq& s, const uint32_t* ids, const uint64_t* offs, uint64_t i, uint64_t j,
                                            int32_t* pos) {
    const uint64_t b = offs[i], q = j - (b + i * s.extra);
    *pos = (int32_t)q;
    return layout_seq_at(s, ids, b, offs[i + 1] - b, q);
}

// ---- windows: out[w, c], w < W, c < L: a long row as overlapping windows (tgx_result_window_pad_device) -------------
// room = L - A >= 1 tokens per window, of which stride < room repeat the window before: step = room - stride >= 1.
__host__ __device__ inline uint64_t window_count(uint64_t n, uint32_t room, uint32_t step) {
    return n <= room ? 1 : 1 + (n - room + step - 1) / step;
}

struct WinRow {
    PadRow p;        // the window as a padded row: src, keep, len, col0 (truncated: the row has more than one window)
    uint32_t first;  // index of the first kept token in its row
};

// Window w of row i, which owns it: Wo[i] <= w < Wo[i+1], Wo = the exclusive prefix sums of window_count.  Window
// k = w - Wo[i] keeps the row's tokens [k·step, min(n, k·step + room)), counted from the row's end with
// kLayoutTruncLeft.  k·step < n for k >= 1, so every window keeps a token unless the row is empty.
__host__ __device__ inline WinRow win_row(const uint64_t* offs, const uint64_t* Wo, uint64_t i, uint64_t w, uint32_t L, const LayoutSeq& s,
                                          uint32_t stride, uint32_t flags) {
    const uint64_t b = offs[i], n = offs[i + 1] - b;
    const uint32_t room = L - s.extra, step = room - stride;
    const uint64_t lo = (w - Wo[i]) * step;
    const uint64_t hi = n - lo < room ? n : lo + room;
    const uint64_t first = (flags & kLayoutTruncLeft) ? n - hi : lo;
    WinRow r;
    r.p.keep = (uint32_t)(hi - lo);
    r.p.src = b + first;
    r.p.len = r.p.keep + s.extra;
    r.p.col0 = (flags & kLayoutPadLeft) ? L - r.p.len : 0;
    r.p.truncated = n > room ? 1u : 0u;
    r.first = (uint32_t)first;
    return r;
}

// A thread slot's walk over n_in <= kLayoutGroup consecutive elements of the flat [W, L] output from element e0 on, as
// pad_group's.  lo / hi: the rows that own the first and last window of the slot's tile (pack_find_row over Wo with
// A = 0: Wo is strictly increasing); a row cursor steps from window to window.  The slot that holds a window's first
// column writes lengths[w], window_row[w] and window_first[w] (each when wanted).
__host__ __device__ inline uint32_t win_group(const LayoutSeq& s, const uint32_t* ids, const uint64_t* offs, const uint64_t* Wo, uint32_t L,
                                              uint32_t stride, uint32_t flags, uint64_t lo, uint64_t hi, uint64_t e0, uint32_t n_in,
                                              int32_t* lengths, int32_t* window_row, int32_t* window_first, uint32_t (&v)[kLayoutGroup]) {
    uint64_t w = e0 / L;
    uint32_t c = (uint32_t)(e0 - w * L);
    PackCursor cur;
    uint64_t i = pack_advance(cur, Wo, 0, lo, hi, w);
    WinRow row = win_row(offs, Wo, i, w, L, s, stride, flags);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLayoutGroup; k++) {
        if (k < n_in) {
            if (c == 0) {
                if (lengths) lengths[w] = (int32_t)row.p.len;
                if (window_row) window_row[w] = (int32_t)i;
                if (window_first) window_first[w] = (int32_t)row.first;
            }
            m |= pad_at(s, row.p, ids, c, &v[k]) << (8 * k);
            if (++c == L) {
                c = 0;
                w++;
                if (k + 1 < n_in) {
                    i = pack_advance(cur, Wo, 0, lo, hi, w);
                    row = win_row(offs, Wo, i, w, L, s, stride, flags);
                }
            }
        }
    }
    return m;
}

}  // namespace tgx
