// Index arithmetic of the fill-in-the-middle rearrangement of a result's rows (include/tgx.h: tgx_result_fim).  The
// kernels of fim.hip and the host twin in host_twins.cpp (tgx_fim_host) both go through these functions, so a machine
// without a GPU checks the kernels' index arithmetic.
//
// Row i of S has the tokens t[0..n); g = first_row + i is its index in the whole batch.  What happens to it is a pure
// function of (seed, g, n): fim_row.  A rearranged row has n + 3 tokens, the pieces prefix = t[0:a), middle = t[a:b),
// suffix = t[b:n) behind the three sentinels; fim_source maps a position of the output row to a sentinel or to an index
// of the input row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace tgx {

constexpr uint64_t kFimSalt = 0xA0761D6478BD642FULL;  // TGX_FIM_SALT
constexpr uint32_t kFimGroup = 4;                     // consecutive positions of a thread slot: one 16-byte store
constexpr uint32_t kFimTile = kPackTile;              // positions per tile: the kernel's block of 256 threads x 4 positions
constexpr uint32_t kFimCopy = 0, kFimPsm = 1, kFimSpm = 2;  // a row's mode

// tgx_fim_u01
__host__ __device__ inline double fim_u01(uint64_t seed, uint64_t row, uint64_t draw) {
    uint64_t x = seed ^ kFimSalt ^ (row * 0x9E3779B97F4A7C15ULL) ^ (draw * 0xC2B2AE3D27D4EB4FULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// is row g, of n tokens, rearranged?  (what the lengths' scan needs: one hash)
__host__ __device__ inline bool fim_applies(uint64_t seed, uint64_t g, uint64_t n, double rate) {
    return n >= 1 && fim_u01(seed, g, 0) < rate;
}

// tokens of the output row
__host__ __device__ inline uint64_t fim_out_len(uint64_t seed, uint64_t g, uint64_t n, double rate) {
    return n + (fim_applies(seed, g, n, rate) ? 3u : 0u);
}

// a cut of a row of n >= 1 tokens: min(n, (u64)(u · (n + 1))), the product and the conversion in plain IEEE f64 (one
// multiplication: nothing for the compiler to contract)
__host__ __device__ inline uint64_t fim_cut(uint64_t seed, uint64_t g, uint64_t n, uint64_t draw) {
    const uint64_t c = (uint64_t)(fim_u01(seed, g, draw) * (double)(n + 1));
    return c < n ? c : n;
}

struct FimRow {
    uint32_t mode;  // kFimCopy / kFimPsm / kFimSpm
    uint64_t a, b;  // the cuts, a <= b <= n; (0, 0) for a copied row
};

// the single statement of what happens to row g
__host__ __device__ inline FimRow fim_row(uint64_t seed, uint64_t g, uint64_t n, double rate, double spm_rate) {
    FimRow r;
    r.mode = kFimCopy;
    r.a = r.b = 0;
    if (!fim_applies(seed, g, n, rate)) return r;
    r.mode = fim_u01(seed, g, 1) < spm_rate ? kFimSpm : kFimPsm;
    const uint64_t c2 = fim_cut(seed, g, n, 2), c3 = fim_cut(seed, g, n, 3);
    r.a = c2 < c3 ? c2 : c3;
    r.b = c2 < c3 ? c3 : c2;
    return r;
}

// Position t of the output row (t < n + 3 for a rearranged row, t < n for a copied one) -> an index of the input row, or
// one of the three sentinels.
//   PSM: PRE prefix SUF suffix MID middle        SPM: PRE SUF suffix MID prefix middle
constexpr uint64_t kFimSrcPre = ~0ull, kFimSrcSuf = ~0ull - 1, kFimSrcMid = ~0ull - 2;
__host__ __device__ inline uint64_t fim_source(uint32_t mode, uint64_t n, uint64_t a, uint64_t b, uint64_t t) {
    if (mode == kFimCopy) return t;
    if (t == 0) return kFimSrcPre;
    const uint64_t ns = n - b;  // the suffix
    if (mode == kFimPsm) {
        if (t <= a) return t - 1;  // prefix
        if (t == a + 1) return kFimSrcSuf;
        if (t < a + 2 + ns) return b + (t - (a + 2));  // suffix
        if (t == a + 2 + ns) return kFimSrcMid;
        return a + (t - (a + 3 + ns));  // middle
    }
    if (t == 1) return kFimSrcSuf;
    if (t < 2 + ns) return b + (t - 2);  // suffix
    if (t == 2 + ns) return kFimSrcMid;
    return t - (3 + ns);  // prefix, then middle: t[0:a) and t[a:b) lie back to back
}

// A walk over ascending output positions that all lie between the positions owned by rows lo and hi (a tile's first and
// last), as PackCursor's over the new offsets: the first position searches [lo, hi], a later one stays on its row until
// the next row's start and then searches from the row after it.  What does not change inside a row is computed when the
// cursor enters it: four hashes.
struct FimArgs {
    uint64_t seed, first_row;
    double rate, spm_rate;
    uint32_t pre, suf, mid;
};
struct FimCursor {
    uint64_t i = 0, next = 0;     // the current row and out_offs[i + 1]
    uint64_t start = 0, src = 0;  // out_offs[i] and offs[i]
    uint64_t n = 0;
    FimRow row = {kFimCopy, 0, 0};
    bool have = false;
};

// the id at output position j < T'
__host__ __device__ inline uint32_t fim_at(FimCursor& cur, const FimArgs& f, const uint32_t* ids, const uint64_t* offs, const uint64_t* out_offs,
                                           uint64_t lo, uint64_t hi, uint64_t j) {
    if (!cur.have || j >= cur.next) {
        cur.i = pack_find_row(out_offs, 0, cur.have ? cur.i + 1 : lo, hi, j);
        cur.start = out_offs[cur.i];
        cur.next = out_offs[cur.i + 1];
        cur.src = offs[cur.i];
        cur.n = offs[cur.i + 1] - cur.src;
        cur.row = fim_row(f.seed, f.first_row + cur.i, cur.n, f.rate, f.spm_rate);
        cur.have = true;
    }
    const uint64_t s = fim_source(cur.row.mode, cur.n, cur.row.a, cur.row.b, j - cur.start);
    if (s == kFimSrcPre) return f.pre;
    if (s == kFimSrcSuf) return f.suf;
    if (s == kFimSrcMid) return f.mid;
    return ids[cur.src + s];
}

// A thread slot's walk: v[q] = the id at position e0 + q for q < n_in <= kFimGroup.  lo / hi: the owners of the first
// and last position of the slot's tile.
__host__ __device__ inline void fim_group(const FimArgs& f, const uint32_t* ids, const uint64_t* offs, const uint64_t* out_offs, uint64_t lo,
                                          uint64_t hi, uint64_t e0, uint32_t n_in, uint32_t (&v)[kFimGroup]) {
    FimCursor cur;
#pragma unroll
    for (uint32_t q = 0; q < kFimGroup; q++)
        if (q < n_in) v[q] = fim_at(cur, f, ids, offs, out_offs, lo, hi, e0 + q);
}

}  // namespace tgx
