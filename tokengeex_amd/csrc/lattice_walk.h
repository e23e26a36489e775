// What the lattice passes share (sample.hip, stats.hip, nbest.hip): each is encode's forward sweep with another
// semiring, so the trie walk that fills the lattice, the scaffold of the two-rows-per-wave kernels, the grids and the
// wave-per-sample back-trace exist once, here.  Everything is stateless and inlined; a pass hands its own part — what
// it keeps per match — to the walk as a callable, on_match(d, t, rec): the token of length d + 1 that starts at the
// lane's position is the terminal slot t with the trie record rec (score in rec.z, rec.w).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"

namespace tgx {

// log(exp(a) + exp(b)) for a, b finite or -inf
__device__ __forceinline__ double log_add(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo == -__builtin_huge_val()) return hi;
    return hi + log1p(exp(lo - hi));
}

__device__ __forceinline__ double rec_score(const uint4& rec) { return __hiloint2double((int)rec.w, (int)rec.z); }

// ---- generic kernels: one wave per sample, blocks of 64 positions, any token length <= 64 --------------------------
// LDS per wave: arrays of wave_lds_entries(lm) entries, `entry_bytes` in all (encode_kernel's row stride and padding:
// entry kFront + u * lm + len - 1 for the start position u of the block), then 128 bytes of staged text
__host__ __device__ inline uint32_t lattice_wave_lds_bytes(uint32_t lm, uint32_t entry_bytes) {
    return (wave_lds_entries(lm) * entry_bytes + 128u + 15u) & ~15u;
}

// The match phase of block p0: stages the block's text and its look-ahead in `txt`, then every lane walks the trie from
// position p0 + lane.  Returns the lane's mask of matching lengths (bit d: length d + 1); what on_match wrote to LDS is
// visible to the wave on return.
template <class F>
__device__ __forceinline__ uint64_t walk_block64(const uint4* __restrict__ trie, uint32_t root_base, const uint8_t* __restrict__ text,
                                                 uint32_t n, uint32_t p0, uint32_t lane, uint32_t LM, uint8_t* txt, F&& on_match) {
    const uint32_t p = p0 + lane;
    txt[lane] = (p < n) ? text[p] : (uint8_t)0;
    txt[lane + 64] = (p + 64 < n) ? text[p + 64] : (uint8_t)0;
    __builtin_amdgcn_wave_barrier();

    const uint32_t rem = (p < n) ? (n - p) : 0u;
    const uint32_t maxd = rem < LM ? rem : LM;
    uint32_t cur = 0, base = root_base;
    uint64_t m = 0;
    bool alive = maxd > 0;
    for (uint32_t d = 0; d < LM; ++d) {
        alive = alive && (d < maxd);
        if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
        if (alive) {
            const uint32_t t = base ^ (uint32_t)txt[lane + d];
            const uint4 r = load_rec(trie, t);
            if (r.x == cur) {
                cur = t;
                base = r.y & 0x7FFFFFFFu;
                if (r.y >> 31) {
                    m |= 1ULL << d;
                    on_match(d, t, r);
                }
            } else {
                alive = false;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    return m;
}

// The back-trace of the kernels that write 4-byte back-pointers, slot << 6 | (len - 1) at bp[end position - 1]
// (encode_kernel, sample_kernel): the same wave follows them from n (model.rs:113-126), 64 positions per hop group, and
// writes the ids right-aligned into the sample's slice of tmp.  trace = false skips the walk (encode_kernel's experiment
// switch).
__device__ __forceinline__ void trace_sample(const EncodeParams& P, uint32_t s, uint64_t beg, uint32_t n, uint32_t lane,
                                             const uint32_t* __restrict__ bp, uint32_t reach_n, bool trace = true) {
    __threadfence_block();  // this wave's bp stores are read back below
    uint32_t total = 0;
    uint64_t cursor = beg + n;  // one past this sample's slice of tmp
    // Error::NoPath(n, n), model.rs:119: nothing to trace, the sample is reported below
    int64_t q = reach_n ? (int64_t)n - 1 : (int64_t)-1;  // index into bp of the current end position
    if (!trace) q = -1;
    while (q >= 0) {
        const uint32_t wq = (uint32_t)q & ~63u;
        const uint32_t idx = wq + lane;
        const uint32_t h = (idx < n) ? bp[idx] : 0u;
        uint64_t ends = 0;
        int32_t qq = (int32_t)((uint32_t)q - wq);
        while (qq >= 0) {
            const uint32_t hh = readlane_u32(h, (uint32_t)qq);
            ends |= 1ULL << qq;
            qq -= (int32_t)(hh & 63u) + 1;
        }
        q = (int64_t)wq + qq;
        const uint32_t cnt = (uint32_t)__popcll(ends);
        if ((ends >> lane) & 1ULL) {
            // a handle outside the table can only come from a kernel bug; report it as a
            // failed sample instead of faulting the device
            const uint32_t slot = h >> 6;
            if (slot >= P.n_slots) atomicMin(P.err_sample, (unsigned long long)s | (1ULL << 62));
            const uint32_t id = slot < P.n_slots ? P.tokid[slot] : 0u;
            const uint32_t above = (uint32_t)__popcll((ends >> lane) >> 1);
            P.tmp[cursor - 1 - above] = id;
        }
        cursor -= cnt;
        total += cnt;
    }
    if (lane == 0) {
        P.counts[s] = total;
        if (!reach_n) atomicMin(P.err_sample, (unsigned long long)s);
    }
}

// ---- rows kernels: tokens <= 32 bytes, two samples per wave on 32-lane rows (encode2_kernel's structure) -----------
// Lane (r, l) of the wave owns position p0 + l of row r's sample; the rows advance in lock-step over blocks of 32
// positions.  Linear domain: a row's values are stored as v · 2^scale with one scale per row, renormalised at the start
// of every block by an exact power-of-two ldexp (renorm_row32).
// LDS per wave: two f64 arrays of 64 positions x 32 lengths.  The match (lane, len) lives at column (len - 1 + l) & 31 of
// its lane's row, so that the target lane of relax step U always reads column (l - 1) & 31 of row (r * 32 + U).
constexpr uint32_t kRows32WaveBytes = 2u * 64u * 32u * 8u;  // 32 KiB

struct Rows32 {
    uint32_t s = 0, n = 0, p0 = 0;  // the row's sample, its length, the block's first position
    uint64_t beg = 0;               // the sample's first byte
    int64_t scale = 0;              // the row's values are v · 2^scale
    bool live = false, need_new = true;
};

__device__ __forceinline__ uint32_t rows32_col(uint32_t lane, uint32_t d) { return lane * 32u + ((d + lane) & 31u); }

// Rows that finished their sample claim the next one of the longest-first order; at_start() then runs in the lanes of
// such a row and sets the pass's accumulators to the values of position 0.
template <class F>
__device__ __forceinline__ void rows32_next(const EncodeParams& P, Rows32& R, uint32_t r, F&& at_start) {
    const uint64_t k = claim_rows32(P.queue, R.need_new, r);
    if (R.need_new) {
        R.live = k < P.n_samples;
        if (R.live) {
            R.s = P.order[k];
            R.beg = P.offs[R.s];
            R.n = (uint32_t)(P.offs[R.s + 1] - R.beg);
        }
        R.p0 = 0;
        R.scale = 0;
        at_start();
    }
    R.need_new = false;
}

// The 32 bytes from `at` on, from aligned dwords (the text buffer is padded)
__device__ __forceinline__ void text_window32(const uint8_t* __restrict__ at, uint32_t (&bytes)[8]) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(at);
    const uint32_t sh = (uint32_t)(addr & 3u);
    const uint32_t* __restrict__ wp = reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
    uint32_t w9[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) w9[q] = wp[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) bytes[q] = __builtin_amdgcn_alignbyte(w9[q + 1], w9[q], sh);
}

// Zero = "no token": the wave sweeps its two arrays linearly
__device__ __forceinline__ void zero_rows32(double* wave_lds, uint32_t lane) {
    double2* grp = reinterpret_cast<double2*>(wave_lds);
#pragma unroll
    for (int q = 0; q < 32; ++q) grp[q * 64 + lane] = make_double2(0.0, 0.0);
}

// The lane's walk over its text window, at most maxd <= 32 levels
template <class F>
__device__ __forceinline__ void walk_rows32(const uint4* __restrict__ trie, uint32_t root_base, const uint32_t (&bytes)[8], uint32_t maxd,
                                            F&& on_match) {
    uint32_t cur = 0, base = root_base;
    bool alive = maxd > 0;
#pragma unroll
    for (int d = 0; d < 32; ++d) {
        alive = alive && ((uint32_t)d < maxd);
        if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
        if (alive) {
            const uint32_t c = (bytes[d >> 2] >> ((d & 3) * 8)) & 0xFFu;
            const uint32_t t = base ^ c;
            const uint4 rec = load_rec(trie, t);
            alive = rec.x == cur;
            if (alive) {
                cur = t;
                base = rec.y & 0x7FFFFFFFu;
                if (rec.y >> 31) on_match(d, t, rec);
            }
        }
    }
}

// The match phase of the row's block: text window, zero-fill, walk; lane (r, l) walks from position pg = p0 + l.  What
// on_match wrote to LDS is visible to the wave on return.
template <class F>
__device__ __forceinline__ void match_rows32(const EncodeParams& P, const Rows32& R, uint32_t lane, uint32_t pg, double* wave_lds,
                                             F&& on_match) {
    uint32_t bytes[8];
    text_window32(P.text + (R.live ? R.beg + pg : 0), bytes);
    zero_rows32(wave_lds, lane);
    __builtin_amdgcn_wave_barrier();
    const uint32_t rem = (R.live && pg < R.n) ? (R.n - pg) : 0u;
    walk_rows32(reinterpret_cast<const uint4*>(P.trie), P.root_base, bytes, rem < 32u ? rem : 32u, on_match);
    __builtin_amdgcn_wave_barrier();
}

// Renormalises the row whose positions p0 .. p0 + 31 are in its lanes (partial sums): the largest `acc` of the row goes
// to [0.5, 1), the others follow by the same exact ldexp.  Returns the exponent taken out.
template <class... Others>
__device__ __forceinline__ int renorm_row32(double& acc, Others&... others) {
    int ex = (acc == 0.0) ? -100000 : __builtin_amdgcn_frexp_exp(acc);
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) ex = max(ex, __shfl_xor(ex, o, 32));
    if (ex == -100000) ex = 0;
    acc = __builtin_amdgcn_ldexp(acc, -ex);
    ((others = __builtin_amdgcn_ldexp(others, -ex)), ...);
    return ex;
}

// log of the forward value a · 2^scale of a reached position
__device__ __forceinline__ double rows32_log(double a, int64_t scale) { return log(a) + (double)scale * 0.69314718055994530942; }

// The row's block is done: on to the next one, or, when position n lies in this block, to the next sample — at_end() then
// runs in the lane that holds position n and writes the sample's results.  (A callable, not a returned flag: with the
// stores after the call stats_rows_kernel measured 0.8 % slower, another register allocation.)
template <class F>
__device__ __forceinline__ void rows32_advance(Rows32& R, uint32_t l, F&& at_end) {
    if (R.live) {
        const uint32_t left = R.n - R.p0;
        if (left < 32u) {
            if (left == l) at_end();
            R.need_new = true;
        } else {
            R.p0 += 32u;
        }
    }
}

// ---- grids ---------------------------------------------------------------------------------------------------------
struct LatticeGrid {
    uint32_t blocks, threads, lds_bytes;
};

// Generic kernels: as many waves per block as the LDS holds, four at the most; blocks capped by what the CUs hold
inline LatticeGrid generic_lattice_grid(uint64_t n_samples, uint32_t wave_bytes, uint32_t num_cus) {
    const uint32_t lds = 160u * 1024u;
    uint32_t wpb = lds / wave_bytes;
    wpb = wpb < 1u ? 1u : (wpb > 4u ? 4u : wpb);
    const uint64_t want = (n_samples + wpb - 1) / wpb;
    const uint64_t per_cu = lds / (wpb * wave_bytes) > 0 ? lds / (wpb * wave_bytes) : 1u;
    const uint64_t cap = (uint64_t)num_cus * per_cu;
    return {(uint32_t)(want < 1 ? 1 : (want < cap ? want : cap)), 64u * wpb, wpb * wave_bytes};
}

// Rows kernels: one block of five waves per CU, 5 x 32 KiB of LDS
inline LatticeGrid rows_lattice_grid(uint64_t n_samples, uint32_t num_cus) {
    const uint32_t waves = 5;
    const uint64_t want = (n_samples + 2 * waves - 1) / (2 * waves);
    return {(uint32_t)(want < (uint64_t)num_cus ? (want ? want : 1) : (uint64_t)num_cus), 64u * waves, waves * kRows32WaveBytes};
}

template <class... Params>
inline hipError_t launch_lattice(void (*kernel)(Params...), const LatticeGrid& g, hipStream_t stream, const Params&... params) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds_bytes, stream, params...);
    return hipGetLastError();
}

}  // namespace tgx
