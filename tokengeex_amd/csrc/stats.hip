// Per-sample lattice statistics: log Z, the expected score and the expected token count under
// P(x | text) ∝ exp(alpha · Σ score(t)) — sampling's forward sweep (sample.hip) with the expectation semiring in place of
// the exponential race.  No key, no back-pointer, no trace, no compaction: three numbers per sample.
//
// Besides the forward value a[p] = Σ a[q]·w over the matches (q, len, w = exp(alpha·s)) ending at p, the sweep carries
//   r[p] = Σ (r[q]·w + a[q]·w·s)      (Σ over the paths to p of weight · raw score)
//   c[p] = Σ (c[q]·w + a[q]·w)        (Σ over the paths to p of weight · token count)
// so that E[score] = r[n] / a[n] and E[tokens] = c[n] / a[n].
//
//   stats_kernel       generic: one wave per sample, any token length <= 64, log domain (any finite alpha·s).  It
//                      carries A[p] = log a[p] with sample_kernel's log_add sequence (the same logz, bit for bit) and
//                      the normalised expectations m[p] = r[p]/a[p], t[p] = c[p]/a[p]: with π = exp(A[q] + alpha·s − A[p])
//                      they are the convex combinations m[p] = Σ π·(m[q] + s), t[p] = Σ π·(t[q] + 1), updated with every
//                      log_add the online-softmax way (x joins the sum A: m += exp(x − A')·(m_x − m)).
//   stats_rows_kernel  tokens <= 32 bytes: two samples per wave on 32-lane rows, linear domain, sample_rows_kernel's
//                      structure, rescale and range rule; LDS per match holds w and w·s.  The forward value goes
//                      through sample_rows_kernel's operations in its order: the same logz, bit for bit.
//
// The trie walk, the rows scaffold and the grids are lattice_walk.h's; here are the two semirings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "lattice_walk.h"
#include "stats.h"

namespace tgx {

// ---- generic kernel --------------------------------------------------------------------------------------------
// LDS entry per match: rs = the raw score
constexpr uint32_t kStatsEntryBytes = 8u;

__device__ __forceinline__ void stats_block(const EncodeParams& P, const StatsParams& Q, const uint8_t* __restrict__ text, uint32_t n,
                                            uint32_t p0, uint32_t lane, uint32_t LM, double* rs, uint8_t* txt, double& acc, double& macc,
                                            double& tacc, double& z_n, double& m_n, double& t_n) {
    const uint64_t m = walk_block64(reinterpret_cast<const uint4*>(P.trie), P.root_base, text, n, p0, lane, LM, txt,
                                    [&](uint32_t d, uint32_t, const uint4& rec) { rs[kFront + lane * LM + d] = rec_score(rec); });

    // relax positions p0 .. p0 + 63 in order; -inf = "no value yet" in acc (macc and tacc are then 0)
    const double ninf = -__builtin_huge_val();
    const uint32_t left = n - p0;
    const uint32_t steps = left < 64u ? left : 64u;
    for (uint32_t i = 0; i < steps; ++i) {
        const double best = readlane_f64(acc, i);
        const double bm = readlane_f64(macc, i), bt = readlane_f64(tacc, i);
        const uint64_t mi = readlane_u64(m, i);
        if (lane == i) {  // lane i now accumulates position p0 + i + 64
            acc = ninf;
            macc = 0.0;
            tacc = 0.0;
        }
        if (best == ninf || mi == 0) continue;  // wave-uniform
        const uint64_t active = rotl64(mi, i + 1);  // length L -> lane (i + L) % 64
        if ((active >> lane) & 1ULL) {
            const double s = rs[kFront + i * LM + ((lane - i - 1u) & 63u)];
            const double x = best + Q.alpha * s;
            const double nw = log_add(acc, x);
            const double pi = exp(x - nw);  // the new term's share of the sum; 1 when it is the first
            macc = macc + pi * ((bm + s) - macc);
            tacc = tacc + pi * ((bt + 1.0) - tacc);
            acc = nw;
        }
    }
    if (left < 64u) {  // position n sits in this block
        z_n = readlane_f64(acc, left);
        m_n = readlane_f64(macc, left);
        t_n = readlane_f64(tacc, left);
    }
}

__global__ __launch_bounds__(256) void stats_kernel(EncodeParams P, StatsParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t LM = P.lm;
    unsigned char* wbase = smem + (size_t)wave * lattice_wave_lds_bytes(LM, kStatsEntryBytes);
    double* rs = reinterpret_cast<double*>(wbase);
    uint8_t* txt = wbase + (size_t)wave_lds_entries(LM) * 8u;

    for (;;) {
        const uint64_t k = wave_fetch_add(P.queue, 1u);  // the next sample of the longest-first order
        if (k >= P.n_samples) break;
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.order[k]);
        const uint64_t beg = first_u64(P.offs[s]);
        const uint32_t n = (uint32_t)(first_u64(P.offs[s + 1]) - beg);

        double acc = lane == 0 ? 0.0 : -__builtin_huge_val();  // A[0] = 0
        double macc = 0.0, tacc = 0.0;
        double z_n = 0.0, m_n = 0.0, t_n = 0.0;
        for (uint32_t p0 = 0; p0 <= n; p0 += 64u) stats_block(P, Q, P.text + beg, n, p0, lane, LM, rs, txt, acc, macc, tacc, z_n, m_n, t_n);
        if (lane == 0) {
            const bool reached = z_n != -__builtin_huge_val();
            Q.logz[s] = z_n;
            Q.escore[s] = reached ? m_n : __builtin_nan("");
            Q.etokens[s] = reached ? t_n : __builtin_nan("");
        }
    }
}

// ---- rows kernel -----------------------------------------------------------------------------------------------
// Linear domain (lattice_walk.h): the row is renormalised by the exponent of its largest `a`, applied to a, r and c with
// the same exact ldexp.  Match (position, len) holds w = exp(alpha·s) (from `wslot`) and ws = w · s (s from the trie
// record).  Step U hands the row the final (a, r, c) of position p0 + U and every lane adds the candidate of its own
// length:
//   a += a_U·w,   r += r_U·w + a_U·ws,   c += c_U·w + a_U·w.
// The launcher only picks this kernel when every w lies in [2^-300, 2^300]; a reachable position whose `a` falls
// outside [2^-600, 2^600] of its row's scale, or an r or c that is not finite in the block of its sample's end, sets
// *range_flag.

// Lane U of each 32-lane row to all lanes of its row, without the scalar round trip of sample_rows_kernel's broadcast
// (per f64: four v_readlane, four moves of the scalars back into vector registers, two selects by half).  A 32-lane row
// is two DPP rows of 16: the 64-bit DPP move with row_newbcast gives every DPP row its own lane U & 15, and gfx950's
// v_permlane16_swap, which exchanges the odd DPP rows of its first operand with the even DPP rows of its second, then
// copies the DPP row that holds lane U over its neighbour — one DPP move, one copy per word (the instruction overwrites
// both operands) and one swap per word.
typedef uint32_t stats_u32x2 __attribute__((ext_vector_type(2)));
template <int U>
__device__ __forceinline__ double stats_row_bcast(double v) {
    const uint64_t x = (uint64_t)__builtin_amdgcn_mov_dpp(__double_as_longlong(v), 0x150 + (U & 15), 0xF, 0xF, false);  // row_newbcast
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    uint32_t lo2 = lo, hi2 = hi;
    asm volatile("" : "+v"(lo2), "+v"(hi2));  // a register of its own: the swap writes both of its operands
    if constexpr (U < 16) {  // lane U sits in the even DPP row: the first operand's odd rows take the second's even rows
        const stats_u32x2 a = __builtin_amdgcn_permlane16_swap(lo, lo2, false, false);
        const stats_u32x2 b = __builtin_amdgcn_permlane16_swap(hi, hi2, false, false);
        return __hiloint2double((int)b.x, (int)a.x);
    } else {  // lane U sits in the odd DPP row: the second operand's even rows take the first's odd rows
        const stats_u32x2 a = __builtin_amdgcn_permlane16_swap(lo2, lo, false, false);
        const stats_u32x2 b = __builtin_amdgcn_permlane16_swap(hi2, hi, false, false);
        return __hiloint2double((int)b.y, (int)a.y);
    }
}

// LAST: the block holds the end of one of the wave's samples, so r and c of the finalised positions are kept too (the
// sample's results, and the finiteness of r and c: a non-finite r or c reaches every later position of its sample,
// through r_U · 0 if nothing else, so the end's block is where it is looked for).
// The finalised lane restarts with the candidate alone: acc · keep + cand with keep = 0 in lane U and 1 elsewhere is one
// fma per accumulator — round(acc · 1 + cand) is the plain sum, 0 · acc + cand the candidate — in place of an add and a
// two-word select each.
template <int U, bool LAST>
__device__ __forceinline__ void stats_rows_step(double w, double ws, double& a, double& r, double& c, double& fa, double& fr, double& fc) {
    constexpr uint64_t MU = (1ULL << U) | (1ULL << (32 + U));  // lanes with l == U
    fa = sel_f64(MU, a, fa);                                   // position p0 + U is final now
    if constexpr (LAST) {
        fr = sel_f64(MU, r, fr);
        fc = sel_f64(MU, c, fc);
    }
    const double ba = stats_row_bcast<U>(a), br = stats_row_bcast<U>(r), bc = stats_row_bcast<U>(c);
    const double cand = ba * w;  // w = 0: no token of this length from p0 + U
    const double rc = __builtin_fma(br, w, ba * ws);
    const double cc = __builtin_fma(bc, w, cand);
    const double keep = __hiloint2double((int)sel_u32(MU, 0u, 0x3FF00000u), 0);  // lane U restarts with position p0 + U + 32
    a = __builtin_fma(a, keep, cand);
    r = __builtin_fma(r, keep, rc);
    c = __builtin_fma(c, keep, cc);
}

// 32 static steps, one position per row and step; ofs: row (r*32 + U), column (l - 1) & 31
template <bool LAST>
__device__ __forceinline__ void stats_rows_relax(const double* wl, const double* sl, uint32_t ofs, double& acc, double& racc, double& cacc,
                                                 double& fa, double& fr, double& fc) {
    double w[16], ws[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        w[u] = wl[ofs + u * 32];
        ws[u] = sl[ofs + u * 32];
    }
#define TGX_STATS_STEP(U, K) stats_rows_step<U, LAST>(w[K], ws[K], acc, racc, cacc, fa, fr, fc)
    TGX_STATS_STEP(0, 0); TGX_STATS_STEP(1, 1); TGX_STATS_STEP(2, 2); TGX_STATS_STEP(3, 3);
    TGX_STATS_STEP(4, 4); TGX_STATS_STEP(5, 5); TGX_STATS_STEP(6, 6); TGX_STATS_STEP(7, 7);
    TGX_STATS_STEP(8, 8); TGX_STATS_STEP(9, 9); TGX_STATS_STEP(10, 10); TGX_STATS_STEP(11, 11);
    TGX_STATS_STEP(12, 12); TGX_STATS_STEP(13, 13); TGX_STATS_STEP(14, 14); TGX_STATS_STEP(15, 15);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        w[u] = wl[ofs + (u + 16) * 32];
        ws[u] = sl[ofs + (u + 16) * 32];
    }
    TGX_STATS_STEP(16, 0); TGX_STATS_STEP(17, 1); TGX_STATS_STEP(18, 2); TGX_STATS_STEP(19, 3);
    TGX_STATS_STEP(20, 4); TGX_STATS_STEP(21, 5); TGX_STATS_STEP(22, 6); TGX_STATS_STEP(23, 7);
    TGX_STATS_STEP(24, 8); TGX_STATS_STEP(25, 9); TGX_STATS_STEP(26, 10); TGX_STATS_STEP(27, 11);
    TGX_STATS_STEP(28, 12); TGX_STATS_STEP(29, 13); TGX_STATS_STEP(30, 14); TGX_STATS_STEP(31, 15);
#undef TGX_STATS_STEP
}

__global__ __launch_bounds__(320) void stats_rows_kernel(EncodeParams P, StatsParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane & 31u, r = lane >> 5;
    const uint32_t wave = threadIdx.x >> 6;
    double* wl = reinterpret_cast<double*>(smem + (size_t)wave * kRows32WaveBytes);  // w, then ws
    double* sl = wl + 64u * 32u;

    Rows32 R;
    double acc = 0.0, racc = 0.0, cacc = 0.0;

    for (;;) {
        rows32_next(P, R, r, [&] {
            acc = (l == 0u) ? 1.0 : 0.0;  // a[0] = 1, r[0] = c[0] = 0
            racc = 0.0;
            cacc = 0.0;
        });
        if (__builtin_amdgcn_ballot_w64(R.live) == 0) break;

        const uint32_t pg = R.p0 + l;
        match_rows32(P, R, lane, pg, wl, [&](int d, uint32_t t, const uint4& rec) {
            const double w = Q.wslot[t];
            const uint32_t col = rows32_col(lane, (uint32_t)d);
            wl[col] = w;
            sl[col] = w * rec_score(rec);
        });
        R.scale += renorm_row32(acc, racc, cacc);

        // ---- relax (the wave takes the LAST build when the end of either row's sample lies in this block)
        double fa = 0.0, fr = 0.0, fc = 0.0;
        const bool last = R.live && R.n - R.p0 < 32u;
        const bool any_last = __builtin_amdgcn_ballot_w64(last) != 0;  // wave-uniform
        {
            const uint32_t ofs = r * 1024u + ((l - 1u) & 31u);
            if (any_last) stats_rows_relax<true>(wl, sl, ofs, acc, racc, cacc, fa, fr, fc);
            else stats_rows_relax<false>(wl, sl, ofs, acc, racc, cacc, fa, fr, fc);
        }
        __builtin_amdgcn_wave_barrier();
        const bool reached = fa > 0.0;
        const bool finite_rc = __builtin_fabs(fr) < __builtin_huge_val() && __builtin_fabs(fc) < __builtin_huge_val();  // (false for NaN)
        if (R.live && pg <= R.n && reached && (fa < 0x1p-600 || fa > 0x1p600 || (last && !finite_rc))) atomicOr(Q.range_flag, 1ull);

        rows32_advance(R, l, [&] {  // this lane holds position n: the sample is done
            Q.logz[R.s] = reached ? rows32_log(fa, R.scale) : -__builtin_huge_val();
            Q.escore[R.s] = reached ? fr / fa : __builtin_nan("");
            Q.etokens[R.s] = reached ? fc / fa : __builtin_nan("");
        });
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------
hipError_t launch_stats(const EncodeParams& p, const StatsParams& q, uint32_t num_cus, hipStream_t stream) {
    const LatticeGrid g = generic_lattice_grid(p.n_samples, lattice_wave_lds_bytes(p.lm, kStatsEntryBytes), num_cus);
    return launch_lattice(stats_kernel, g, stream, p, q);
}

hipError_t launch_stats_rows(const EncodeParams& p, const StatsParams& q, uint32_t num_cus, hipStream_t stream) {
    return launch_lattice(stats_rows_kernel, rows_lattice_grid(p.n_samples, num_cus), stream, p, q);
}

}  // namespace tgx
