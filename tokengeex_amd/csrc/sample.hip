// Subword regularisation (Kudo 2018, SentencePiece's enable_sampling with nbest_size = -1): one segmentation per sample
// drawn from P(x | text) ∝ exp(alpha · Σ score(t)), by forward filtering and backward sampling over the lattice.
//
// The choice of the token that ends at position p has probability exp(A[q] + alpha·s − A[p]) for the match (q, len),
// q + len = p, where A is the forward value of the tempered lattice (A[0] = 0, A[p] = logsumexp of A[q] + alpha·s).  It
// depends on p alone, not on the path that led back to it, so every position draws its back-pointer on its own and the
// sampled path is whatever the usual back-trace follows from n.  The draw is an exponential race (Gumbel-max): match e
// gets u_e = sample_u01(seed, sample, q, len) and key A[q] + alpha·s − log(−log u_e); the largest key wins, exact ties go
// to the longer token (candidates arrive in ascending start order and replace only on a strict '>', as in encode).
// Encode with the semiring (logsumexp, perturbed argmax) in place of (max, argmax): one forward sweep writes the same
// back-pointers encode writes.
//
//   sample_kernel       generic: one wave per sample, any token length <= 64, log domain (any finite alpha), the
//                       double array's 16-byte records; its own back-trace into tmp / counts (then scan + compact).
//   sample_rows_kernel  tokens <= 32 bytes: two samples per wave on 32-lane rows (encode2_kernel's structure), linear
//                       domain with a power-of-two rescale per block of 32 positions; plain 1-byte back-pointers for the
//                       unchanged trace32_kernel.  Sets *range_flag when a value leaves the range it can hold exactly
//                       (the launcher then redoes the call on sample_kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "sample.h"

namespace tgx {

// same function as tgx_sample_u01 (lattice_pass.cpp): tgx_dropout_u01's rounds over its own start value, and a result in (0, 1)
__device__ __forceinline__ double sample_u01(uint64_t seed, uint64_t sample, uint64_t pos, uint32_t len) {
    uint64_t x = seed ^ 0xD6E8FEB86659FD93ULL ^ (sample * 0x9E3779B97F4A7C15ULL) ^ (pos * 0xC2B2AE3D27D4EB4FULL) ^
                 ((uint64_t)len * 0x165667B19E3779F9ULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    const double u = ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;  // (2^53 - 1 + 0.5 rounds to 2^53)
}

// log(exp(a) + exp(b)) for a, b finite or -inf
__device__ __forceinline__ double log_add(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo == -__builtin_huge_val()) return hi;
    return hi + log1p(exp(lo - hi));
}

// ---- generic kernel --------------------------------------------------------------------------------------------
// LDS per wave: sv[row u = start position in the 64-block][len - 1] = alpha·score, gv[...] = alpha·score − log(−log u),
// hl[...] = slot << 6 | (len - 1), then 128 bytes of staged text.  Same row stride and padding as encode_kernel.
__host__ __device__ inline uint32_t sample_wave_lds_bytes(uint32_t lm) {
    return (wave_lds_entries(lm) * 20u + 128u + 15u) & ~15u;
}

__device__ __forceinline__ void sample_block(const EncodeParams& P, const SampleParams& Q, const uint8_t* __restrict__ text, uint32_t n,
                                             uint32_t s, uint32_t p0, uint32_t lane, uint32_t LM, double* sv, double* gv, uint32_t* hl,
                                             uint8_t* txt, uint32_t* __restrict__ bp, double& acc, double& key, uint32_t& bpv,
                                             double& logz_n, uint32_t& reach_n) {
    const uint4* __restrict__ trie = reinterpret_cast<const uint4*>(P.trie);
    const uint32_t p = p0 + lane;
    txt[lane] = (p < n) ? text[p] : (uint8_t)0;
    txt[lane + 64] = (p + 64 < n) ? text[p + 64] : (uint8_t)0;
    __builtin_amdgcn_wave_barrier();

    // match: every lane walks the trie from its own position
    const uint32_t rem = (p < n) ? (n - p) : 0u;
    const uint32_t maxd = rem < LM ? rem : LM;
    uint32_t cur = 0, base = P.root_base;
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
                    const double a = Q.alpha * __hiloint2double((int)r.w, (int)r.z);
                    const double e = -log(sample_u01(P.seed, s, p, d + 1));  // > 0
                    m |= 1ULL << d;
                    sv[kFront + lane * LM + d] = a;
                    gv[kFront + lane * LM + d] = a - log(e);
                    hl[kFront + lane * LM + d] = (t << 6) | d;
                }
            } else {
                alive = false;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();

    // relax positions p0 .. p0 + 63 in order; -inf = "no value yet" in acc and key
    const double ninf = -__builtin_huge_val();
    const uint32_t left = n - p0;
    const uint32_t steps = left < 64u ? left : 64u;
    uint32_t fin = 0;
    for (uint32_t i = 0; i < steps; ++i) {
        fin = (lane == i) ? bpv : fin;  // back-pointer of position p0 + i is final now
        const double best = readlane_f64(acc, i);
        const uint64_t mi = readlane_u64(m, i);
        if (lane == i) {  // lane i now accumulates position p0 + i + 64
            acc = ninf;
            key = ninf;
        }
        if (best == ninf || mi == 0) continue;  // wave-uniform
        const uint64_t active = rotl64(mi, i + 1);  // length L -> lane (i + L) % 64
        if ((active >> lane) & 1ULL) {
            const uint32_t idx = kFront + i * LM + ((lane - i - 1u) & 63u);
            const double k = best + gv[idx];
            acc = log_add(acc, best + sv[idx]);
            if (k > key) {  // strict: ties keep the longer token, which came first
                key = k;
                bpv = hl[idx];
            }
        }
    }
    if (left < 64u) {  // position n sits in this block
        fin = (lane == left) ? bpv : fin;
        logz_n = readlane_f64(acc, left);
        reach_n = logz_n != ninf ? 1u : 0u;
    }
    const uint32_t e = p0 + lane;
    if (e >= 1 && e <= n) bp[e - 1] = fin;
}

// encode_kernel's back-trace (kernels.hip: trace_sample): ids right-aligned in the sample's slice of tmp
__device__ __forceinline__ void sample_trace(const EncodeParams& P, uint32_t s, uint64_t beg, uint32_t n, uint32_t lane,
                                             const uint32_t* __restrict__ bp, uint32_t reach_n) {
    __threadfence_block();
    uint32_t total = 0;
    uint64_t cursor = beg + n;
    int64_t q = reach_n ? (int64_t)n - 1 : (int64_t)-1;
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

__global__ __launch_bounds__(256) void sample_kernel(EncodeParams P, SampleParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t LM = P.lm;
    const uint32_t entries = wave_lds_entries(LM);
    unsigned char* wbase = smem + (size_t)wave * sample_wave_lds_bytes(LM);
    double* sv = reinterpret_cast<double*>(wbase);
    double* gv = reinterpret_cast<double*>(wbase + (size_t)entries * 8u);
    uint32_t* hl = reinterpret_cast<uint32_t*>(wbase + (size_t)entries * 16u);
    uint8_t* txt = wbase + (size_t)entries * 20u;

    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t n_waves = gridDim.x * wpb;
    const uint32_t wave_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + wave));
    for (uint64_t k = wave_id; k < P.n_samples; k += n_waves) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.order[k]);
        const uint64_t beg = first_u64(P.offs[s]);
        const uint32_t n = (uint32_t)(first_u64(P.offs[s + 1]) - beg);
        uint32_t* __restrict__ bp = P.bp + beg;

        double acc = lane == 0 ? 0.0 : -__builtin_huge_val();  // A[0] = 0
        double key = -__builtin_huge_val();
        uint32_t bpv = 0;
        double logz_n = 0.0;
        uint32_t reach_n = (n == 0) ? 1u : 0u;
        for (uint32_t p0 = 0; p0 <= n; p0 += 64u)
            sample_block(P, Q, P.text + beg, n, s, p0, lane, LM, sv, gv, hl, txt, bp, acc, key, bpv, logz_n, reach_n);
        if (lane == 0) Q.logz[s] = logz_n;
        sample_trace(P, s, beg, n, lane, bp, reach_n);
    }
}

// ---- rows kernel -----------------------------------------------------------------------------------------------
// Linear domain: a row's values are stored as a · 2^scale with one scale per row, renormalised (max accumulator in
// [0.5, 1)) at the start of every block of 32 positions by an exact power-of-two ldexp.  Match (position, len) holds
// w = exp(alpha·s) (from `wslot`, once per trie slot and call) and kv = w / (−log u); the candidate of step U for lane l
// is best·w, its key best·kv — the order of best·w / E is the order of A[q] + alpha·s − log E, so the keys pick the same
// edge as the log-domain race.  The launcher only picks this kernel when every w lies in [2^-300, 2^300]; a reachable
// position whose value falls outside [2^-600, 2^600] of its row's scale sets *range_flag (no candidate can then underflow
// to zero or overflow, and a key is never further than a factor 2^11 below its accumulator, so the rescale loses none).
constexpr uint32_t kSampleRowsBytes = 2u * 64u * 32u * 8u;  // 32 KiB per wave: w and kv, 64 positions x 32 lengths
constexpr uint64_t kSampleHiHalf = 0xFFFFFFFF00000000ULL;   // lanes of row 1

template <int U>
__device__ __forceinline__ void sample_rows_step(double w, double kv, double& acc, double& key, uint32_t& bpv, uint32_t& fin,
                                                 double& fina) {
    constexpr uint64_t MU = (1ULL << U) | (1ULL << (32 + U));  // lanes with l == U
    fin = sel_u32(MU, bpv, fin);                               // position p0 + U is final now
    fina = sel_f64(MU, acc, fina);
    const double b0 = readlane_f64(acc, (uint32_t)U), b1 = readlane_f64(acc, 32u + (uint32_t)U);
    const double best = sel_f64(kSampleHiHalf, b1, b0);
    const double cand = best * w;  // w = 0: no token of this length from p0 + U
    const double kc = best * kv;
    acc = sel_f64(MU, cand, acc + cand);  // lane U restarts with position p0 + U + 32
    const uint64_t take = __builtin_amdgcn_fcmp(kc, key, 2 /* OGT */) | MU;
    key = sel_f64(take, kc, key);
    bpv = sel_imm_u32<U>(take, bpv);
}

__global__ __launch_bounds__(320) void sample_rows_kernel(EncodeParams P, SampleParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t LM = 32;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane & 31u, r = lane >> 5;
    const uint32_t wave = threadIdx.x >> 6;
    const uint4* __restrict__ trie = reinterpret_cast<const uint4*>(P.trie);
    double* wl = reinterpret_cast<double*>(smem + (size_t)wave * kSampleRowsBytes);
    double* kl = wl + 64u * 32u;

    uint32_t s = 0, n = 0, p0 = 0;
    uint64_t beg = 0;
    int64_t scale = 0;  // the row's values are a · 2^scale
    bool live = false, need_new = true;
    double acc = 0.0, key = 0.0;
    uint32_t bpv = 0;

    for (;;) {
        {
            const uint64_t want = __builtin_amdgcn_ballot_w64(need_new) & 0x0000000100000001ULL;
            uint64_t k = ~0ull;
            if (want != 0) {  // wave-uniform
                const uint64_t b = wave_fetch_add(P.queue, (uint32_t)__builtin_popcountll(want));
                if (need_new) k = b + (uint64_t)__builtin_popcountll(want & ((1ull << (r * 32u)) - 1ull));
            }
            if (need_new) {
                live = k < P.n_samples;
                if (live) {
                    s = P.order[k];
                    beg = P.offs[s];
                    n = (uint32_t)(P.offs[s + 1] - beg);
                }
                p0 = 0;
                scale = 0;
                acc = (l == 0u) ? 1.0 : 0.0;  // A[0] = 0
                key = 0.0;
                bpv = 0;
            }
        }
        need_new = false;
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;

        // ---- match: lane (r, l) walks from position p0 + l
        const uintptr_t addr = reinterpret_cast<uintptr_t>(P.text + (live ? beg + p0 + l : 0));
        const uint32_t sh = (uint32_t)(addr & 3u);
        const uint32_t* __restrict__ wp = reinterpret_cast<const uint32_t*>(addr & ~uintptr_t(3));
        uint32_t w9[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) w9[q] = wp[q];
        uint32_t bytes[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) bytes[q] = __builtin_amdgcn_alignbyte(w9[q + 1], w9[q], sh);
        {
            double2* grp = reinterpret_cast<double2*>(wl);  // w and kv of the wave: 32 KiB, swept linearly
#pragma unroll
            for (int q = 0; q < 32; ++q) grp[q * 64 + lane] = make_double2(0.0, 0.0);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t pg = p0 + l;
        const uint32_t rem = (live && pg < n) ? (n - pg) : 0u;
        const uint32_t maxd = rem < LM ? rem : LM;
        uint32_t cur = 0, base = P.root_base;
        bool alive = maxd > 0;
#pragma unroll
        for (int d = 0; d < (int)LM; ++d) {
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
                    if (rec.y >> 31) {
                        const double w = Q.wslot[t];
                        const double e = -log(sample_u01(P.seed, s, pg, (uint32_t)d + 1u));
                        const uint32_t col = lane * LM + (((uint32_t)d + l) & 31u);  // reader's column is a per-lane constant
                        wl[col] = w;
                        kl[col] = w / e;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();

        // ---- renormalise the row: positions p0 .. p0 + 31 are in its lanes (partial sums)
        {
            int ex = (acc == 0.0) ? -100000 : __builtin_amdgcn_frexp_exp(acc);
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) ex = max(ex, __shfl_xor(ex, o, 32));
            if (ex == -100000) ex = 0;
            acc = __builtin_amdgcn_ldexp(acc, -ex);
            key = __builtin_amdgcn_ldexp(key, -ex);
            scale += ex;
        }

        // ---- relax: 32 static steps, one position per row and step
        uint32_t fin = 0;
        double fina = 0.0;
        {
            const uint32_t ofs = r * 1024u + ((l - 1u) & 31u);  // row (r*32 + U), column (l - 1) & 31
            double w[16], kv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                w[u] = wl[ofs + u * 32];
                kv[u] = kl[ofs + u * 32];
            }
            sample_rows_step<0>(w[0], kv[0], acc, key, bpv, fin, fina);
            sample_rows_step<1>(w[1], kv[1], acc, key, bpv, fin, fina);
            sample_rows_step<2>(w[2], kv[2], acc, key, bpv, fin, fina);
            sample_rows_step<3>(w[3], kv[3], acc, key, bpv, fin, fina);
            sample_rows_step<4>(w[4], kv[4], acc, key, bpv, fin, fina);
            sample_rows_step<5>(w[5], kv[5], acc, key, bpv, fin, fina);
            sample_rows_step<6>(w[6], kv[6], acc, key, bpv, fin, fina);
            sample_rows_step<7>(w[7], kv[7], acc, key, bpv, fin, fina);
            sample_rows_step<8>(w[8], kv[8], acc, key, bpv, fin, fina);
            sample_rows_step<9>(w[9], kv[9], acc, key, bpv, fin, fina);
            sample_rows_step<10>(w[10], kv[10], acc, key, bpv, fin, fina);
            sample_rows_step<11>(w[11], kv[11], acc, key, bpv, fin, fina);
            sample_rows_step<12>(w[12], kv[12], acc, key, bpv, fin, fina);
            sample_rows_step<13>(w[13], kv[13], acc, key, bpv, fin, fina);
            sample_rows_step<14>(w[14], kv[14], acc, key, bpv, fin, fina);
            sample_rows_step<15>(w[15], kv[15], acc, key, bpv, fin, fina);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                w[u] = wl[ofs + (u + 16) * 32];
                kv[u] = kl[ofs + (u + 16) * 32];
            }
            sample_rows_step<16>(w[0], kv[0], acc, key, bpv, fin, fina);
            sample_rows_step<17>(w[1], kv[1], acc, key, bpv, fin, fina);
            sample_rows_step<18>(w[2], kv[2], acc, key, bpv, fin, fina);
            sample_rows_step<19>(w[3], kv[3], acc, key, bpv, fin, fina);
            sample_rows_step<20>(w[4], kv[4], acc, key, bpv, fin, fina);
            sample_rows_step<21>(w[5], kv[5], acc, key, bpv, fin, fina);
            sample_rows_step<22>(w[6], kv[6], acc, key, bpv, fin, fina);
            sample_rows_step<23>(w[7], kv[7], acc, key, bpv, fin, fina);
            sample_rows_step<24>(w[8], kv[8], acc, key, bpv, fin, fina);
            sample_rows_step<25>(w[9], kv[9], acc, key, bpv, fin, fina);
            sample_rows_step<26>(w[10], kv[10], acc, key, bpv, fin, fina);
            sample_rows_step<27>(w[11], kv[11], acc, key, bpv, fin, fina);
            sample_rows_step<28>(w[12], kv[12], acc, key, bpv, fin, fina);
            sample_rows_step<29>(w[13], kv[13], acc, key, bpv, fin, fina);
            sample_rows_step<30>(w[14], kv[14], acc, key, bpv, fin, fina);
            sample_rows_step<31>(w[15], kv[15], acc, key, bpv, fin, fina);
        }
        __builtin_amdgcn_wave_barrier();
        const bool reached = fina > 0.0;
        if (live && pg <= n && reached && (fina < 0x1p-600 || fina > 0x1p600)) atomicOr(Q.range_flag, 1ull);

        // ---- back-pointer of this lane's position (plain bytes: index = end position - 1; len - 1, 0xFF = unreachable)
        if (live && pg >= 1u && pg <= n) {
            const uint8_t b = reached ? (uint8_t)((l - fin - 1u) & 31u) : (uint8_t)0xFF;
            __builtin_nontemporal_store(b, P.bp8 + bp8_base(beg, s) + (pg - 1u));
        }
        if (live) {
            const uint32_t left = n - p0;
            if (left < 32u) {  // position n lies in this block: the sample is done
                if (left == l) {
                    P.status[s] = (n == 0u || reached) ? 1u : 0u;
                    Q.logz[s] = reached ? log(fina) + (double)scale * 0.69314718055994530942 : -__builtin_huge_val();
                }
                need_new = true;
            } else {
                p0 += 32u;
            }
        }
    }
}

// w = exp(alpha · score) of every terminal slot of the double array (0 elsewhere)
__global__ __launch_bounds__(256) void sample_wslot_kernel(const uint4* __restrict__ trie, uint32_t n_slots, double alpha,
                                                           double* __restrict__ out) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_slots; t += gridDim.x * blockDim.x) {
        const uint4 rec = trie[t];
        out[t] = (rec.y >> 31) ? exp(alpha * __hiloint2double((int)rec.w, (int)rec.z)) : 0.0;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------
hipError_t launch_sample(const EncodeParams& p, const SampleParams& q, uint32_t num_cus, hipStream_t stream) {
    const uint32_t wb = sample_wave_lds_bytes(p.lm);
    uint32_t wpb = (160u * 1024u) / wb;
    wpb = wpb < 1u ? 1u : (wpb > 4u ? 4u : wpb);
    const uint64_t want = (p.n_samples + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)num_cus * ((160u * 1024u) / (wpb * wb) > 0 ? (160u * 1024u) / (wpb * wb) : 1u);
    const uint32_t blocks = (uint32_t)(want < 1 ? 1 : (want < cap ? want : cap));
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_kernel, dim3(blocks), dim3(64u * wpb), wpb * wb, stream, p, q);
    return hipGetLastError();
}

hipError_t launch_sample_wslot(const void* trie, uint32_t n_slots, double alpha, double* out, hipStream_t stream) {
    const uint32_t blocks = (n_slots + 255u) / 256u < 2048u ? ((n_slots + 255u) / 256u ? (n_slots + 255u) / 256u : 1u) : 2048u;
    hipLaunchKernelGGL(sample_wslot_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4*>(trie), n_slots, alpha, out);
    return hipGetLastError();
}

// one block of five waves per CU: 5 x 32 KiB of LDS
hipError_t launch_sample_rows(const EncodeParams& p, const SampleParams& q, uint32_t num_cus, hipStream_t stream) {
    const uint32_t waves = 5;
    const uint64_t want = (p.n_samples + 2 * waves - 1) / (2 * waves);
    const uint32_t blocks = (uint32_t)(want < (uint64_t)num_cus ? (want ? want : 1) : (uint64_t)num_cus);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(blocks), dim3(64u * waves), waves * kSampleRowsBytes, stream, p, q);
    return hipGetLastError();
}

}  // namespace tgx
