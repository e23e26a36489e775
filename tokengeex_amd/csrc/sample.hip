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
//                       double array's 16-byte records; encode_kernel's back-trace into tmp / counts (then scan + compact).
//   sample_rows_kernel  tokens <= 32 bytes: two samples per wave on 32-lane rows (encode2_kernel's structure), linear
//                       domain with a power-of-two rescale per block of 32 positions; plain 1-byte back-pointers for the
//                       unchanged trace32_kernel.  Sets *range_flag when a value leaves the range it can hold exactly
//                       (the launcher then redoes the call on sample_kernel).
//
// The trie walk, the rows scaffold, the back-trace and the grids are lattice_walk.h's; here are the two semirings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "lattice_walk.h"
#include "sample.h"

namespace tgx {

// same function as tgx_sample_u01 (lattice_pass.cpp): tgx_dropout_u01's rounds over its own start value, and a result in
// (0, 1).  In two parts, sample_u01(sample_u01_at(seed, sample, pos), len): a walk computes the part that all lengths
// from its position share once, whether or not the compiler would have moved it out of the unrolled levels.
__device__ __forceinline__ uint64_t sample_u01_at(uint64_t seed, uint64_t sample, uint64_t pos) {
    return seed ^ 0xD6E8FEB86659FD93ULL ^ (sample * 0x9E3779B97F4A7C15ULL) ^ (pos * 0xC2B2AE3D27D4EB4FULL);
}
__device__ __forceinline__ double sample_u01(uint64_t at, uint32_t len) {
    uint64_t x = at ^ ((uint64_t)len * 0x165667B19E3779F9ULL);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    const double u = ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;  // (2^53 - 1 + 0.5 rounds to 2^53)
}

// ---- generic kernel --------------------------------------------------------------------------------------------
// LDS entries per match: sv = alpha·score, gv = alpha·score − log(−log u), hl = slot << 6 | (len - 1)
constexpr uint32_t kSampleEntryBytes = 8u + 8u + 4u;

__device__ __forceinline__ void sample_block(const EncodeParams& P, const SampleParams& Q, const uint8_t* __restrict__ text, uint32_t n,
                                             uint32_t s, uint32_t p0, uint32_t lane, uint32_t LM, double* sv, double* gv, uint32_t* hl,
                                             uint8_t* txt, uint32_t* __restrict__ bp, double& acc, double& key, uint32_t& bpv,
                                             double& logz_n, uint32_t& reach_n) {
    const uint64_t m = walk_block64(reinterpret_cast<const uint4*>(P.trie), P.root_base, text, n, p0, lane, LM, txt,
                                    [&, at = sample_u01_at(P.seed, s, p0 + lane)](uint32_t d, uint32_t t, const uint4& rec) {
                                        const double a = Q.alpha * rec_score(rec);
                                        const double e = -log(sample_u01(at, d + 1));  // > 0
                                        sv[kFront + lane * LM + d] = a;
                                        gv[kFront + lane * LM + d] = a - log(e);
                                        hl[kFront + lane * LM + d] = (t << 6) | d;
                                    });

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

__global__ __launch_bounds__(256) void sample_kernel(EncodeParams P, SampleParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t LM = P.lm;
    const uint32_t entries = wave_lds_entries(LM);
    unsigned char* wbase = smem + (size_t)wave * lattice_wave_lds_bytes(LM, kSampleEntryBytes);
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
        trace_sample(P, s, beg, n, lane, bp, reach_n);  // (P.flags is encode's: not read here)
    }
}

// ---- rows kernel -----------------------------------------------------------------------------------------------
// Linear domain (lattice_walk.h): the row is renormalised by its largest accumulator.  Match (position, len) holds
// w = exp(alpha·s) (from `wslot`, once per trie slot and call) and kv = w / (−log u); the candidate of step U for lane l
// is best·w, its key best·kv — the order of best·w / E is the order of A[q] + alpha·s − log E, so the keys pick the same
// edge as the log-domain race.  The launcher only picks this kernel when every w lies in [2^-300, 2^300]; a reachable
// position whose value falls outside [2^-600, 2^600] of its row's scale sets *range_flag (no candidate can then underflow
// to zero or overflow, and a key is never further than a factor 2^11 below its accumulator, so the rescale loses none).
constexpr uint64_t kSampleHiHalf = 0xFFFFFFFF00000000ULL;  // lanes of row 1

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

// 32 static steps, one position per row and step; ofs: row (r*32 + U), column (l - 1) & 31
__device__ __forceinline__ void sample_rows_relax(const double* wl, const double* kl, uint32_t ofs, double& acc, double& key, uint32_t& bpv,
                                                  uint32_t& fin, double& fina) {
    double w[16], kv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        w[u] = wl[ofs + u * 32];
        kv[u] = kl[ofs + u * 32];
    }
#define TGX_SAMPLE_STEP(U, K) sample_rows_step<U>(w[K], kv[K], acc, key, bpv, fin, fina)
    TGX_SAMPLE_STEP(0, 0); TGX_SAMPLE_STEP(1, 1); TGX_SAMPLE_STEP(2, 2); TGX_SAMPLE_STEP(3, 3);
    TGX_SAMPLE_STEP(4, 4); TGX_SAMPLE_STEP(5, 5); TGX_SAMPLE_STEP(6, 6); TGX_SAMPLE_STEP(7, 7);
    TGX_SAMPLE_STEP(8, 8); TGX_SAMPLE_STEP(9, 9); TGX_SAMPLE_STEP(10, 10); TGX_SAMPLE_STEP(11, 11);
    TGX_SAMPLE_STEP(12, 12); TGX_SAMPLE_STEP(13, 13); TGX_SAMPLE_STEP(14, 14); TGX_SAMPLE_STEP(15, 15);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        w[u] = wl[ofs + (u + 16) * 32];
        kv[u] = kl[ofs + (u + 16) * 32];
    }
    TGX_SAMPLE_STEP(16, 0); TGX_SAMPLE_STEP(17, 1); TGX_SAMPLE_STEP(18, 2); TGX_SAMPLE_STEP(19, 3);
    TGX_SAMPLE_STEP(20, 4); TGX_SAMPLE_STEP(21, 5); TGX_SAMPLE_STEP(22, 6); TGX_SAMPLE_STEP(23, 7);
    TGX_SAMPLE_STEP(24, 8); TGX_SAMPLE_STEP(25, 9); TGX_SAMPLE_STEP(26, 10); TGX_SAMPLE_STEP(27, 11);
    TGX_SAMPLE_STEP(28, 12); TGX_SAMPLE_STEP(29, 13); TGX_SAMPLE_STEP(30, 14); TGX_SAMPLE_STEP(31, 15);
#undef TGX_SAMPLE_STEP
}

__global__ __launch_bounds__(320) void sample_rows_kernel(EncodeParams P, SampleParams Q) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t l = lane & 31u, r = lane >> 5;
    const uint32_t wave = threadIdx.x >> 6;
    double* wl = reinterpret_cast<double*>(smem + (size_t)wave * kRows32WaveBytes);  // w, then kv
    double* kl = wl + 64u * 32u;

    Rows32 R;
    double acc = 0.0, key = 0.0;
    uint32_t bpv = 0;

    for (;;) {
        rows32_next(P, R, r, [&] {
            acc = (l == 0u) ? 1.0 : 0.0;  // A[0] = 0
            key = 0.0;
            bpv = 0;
        });
        if (__builtin_amdgcn_ballot_w64(R.live) == 0) break;

        const uint32_t pg = R.p0 + l;
        match_rows32(P, R, lane, pg, wl, [&, at = sample_u01_at(P.seed, R.s, pg)](int d, uint32_t t, const uint4&) {
            const double w = Q.wslot[t];
            const double e = -log(sample_u01(at, (uint32_t)d + 1u));
            const uint32_t col = rows32_col(lane, (uint32_t)d);
            wl[col] = w;
            kl[col] = w / e;
        });
        R.scale += renorm_row32(acc, key);

        uint32_t fin = 0;
        double fina = 0.0;
        sample_rows_relax(wl, kl, r * 1024u + ((l - 1u) & 31u), acc, key, bpv, fin, fina);
        __builtin_amdgcn_wave_barrier();
        const bool reached = fina > 0.0;
        if (R.live && pg <= R.n && reached && (fina < 0x1p-600 || fina > 0x1p600)) atomicOr(Q.range_flag, 1ull);

        // ---- back-pointer of this lane's position (plain bytes: index = end position - 1; len - 1, 0xFF = unreachable)
        if (R.live && pg >= 1u && pg <= R.n) {
            const uint8_t b = reached ? (uint8_t)((l - fin - 1u) & 31u) : (uint8_t)0xFF;
            __builtin_nontemporal_store(b, P.bp8 + bp8_base(R.beg, R.s) + (pg - 1u));
        }
        rows32_advance(R, l, [&] {  // this lane holds position n: the sample is done
            P.status[R.s] = (R.n == 0u || reached) ? 1u : 0u;
            Q.logz[R.s] = reached ? rows32_log(fina, R.scale) : -__builtin_huge_val();
        });
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
    const LatticeGrid g = generic_lattice_grid(p.n_samples, lattice_wave_lds_bytes(p.lm, kSampleEntryBytes), num_cus);
    return launch_lattice(sample_kernel, g, stream, p, q);
}

hipError_t launch_sample_wslot(const void* trie, uint32_t n_slots, double alpha, double* out, hipStream_t stream) {
    const uint32_t blocks = (n_slots + 255u) / 256u < 2048u ? ((n_slots + 255u) / 256u ? (n_slots + 255u) / 256u : 1u) : 2048u;
    hipLaunchKernelGGL(sample_wslot_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4*>(trie), n_slots, alpha, out);
    return hipGetLastError();
}

hipError_t launch_sample_rows(const EncodeParams& p, const SampleParams& q, uint32_t num_cus, hipStream_t stream) {
    return launch_lattice(sample_rows_kernel, rows_lattice_grid(p.n_samples, num_cus), stream, p, q);
}

}  // namespace tgx
