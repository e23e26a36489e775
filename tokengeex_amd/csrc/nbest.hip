// N-best segmentation (SentencePiece's NBestEncode; Kudo 2018's subword regularisation with nbest_size > 1): the k
// highest-scoring segmentations of every sample, best first.  Encode with the semiring (top-K merge, K back-pointers)
// in place of (max, argmax).
//
// Every position p keeps a list L[p] of at most K entries (score, back-pointer), sorted by the pinned order of
// include/tgx.h: score descending, then q = p - len ascending, then the source rank r ascending.  The back-pointer
// (nbest.h) is built so that this tie order is its integer order, so a compare is (score, u32) and the lists do not
// depend on how they were merged.  L[0] = [(0, -)], L[p] = the top K of (L[q][r] + s, q, r) over the matches (q, len),
// q + len = p.  Because fl(a + s) is monotone in a, the source list plus s is itself sorted, and merging it into the
// receiver's list is one bitonic merge: the better of A[j] and B[K-1-j], then log2 K half-cleaner stages.
//
//   nbest_kernel<K>        one wave per sample, encode_kernel's block structure: blocks of 64 positions, every lane
//                          walks the trie from its own position (matches into LDS), then 64 ordered relax steps.  At
//                          step i the list of position p0 + i (lane i) is final: it goes out to HBM as K back-pointers,
//                          its scores are broadcast with readlane, and every lane i + len that a match from it reaches
//                          merges them (+ s) into its own list.  Lists live in registers, every index compile-time.
//   nbest_trace_kernel<K>  one thread per row: the back-trace from (n, r), ids right-aligned in the row's scratch.
//   nbest_compact_kernel   one wave per row: scratch -> the result's ids (after scan_counts_kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"
#include "kernels.h"
#include "lattice_walk.h"
#include "nbest.h"

namespace tgx {

// (a, ak) comes before (b, bk): score descending, then back-pointer ascending
__device__ __forceinline__ bool nb_before(double a, uint32_t ak, double b, uint32_t bk) {
    return a > b || (a == b && ak < bk);
}

// A (sorted) <- the top K of A and B, B[m] = (S[m] + s, key | m << 22) (sorted: S is a final list)
template <int K>
__device__ __forceinline__ void nb_merge(double (&A)[K], uint32_t (&AK)[K], const double (&S)[K], double s, uint32_t key) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double b = S[K - 1 - j] + s;
        const uint32_t bk = key | ((uint32_t)(K - 1 - j) << 22);
        const bool t = nb_before(b, bk, A[j], AK[j]);
        A[j] = t ? b : A[j];
        AK[j] = t ? bk : AK[j];
    }
#pragma unroll
    for (int h = K / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if ((j & h) == 0) {
                const double x = A[j], y = A[j + h];
                const uint32_t xk = AK[j], yk = AK[j + h];
                const bool t = nb_before(y, yk, x, xk);
                A[j] = t ? y : x;
                AK[j] = t ? yk : xk;
                A[j + h] = t ? x : y;
                AK[j + h] = t ? xk : yk;
            }
        }
    }
}

// LDS per wave: sv[row u = start position in the 64-block][len - 1] = score, hid[...] = id, then 128 bytes of staged
// text: encode_kernel's layout (wave_lds_bytes)
template <int K>
__device__ __forceinline__ void nbest_block(const NbestParams& P, const uint8_t* __restrict__ text, uint32_t n, uint32_t p0, uint32_t lane,
                                            uint32_t LM, double* sv, uint32_t* hid, uint8_t* txt, uint32_t* __restrict__ bp,
                                            double (&A)[K], uint32_t (&AK)[K]) {
    const uint64_t m = walk_block64(reinterpret_cast<const uint4*>(P.trie), P.root_base, text, n, p0, lane, LM, txt,
                                    [&](uint32_t d, uint32_t t, const uint4& rec) {
                                        sv[kFront + lane * LM + d] = rec_score(rec);
                                        hid[kFront + lane * LM + d] = t < P.n_slots ? P.tokid[t] : 0u;
                                    });

    // relax positions p0 .. p0 + 63 in order
    const double ninf = -__builtin_huge_val();
    const uint32_t left = n - p0;
    const uint32_t steps = left < 64u ? left : 64u;
    for (uint32_t i = 0; i < steps; ++i) {
        const uint64_t mi = readlane_u64(m, i);
        double S[K];
#pragma unroll
        for (int j = 0; j < K; ++j) S[j] = readlane_f64(A[j], i);
        if (lane == i) {  // the list of position p0 + i is final: its back-pointers; lane i now gathers p0 + i + 64
            uint32_t* __restrict__ o = bp + (uint64_t)(p0 + i) * K;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                o[j] = AK[j];
                A[j] = ninf;
                AK[j] = ~0u;
            }
        }
        if (S[0] == ninf || mi == 0) continue;  // wave-uniform
        const uint64_t active = rotl64(mi, i + 1);  // length L -> lane (i + L) % 64
        if ((active >> lane) & 1ULL) {
            const uint32_t d = (lane - i - 1u) & 63u;  // len - 1
            const uint32_t idx = kFront + i * LM + d;
            nb_merge<K>(A, AK, S, sv[idx], ((63u - d) << 26) | hid[idx]);
        }
    }
    if (left < 64u && lane == left) {  // position n sits in this block: its list is complete in lane `left`
        uint32_t* __restrict__ o = bp + (uint64_t)n * K;
#pragma unroll
        for (int j = 0; j < K; ++j) o[j] = AK[j];
    }
}

template <int K>
__global__ __launch_bounds__(256) void nbest_kernel(NbestParams P) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t LM = P.lm;
    const uint32_t entries = wave_lds_entries(LM);
    unsigned char* wbase = smem + (size_t)wave * wave_lds_bytes(LM);
    double* sv = reinterpret_cast<double*>(wbase);
    uint32_t* hid = reinterpret_cast<uint32_t*>(wbase + (size_t)entries * 8u);
    uint8_t* txt = wbase + (size_t)entries * 12u;

    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t n_waves = gridDim.x * wpb;
    const uint32_t wave_id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * wpb + wave));
    for (uint64_t k = wave_id; k < P.n_samples; k += n_waves) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.order[k]);
        const uint64_t beg = first_u64(P.offs[s]);
        const uint32_t n = (uint32_t)(first_u64(P.offs[s + 1]) - beg);
        uint32_t* __restrict__ bp = P.bp + (beg - P.byte0 + (s - P.s0)) * K;

        double A[K];
        uint32_t AK[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            A[j] = -__builtin_huge_val();
            AK[j] = ~0u;
        }
        if (lane == 0) {  // L[0] = [(0, -)]
            A[0] = 0.0;
            AK[0] = 0u;
        }
        for (uint32_t p0 = 0; p0 <= n; p0 += 64u) nbest_block<K>(P, P.text + beg, n, p0, lane, LM, sv, hid, txt, bp, A, AK);
        // L[n] is in lane n % 64: the scores of the first k entries and how many are paths
        const uint32_t ln = n & 63u;
        uint32_t found = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if ((uint32_t)j < P.k) {
                const double v = readlane_f64(A[j], ln);
                found += v != -__builtin_huge_val() ? 1u : 0u;
                if (lane == (uint32_t)j) P.scores[(uint64_t)s * P.k + j] = v;
            }
        }
        if (lane == 0) {
            P.n_found[s] = found;
            if (found == 0) atomicMin(P.err_sample, (unsigned long long)s);
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void nbest_trace_kernel(NbestParams P) {
    const uint64_t rows = P.n_samples * P.k;
    for (uint64_t R = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; R < rows; R += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t sl = R / P.k;
        const uint32_t r = (uint32_t)(R - sl * P.k);
        const uint64_t s = P.s0 + sl;
        const uint64_t beg = P.offs[s] - P.byte0;
        const uint32_t n = (uint32_t)(P.offs[s + 1] - P.offs[s]);
        const uint32_t* __restrict__ bp = P.bp + (beg + sl) * K;
        uint32_t* __restrict__ out = P.tmp + (uint64_t)r * P.chunk_bytes + beg;
        uint32_t cnt = 0;
        if (r < P.n_found[s]) {
            uint32_t q = n, rr = r;
            while (q > 0) {
                const uint32_t v = bp[(uint64_t)q * K + rr];
                const uint32_t len = 64u - (v >> 26);
                const uint32_t nr = (v >> 22) & 15u;
                if (len > q || nr >= (uint32_t)K || (v & (kNbestMaxVocab - 1u)) == kNbestMaxVocab - 1u) {
                    atomicMin(P.err_sample, (unsigned long long)s | (1ULL << 62));
                    break;
                }
                out[n - 1u - cnt] = v & (kNbestMaxVocab - 1u);
                cnt++;
                q -= len;
                rr = nr;
            }
        }
        P.counts[R] = cnt;
    }
}

__global__ __launch_bounds__(256) void nbest_compact_kernel(NbestParams P, const uint64_t* __restrict__ out_offs, uint32_t* __restrict__ ids) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t rows = P.n_samples * P.k;
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t R = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); R < rows; R += n_waves) {
        const uint64_t sl = R / P.k;
        const uint32_t r = (uint32_t)(R - sl * P.k);
        const uint64_t s = P.s0 + sl;
        const uint64_t end = P.offs[s + 1] - P.byte0;
        const uint64_t o0 = out_offs[R];
        const uint32_t cnt = (uint32_t)(out_offs[R + 1] - o0);
        const uint32_t* __restrict__ src = P.tmp + (uint64_t)r * P.chunk_bytes + end - cnt;
        for (uint32_t i = lane; i < cnt; i += 64u) ids[o0 + i] = src[i];
    }
}

__global__ __launch_bounds__(256) void offs_add_kernel(uint64_t* offs, uint64_t n, uint64_t add) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) offs[i] += add;
}

// ---- launchers ---------------------------------------------------------------------------------------------------
template <int K>
static hipError_t launch_nbest_k(const NbestParams& p, uint32_t num_cus, hipStream_t stream) {
    return launch_lattice(nbest_kernel<K>, generic_lattice_grid(p.n_samples, wave_lds_bytes(p.lm), num_cus), stream, p);
}

hipError_t launch_nbest(const NbestParams& p, uint32_t K, uint32_t num_cus, hipStream_t stream) {
    switch (K) {
        case 1: return launch_nbest_k<1>(p, num_cus, stream);
        case 2: return launch_nbest_k<2>(p, num_cus, stream);
        case 4: return launch_nbest_k<4>(p, num_cus, stream);
        case 8: return launch_nbest_k<8>(p, num_cus, stream);
        case 16: return launch_nbest_k<16>(p, num_cus, stream);
        default: return hipErrorInvalidValue;
    }
}

static uint32_t grid_for(uint64_t units, uint64_t per_block, uint32_t num_cus) {
    const uint64_t want = (units + per_block - 1) / per_block;
    const uint64_t cap = (uint64_t)num_cus * 8u;
    return (uint32_t)(want < 1 ? 1 : (want < cap ? want : cap));
}

hipError_t launch_nbest_trace(const NbestParams& p, uint32_t K, uint32_t num_cus, hipStream_t stream) {
    const uint32_t blocks = grid_for(p.n_samples * p.k, 256, num_cus);
    switch (K) {
        case 1: hipLaunchKernelGGL(nbest_trace_kernel<1>, dim3(blocks), dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL(nbest_trace_kernel<2>, dim3(blocks), dim3(256), 0, stream, p); break;
        case 4: hipLaunchKernelGGL(nbest_trace_kernel<4>, dim3(blocks), dim3(256), 0, stream, p); break;
        case 8: hipLaunchKernelGGL(nbest_trace_kernel<8>, dim3(blocks), dim3(256), 0, stream, p); break;
        case 16: hipLaunchKernelGGL(nbest_trace_kernel<16>, dim3(blocks), dim3(256), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_nbest_compact(const NbestParams& p, const uint64_t* out_offs, uint32_t* ids, uint32_t num_cus, hipStream_t stream) {
    const uint32_t blocks = grid_for(p.n_samples * p.k, 4, num_cus);
    hipLaunchKernelGGL(nbest_compact_kernel, dim3(blocks), dim3(256), 0, stream, p, out_offs, ids);
    return hipGetLastError();
}

hipError_t launch_offs_add(uint64_t* offs, uint64_t n, uint64_t add, hipStream_t stream) {
    const uint64_t want = (n + 1 + 255) / 256;
    const uint32_t blocks = (uint32_t)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(offs_add_kernel, dim3(blocks), dim3(256), 0, stream, offs, n, add);
    return hipGetLastError();
}

}  // namespace tgx
