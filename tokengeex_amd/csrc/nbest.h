// N-best segmentation (nbest.hip): parameters and launchers used by lattice_pass.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

// Back-pointer of list entry (p, r): (64 - len) << 26 | r' << 22 | id, the last token (id, len) and the rank r' of the
// list at p - len it extends.  Compared as an integer it orders equal scores by q = p - len ascending, then r'.
constexpr uint32_t kNbestIdBits = 22;
constexpr uint32_t kNbestMaxVocab = 1u << kNbestIdBits;

struct NbestParams {
    const uint8_t* text;            // the corpus
    const uint64_t* offs;           // u64[S+1] (the corpus's)
    const uint32_t* order;          // u32[n_samples] the chunk's samples, longest first (global sample indices)
    uint64_t n_samples;             // samples of the chunk
    uint64_t s0, byte0;             // its first sample and that sample's first byte
    uint64_t chunk_bytes;           // its bytes
    const void* trie;               // TrieRec[n_slots] (16 B each)
    const uint32_t* tokid;          // u32[n_slots]
    uint32_t root_base, n_slots, lm;
    uint32_t k;                     // rows per sample (<= the kernel's K)
    uint32_t* bp;                   // u32[(chunk_bytes + n_samples) · K]: sample s, position p at ((offs[s] − byte0) + (s − s0) + p) · K
    uint32_t* tmp;                  // u32[k · chunk_bytes]: row r's ids right-aligned at r · chunk_bytes + offs[s] − byte0
    uint32_t* counts;               // u32[n_samples · k] ids per row, the chunk's rows
    double* scores;                 // f64[S · k] L[n][r].score (−inf past the list), by global row
    uint32_t* n_found;              // u32[S]
    unsigned long long* err_sample; // min failing sample (init ~0); | 1 << 62: corrupt back-pointer
};

// forward sweep (back-pointers, scores, n_found) for K in {1, 2, 4, 8, 16}, K >= p.k
hipError_t launch_nbest(const NbestParams& p, uint32_t K, uint32_t num_cus, hipStream_t stream);
// back-traces of the chunk's rows into tmp / counts
hipError_t launch_nbest_trace(const NbestParams& p, uint32_t K, uint32_t num_cus, hipStream_t stream);
// rows of tmp -> ids[out_offs[R] ..) (out_offs: the chunk's rows, from 0)
hipError_t launch_nbest_compact(const NbestParams& p, const uint64_t* out_offs, uint32_t* ids, uint32_t num_cus, hipStream_t stream);
// offs[i] += add for i in [0, n]
hipError_t launch_offs_add(uint64_t* offs, uint64_t n, uint64_t add, hipStream_t stream);

}  // namespace tgx
