// Sampling a segmentation from the lattice (sample.hip): parameters and launchers used by lattice_pass.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tgx {

struct SampleParams {
    double alpha;                    // temperature: P(x) ∝ exp(alpha · Σ score)
    double* logz;                    // f64[S] A[n] of every sample, by sample index
    const double* wslot;             // rows kernel: f64[n_slots] exp(alpha · score) of terminal slots, 0 elsewhere
    unsigned long long* range_flag;  // rows kernel: set when a value left the range it holds exactly (init 0)
};

// sample_kernel: one wave per sample, log domain, any token length <= 64 (EncodeParams: text, offs, order, n_samples,
// trie, tokid, root_base, n_slots, lm, bp, tmp, counts, err_sample, seed)
hipError_t launch_sample(const EncodeParams& p, const SampleParams& q, uint32_t num_cus, hipStream_t stream);
// q.wslot for sample_rows_kernel
hipError_t launch_sample_wslot(const void* trie, uint32_t n_slots, double alpha, double* out, hipStream_t stream);
// sample_rows_kernel: tokens <= 32 bytes, plain back-pointer bytes + status for trace32_kernel (EncodeParams as
// encode2_kernel's: ... bp8, status, queue (init 0))
hipError_t launch_sample_rows(const EncodeParams& p, const SampleParams& q, uint32_t num_cus, hipStream_t stream);

}  // namespace tgx
