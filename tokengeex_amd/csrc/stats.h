// Per-sample lattice statistics (stats.hip): parameters and launchers used by lattice_pass.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tgx {

struct StatsParams {
    double alpha;                    // temperature: P(x) ∝ exp(alpha · Σ score)
    double* logz;                    // f64[S] A[n] of every sample, by sample index (-inf: no path)
    double* escore;                  // f64[S] E_P[Σ score] on the raw scores (NaN: no path)
    double* etokens;                 // f64[S] E_P[number of tokens] (NaN: no path)
    const double* wslot;             // rows kernel: f64[n_slots] exp(alpha · score) of terminal slots, 0 elsewhere
    unsigned long long* range_flag;  // rows kernel: set when a value left the range it holds exactly (init 0)
};

// stats_kernel: one wave per sample, log domain, any token length <= 64 (EncodeParams: text, offs, order, n_samples,
// trie, root_base, lm, queue (init 0))
hipError_t launch_stats(const EncodeParams& p, const StatsParams& q, uint32_t num_cus, hipStream_t stream);
// stats_rows_kernel: tokens <= 32 bytes, two samples per wave, linear domain; q.wslot from launch_sample_wslot
hipError_t launch_stats_rows(const EncodeParams& p, const StatsParams& q, uint32_t num_cus, hipStream_t stream);

}  // namespace tgx
