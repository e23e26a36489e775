// Which samples of an encode pass go to encode6_kernel, and whether the two encode kernels run at once (encode_pass.cpp:
// split_long_samples), host side: the cost model over the batch's length distribution as a pure function.  No HIP call, no
// environment read: the caller parses the knobs.  tests/native/encode_split_main.cpp runs it under sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace tgx {

// What the pass knows about the batch, the device and the kernels' builds when it decides
struct EncodeSplitQuery {
    const uint32_t* sorted_len;  // the samples' lengths, descending: the long samples are a prefix of the order
    const uint64_t* sorted_cum;  // their running sums
    uint64_t n_samples;
    uint64_t n_bytes;
    uint64_t max_len;            // sorted_len[0] (0: no sample)
    int num_cus;
    bool cold6;                  // encode6_kernel's LDS copy does not hold every value
    int e6_bpc;                  // blocks of encode6_kernel per CU
    bool values_fit;             // every value fits encode5_kernel's LDS at 8 waves x 4 positions per lane
    bool corun_timeouts;         // a host wait for encode5_kernel's blocks has timed out on this model
    bool threshold_set;          // TGX_LONG_THRESHOLD is set ...
    uint64_t threshold;          // ... to this many bytes (0: never)
    bool corun_set;              // TGX_CORUN is set ...
    int corun;                   // ... to this many CUs (0: no co-run)
};

struct EncodeSplit {
    uint64_t n_long = 0;     // the n_long longest samples go to encode6_kernel
    uint32_t corun_cus = 0;  // CUs of encode6_kernel when both kernels run at once (0: one after the other)
};

inline EncodeSplit encode_split(const EncodeSplitQuery& q) {
    EncodeSplit s;
    if (!q.n_samples) return s;
    const auto count_ge = [&](uint64_t thr) {  // sorted_len descends: the long samples are a prefix of the order
        return (uint64_t)(std::partition_point(q.sorted_len, q.sorted_len + q.n_samples,
                                               [thr](uint32_t len) { return len >= thr; }) - q.sorted_len);
    };
    if (q.threshold_set) {
        const uint64_t thr = q.threshold;
        if (thr) s.n_long = count_ge(thr);
    } else {
        const double N = (double)q.n_bytes;
        // encode5_kernel's chain of a long sample on the few waves such a batch gets: 7.1 ms per 64 KiB with every
        // value in LDS, 8.7 ms with the COLD build (profiles/r03/l_*, o_*)
        const double c5 = !q.values_fit ? 0.135e-6 : 0.108e-6;
        auto cost = [&](uint64_t k) {  // the k longest samples to encode6_kernel
            const double bytes_long = k ? (double)q.sorted_cum[k - 1] : 0.0;
            const double t6 = k ? std::max((double)q.sorted_len[0] * (q.cold6 ? 0.042e-6 : 0.0369e-6), bytes_long / (q.cold6 ? 46e9 : 55e9)) + 20e-6 : 0.0;
            const double rest_max = k < q.n_samples ? (double)q.sorted_len[k] : 0.0;
            const double t5 = std::max(rest_max * c5, (N - bytes_long) / 88e9);
            return t6 + t5;
        };
        double best = cost(0);
        for (uint64_t thr = 1024; thr <= q.max_len; thr *= 2) {
            const uint64_t k = count_ge(thr);
            const double ck = cost(k);
            if (k && ck < best * 0.9) {  // switch for a clear gain only
                best = ck;
                s.n_long = k;
            }
        }
        // Both kernels at once, each on CUs of its own: between ~200 and ~450 MiB neither wins alone — the
        // long-sample kernel is bound by its eight relaxing rows per CU, encode5_kernel by the chains of the
        // longest samples.  `corun_cus` CUs (two blocks each) take the samples of at least thr bytes, the others
        // run encode5_kernel on the rest; its blocks are launched first and ask for more than half of a CU's
        // LDS, so no block of the other kernel shares their CU.  Estimates: a long-sample row does
        // 1 / 0.0369 us (0.042 us with cold values) per byte, a CU 55 (46) GB/s / 256; encode5_kernel 0.12 us
        // per byte of chain (measured beside the other kernel) and 70 GB/s x its share of the CUs.
        const double c6 = q.cold6 ? 0.042e-6 : 0.0369e-6, r6 = (q.cold6 ? 46e9 : 55e9) / (double)q.num_cus;
        double best_co = best * 0.9;
        uint64_t k_co = 0;
        static const uint64_t thrs[] = {8192, 12288, 16384, 24576, 32768, 40960, 49152};
        static const uint32_t shares[] = {32, 48, 64, 96, 128, 160, 192};
        // (only when encode5_kernel keeps every value in LDS on its few waves: its COLD builds are bound by the
        // chains of mid-length samples at twice the estimate — profiles/r03/p_corun_sweep*.txt)
        // (and never again after a pass whose host wait for encode5_kernel's blocks timed out: the device's atomic to
        // mapped host memory was not delivered, every co-run would pay the full 2 ms and lose the CU separation)
        const bool corun_off = (q.corun_set && q.corun == 0) || q.corun_timeouts || !q.values_fit;
        for (uint64_t thr : thrs) {
            if (corun_off || thr > q.max_len || q.e6_bpc != 2) break;
            const uint64_t k = count_ge(thr);
            if (!k || k >= q.n_samples) continue;
            const double bytes_long = (double)q.sorted_cum[k - 1];
            const double r_max = (double)q.sorted_len[k], r_bytes = N - bytes_long;
            for (uint32_t X : shares) {
                if ((int)X >= q.num_cus) break;
                const double t6 = std::max((double)q.sorted_len[0] * c6, bytes_long / (X * r6)) + 20e-6;
                const double t5 = std::max(r_max * 0.12e-6, r_bytes / ((double)(q.num_cus - (int)X) / (double)q.num_cus * 70e9));
                const double t = std::max(t5, t6);
                if (t < best_co) {
                    best_co = t;
                    k_co = k;
                    s.corun_cus = X;
                }
            }
        }
        if (s.corun_cus) s.n_long = k_co;
    }
    if (q.corun_set) {  // forces the share of the long-sample kernel (0: no co-run)
        const int v = q.corun;
        s.corun_cus = (v > 0 && v < q.num_cus && s.n_long > 0 && s.n_long < q.n_samples && q.e6_bpc == 2) ? (uint32_t)v : 0u;
    }
    return s;
}

}  // namespace tgx
