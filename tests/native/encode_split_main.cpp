// Stand-alone driver of the encode pass's long-sample split (csrc/encode_split.h) for a sanitizer build:
// tests/test_encode_split_native.py compiles it under -fsanitize=address,undefined and runs it.  No device is opened.
//
// It checks the properties that follow from the function's code on fixed and random batches, with every knob, and prints
// the decision for a list of batches (built in, and one per file of sample offsets named on the command line: raw
// little-endian u64) at 256 CUs and two blocks of encode6_kernel per CU, which the pytest compares with decisions
// recorded from the code the header was lifted from.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../tokengeex_amd/csrc/encode_split.h"

namespace {

int g_failed = 0;
void expect(bool ok, const char* what, const char* batch) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (%s)\n", what, batch);
}

// A batch as the pass sees it: lengths descending and their running sums, in heap blocks of exactly n elements — an
// access past either end is a report.
struct Batch {
    std::string name;
    uint64_t n = 0, bytes = 0, max_len = 0;
    std::unique_ptr<uint32_t[]> len;
    std::unique_ptr<uint64_t[]> cum;
};

Batch make_batch(const std::string& name, std::vector<uint32_t> lens) {
    std::stable_sort(lens.begin(), lens.end(), std::greater<uint32_t>());
    Batch b;
    b.name = name;
    b.n = lens.size();
    b.len.reset(new uint32_t[b.n]);
    b.cum.reset(new uint64_t[b.n]);
    for (uint64_t i = 0; i < b.n; i++) {
        b.len[i] = lens[i];
        b.bytes += lens[i];
        b.cum[i] = b.bytes;
    }
    b.max_len = b.n ? b.len[0] : 0;
    return b;
}

tgx::EncodeSplitQuery query(const Batch& b, int num_cus, int e6_bpc, bool cold6, bool fit) {
    tgx::EncodeSplitQuery q{};
    q.sorted_len = b.len.get();
    q.sorted_cum = b.cum.get();
    q.n_samples = b.n;
    q.n_bytes = b.bytes;
    q.max_len = b.max_len;
    q.num_cus = num_cus;
    q.cold6 = cold6;
    q.e6_bpc = e6_bpc;
    q.values_fit = fit;
    return q;
}

void check_common(const tgx::EncodeSplitQuery& q, const tgx::EncodeSplit& s, const char* name) {
    expect(s.n_long <= q.n_samples, "n_long <= n_samples", name);
    if (s.corun_cus > 0) {
        expect(s.n_long > 0 && s.n_long < q.n_samples, "a co-run splits the batch", name);
        expect((int)s.corun_cus < q.num_cus, "a co-run leaves CUs for encode5_kernel", name);
        expect(q.e6_bpc == 2, "a co-run has two blocks of encode6_kernel per CU", name);
    }
}

void check_properties(const Batch& b) {
    const char* name = b.name.c_str();
    for (int num_cus : {256, 64, 32, 1})
        for (int e6_bpc : {2, 1, 4})
            for (int variant = 0; variant < 4; variant++) {
                const bool cold6 = variant & 1, fit = !(variant & 2);
                const tgx::EncodeSplitQuery base = query(b, num_cus, e6_bpc, cold6, fit);
                const tgx::EncodeSplit by_estimate = tgx::encode_split(base);
                check_common(base, by_estimate, name);
                if (!fit) expect(by_estimate.corun_cus == 0, "values that do not fit: no co-run by estimate", name);
                {
                    auto q = base;
                    q.corun_timeouts = true;
                    const tgx::EncodeSplit s = tgx::encode_split(q);
                    check_common(q, s, name);
                    expect(s.corun_cus == 0, "timeouts recorded: no co-run by estimate", name);
                }
                // ---- a forced threshold
                for (uint64_t thr : {(uint64_t)0, (uint64_t)1, (uint64_t)1024, (uint64_t)8192, b.max_len, b.max_len + 1, (uint64_t)1 << 62}) {
                    auto q = base;
                    q.threshold_set = true;
                    q.threshold = thr;
                    const tgx::EncodeSplit s = tgx::encode_split(q);
                    check_common(q, s, name);
                    expect(s.corun_cus == 0, "a forced threshold alone: no co-run", name);
                    if (thr == 0) expect(s.n_long == 0, "threshold 0: no long sample", name);
                    if (thr > b.max_len) expect(s.n_long == 0, "a threshold above the longest sample: no long sample", name);
                    if (thr == 1) {
                        uint64_t non_empty = 0;
                        while (non_empty < b.n && b.len[non_empty] >= 1) non_empty++;
                        expect(s.n_long == non_empty, "threshold 1: every sample with a byte goes to encode6_kernel", name);
                    }
                    uint64_t direct = 0;  // and in general: the count of samples of at least thr bytes
                    for (uint64_t i = 0; i < b.n && thr; i++) direct += b.len[i] >= thr;
                    expect(s.n_long == direct, "a forced threshold counts the samples at or above it", name);
                }
                // ---- a forced co-run
                for (int v : {0, -3, 1, 32, num_cus - 1, num_cus, num_cus + 7}) {
                    for (int with_thr = 0; with_thr < 2; with_thr++) {
                        auto q = base;
                        q.corun_set = true;
                        q.corun = v;
                        q.threshold_set = with_thr;
                        q.threshold = 8192;
                        q.corun_timeouts = with_thr;  // (a forced share holds whatever the estimate may use)
                        const tgx::EncodeSplit s = tgx::encode_split(q);
                        check_common(q, s, name);
                        if (v <= 0 || v >= num_cus) expect(s.corun_cus == 0, "a forced co-run of 0 or of every CU: none", name);
                        const bool can = v > 0 && v < num_cus && s.n_long > 0 && s.n_long < b.n && e6_bpc == 2;
                        expect(s.corun_cus == (can ? (uint32_t)v : 0u), "a forced co-run holds where the batch is split", name);
                    }
                }
            }
}

std::vector<uint32_t> repeat(uint64_t n, uint32_t len) { return std::vector<uint32_t>(n, len); }

std::vector<uint32_t> lengths_of_offsets(const char* path) {
    std::vector<uint32_t> lens;
    FILE* f = fopen(path, "rb");
    if (!f) return lens;
    std::vector<uint64_t> offs;
    uint64_t buf[4096];
    size_t got;
    while ((got = fread(buf, 8, 4096, f)) > 0) offs.insert(offs.end(), buf, buf + got);
    fclose(f);
    for (size_t i = 0; i + 1 < offs.size(); i++) lens.push_back((uint32_t)(offs[i + 1] - offs[i]));
    return lens;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<Batch> cases;
    cases.push_back(make_batch("empty", {}));
    for (uint32_t len : {1023u, 1024u, 65536u, 1u << 20}) cases.push_back(make_batch("one_" + std::to_string(len), {len}));
    cases.push_back(make_batch("short_100000x140", repeat(100000, 140)));
    {
        std::vector<uint32_t> l = repeat(100000, 140);
        l.push_back(65536);
        cases.push_back(make_batch("short_plus_65536", l));
    }
    {
        std::vector<uint32_t> l = repeat(100000, 140);
        l.push_back(8192);
        l.push_back(8191);
        cases.push_back(make_batch("short_plus_8192_8191", l));
    }
    cases.push_back(make_batch("long_64x49152", repeat(64, 49152)));
    {
        std::vector<uint32_t> l;
        for (uint32_t len = 1024; len <= (1u << 20); len *= 2)
            for (int i = 0; i < 4; i++) l.push_back(len);
        cases.push_back(make_batch("ladder_1KiB_1MiB_x4", l));
    }
    for (int i = 1; i < argc; i++) {
        const char* slash = strrchr(argv[i], '/');
        std::vector<uint32_t> l = lengths_of_offsets(argv[i]);
        if (l.empty()) {
            fprintf(stderr, "FAILED no offsets in %s\n", argv[i]);
            return 2;
        }
        cases.push_back(make_batch(slash ? slash + 1 : argv[i], l));
    }
    // ---- the decisions the pytest compares with the recorded ones
    for (const Batch& b : cases)
        for (int cold6 = 0; cold6 < 2; cold6++)
            for (int fit = 1; fit >= 0; fit--) {
                const tgx::EncodeSplit s = tgx::encode_split(query(b, 256, 2, cold6 != 0, fit != 0));
                printf("split %s cold6=%d fit=%d n_long=%llu corun_cus=%u\n", b.name.c_str(), cold6, fit, (unsigned long long)s.n_long, s.corun_cus);
            }
    // ---- the properties: the cases above, and random batches around the thresholds
    for (const Batch& b : cases)
        if (b.n <= 200000) check_properties(b);
    {
        std::mt19937_64 rng(20261020);
        for (int trial = 0; trial < 60; trial++) {
            const size_t n = 1 + (size_t)(rng() % (trial < 20 ? 8 : 3000));
            const int top = 10 + (int)(rng() % 11);  // longest sample below 2^10 .. 2^20
            std::vector<uint32_t> l(n);
            for (uint32_t& x : l) x = (uint32_t)(rng() % (1ull << (6 + rng() % (uint64_t)(top - 5))));
            if (trial % 3 == 0) l[0] = 8192;
            check_properties(make_batch("random_" + std::to_string(trial), l));
        }
    }
    if (g_failed) return 1;
    printf("encode split: ok\n");
    return 0;
}
