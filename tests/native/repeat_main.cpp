// Stand-alone driver of the repetition twin (include/tgx.h: tgx_repeat_stats_host) for a sanitizer build:
// tests/test_repeat_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (the elements, S + 1
// offsets, 6 S statistics, n_elems mask bytes), so that reading or writing one element too many is a report: an invalid
// position must load nothing, the last row's last gram ends at the block's end, and the coverage window of the first
// chunk must not look in front of the flags.  The shapes are the edge shapes of tests/repeat_cases.py: rows of 0 .. w + 2
// elements for w = 1, 2, 5, 13 and the widest (64 bytes, 16 ids) between runs of empty rows, rows that end one to three
// elements on either side of a chunk of 64 elements, of a tile of 256 and of two tiles, a row of five tiles of one
// element, a batch whose rows are all shorter than w.  The content is over three symbols, so repeats are everywhere,
// and every answer is checked against the definitions written out plainly: grams compared element by element.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tgx.h"

namespace {

template <class T>
std::unique_ptr<T[]> block(size_t n) {  // exactly n elements; n = 0: a block no element of which may be touched
    return std::unique_ptr<T[]>(new T[n]);
}
template <class T>
std::unique_ptr<T[]> block_of(const std::vector<T>& v) {
    std::unique_ptr<T[]> b = block<T>(v.size());
    if (!v.empty()) memcpy(b.get(), v.data(), v.size() * sizeof(T));
    return b;
}

int g_failed = 0;
void expect(bool ok, const char* what, uint64_t run, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (run %llu: %llu, %llu)\n", what, (unsigned long long)run, (unsigned long long)a, (unsigned long long)b);
}

// the rows' lengths; symbols: the size of the alphabet the content is drawn from (1: a row of one element)
template <class T>
void run(uint64_t run_id, const std::vector<uint64_t>& lens, uint32_t w, uint64_t seed, uint32_t symbols) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<T> data;
    uint64_t x = 88172645463325252ull + run_id;
    for (uint64_t i = 0; i < lens.size(); i++) {
        for (uint64_t t = 0; t < lens[i]; t++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            data.push_back((T)(1 + (x >> 33) % symbols));
        }
        offs.push_back(data.size());
    }
    const uint64_t S = lens.size(), N = data.size();
    // the definitions, plainly
    std::vector<int64_t> want(6 * S, 0);
    std::vector<uint8_t> want_mask(N, 0);
    for (uint64_t i = 0; i < S; i++) {
        const uint64_t a = offs[i], n = offs[i + 1] - a, grams = n >= w ? n - w + 1 : 0;
        std::vector<uint64_t> members(grams, 0);
        std::vector<uint8_t> cov(n, 0), cov_all(n, 0);
        auto same = [&](uint64_t s, uint64_t t) { return std::equal(data.begin() + a + s, data.begin() + a + s + w, data.begin() + a + t); };
        int64_t top = 0;
        for (uint64_t t = 0; t < grams; t++) {
            bool earlier = false;
            for (uint64_t s = 0; s < grams; s++)
                if (same(s, t)) {
                    members[t]++;
                    earlier = earlier || s < t;
                }
            top = std::max(top, (int64_t)members[t]);
            if (earlier) want_mask[a + t] |= TGX_REPEAT_MASK_REPEAT;
            if (members[t] >= 2) want_mask[a + t] |= TGX_REPEAT_MASK_MULTI;
            for (uint32_t j = 0; j < w; j++) {
                if (earlier) cov[t + j] = 1;
                if (members[t] >= 2) cov_all[t + j] = 1;
            }
            want[1 * S + i] += earlier;
            want[2 * S + i] += members[t] >= 2;
        }
        want[0 * S + i] = (int64_t)grams;
        want[3 * S + i] = top;
        want[4 * S + i] = std::count(cov.begin(), cov.end(), 1);
        want[5 * S + i] = std::count(cov_all.begin(), cov_all.end(), 1);
    }
    const std::unique_ptr<T[]> b_data = block_of(data);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    std::unique_ptr<int64_t[]> stats = block<int64_t>(6 * S), stats_only = block<int64_t>(6 * S);
    std::unique_ptr<uint8_t[]> mask = block<uint8_t>(N), mask_only = block<uint8_t>(N);
    const uint32_t eb = (uint32_t)sizeof(T);
    expect(tgx_repeat_stats_host(b_data.get(), eb, b_offs.get(), S, w, seed, stats.get(), mask.get()) == TGX_OK, "status", run_id);
    expect(tgx_repeat_stats_host(b_data.get(), eb, b_offs.get(), S, w, seed, stats_only.get(), nullptr) == TGX_OK, "stats status", run_id);
    expect(tgx_repeat_stats_host(b_data.get(), eb, b_offs.get(), S, w, seed, nullptr, mask_only.get()) == TGX_OK, "mask status", run_id);
    if (S == 0) return;  // (nothing was written)
    for (uint64_t k = 0; k < 6 * S; k++) expect(stats[k] == want[k] && stats_only[k] == want[k], "stat", run_id, k, (uint64_t)stats[k]);
    for (uint64_t e = 0; e < N; e++) expect(mask[e] == want_mask[e] && mask_only[e] == want_mask[e], "mask", run_id, e, mask[e]);
}

template <class T>
void run_all(uint64_t base, uint32_t w_max) {
    uint64_t id = base;
    for (uint32_t w : {1u, 2u, 5u, 13u, w_max}) {
        std::vector<uint64_t> small = {0, 0, 0};
        for (uint64_t n = 1; n <= w + 2; n++) {
            small.push_back(n);
            if (n == 3) small.insert(small.end(), {0, 0});
        }
        small.insert(small.end(), {w, w - 1, w + 1, 0, 0});
        run<T>(id++, small, w, w == 5 ? 3 : 0, 2);
        run<T>(id++, {3, w + 1, 0, w + 40, 2}, w, 1, 1);  // rows of one element
    }
    for (uint32_t w : {5u, w_max}) {
        for (uint64_t edge : {64, 256, 512}) {
            std::vector<uint64_t> lens;
            uint64_t cum = 0;
            for (int d = -3; d <= 3; d++) {
                for (uint64_t n : {0, 2, 5, 6}) {
                    lens.push_back(n);
                    cum += n;
                }
                const uint64_t target = (cum / edge + 2) * edge + d;
                lens.push_back(target - cum);
                cum = target;
            }
            lens.push_back(3);
            run<T>(id++, lens, w, 0x9E3779B97F4A7C15ull, w == 5 ? 3 : 2);
        }
    }
    run<T>(id++, {0, 7, 5 * 256, 1, 0, 30, 12}, 13, 1, 1);  // five tiles of one element: one run of about 1 280
    run<T>(id++, {0, 4, 1, 3, 0, 2, 4}, 5, 0, 2);         // every row shorter than w: no gram
    run<T>(id++, {0, 0, 0}, 2, 0, 2);
    run<T>(id++, {}, 5, 0, 2);
}

}  // namespace

int main() {
    run_all<uint8_t>(100, 64);
    run_all<uint32_t>(200, 16);
    // refused: offsets that do not start at 0 or descend, an element size of 3, the widths outside their ranges, no output
    {
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 3};
        const uint8_t d[3] = {1, 2, 3};
        int64_t stats[12];
        uint8_t mask[3] = {7, 7, 7};
        std::fill(stats, stats + 12, -7);
        expect(tgx_repeat_stats_host(d, 1, bad0, 2, 2, 0, stats, mask) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_repeat_stats_host(d, 1, bad1, 2, 2, 0, stats, mask) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_repeat_stats_host(d, 3, good, 2, 2, 0, stats, mask) == TGX_ERR_INVALID, "elem_bytes", 0);
        expect(tgx_repeat_stats_host(d, 1, good, 2, 0, 0, stats, mask) == TGX_ERR_INVALID, "width 0", 0);
        expect(tgx_repeat_stats_host(d, 1, good, 2, 65, 0, stats, mask) == TGX_ERR_INVALID, "width 65", 0);
        expect(tgx_repeat_stats_host(d, 4, good, 0, 17, 0, stats, mask) == TGX_ERR_INVALID, "width 17 of ids", 0);
        expect(tgx_repeat_stats_host(d, 1, good, 2, 2, 0, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
        expect(tgx_repeat_stats_host(nullptr, 1, good, 2, 2, 0, stats, mask) == TGX_ERR_INVALID, "data NULL", 0);
        expect(std::count(stats, stats + 12, -7) == 12 && mask[0] == 7 && mask[1] == 7 && mask[2] == 7, "a refused call writes nothing", 0);
        expect(tgx_repeat_stats_host(d, 1, good, 2, 2, 0, stats, mask) == TGX_OK && stats[1] == 1 && stats[7] == 1 && mask[1] == 0, "one gram", 0);
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("repeat twin: ok\n");
    return 0;
}
