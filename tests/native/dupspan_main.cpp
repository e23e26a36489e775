// Stand-alone driver of the duplicate-span twin (include/tgx_dupspans.h: tgx_dup_spans_host) for a sanitizer build:
// tests/test_dupspan_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it; no
// device is opened.  Every buffer is a heap block of exactly the documented size, so one element too many is a report (the
// last gram's comparison, the walk back at slot 0, the first chunk's window).  Two symbols, so duplicates are everywhere
// and key_bits 1 mixes every run; the answers are checked against the definition, element by element.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/tgx_dupspans.h"

template <class T>
int run(const std::vector<uint64_t>& lens, uint32_t w) {
    const uint64_t S = lens.size();
    std::unique_ptr<uint64_t[]> offs(new uint64_t[S + 1]);
    offs[0] = 0;
    for (uint64_t i = 0; i < S; i++) offs[i + 1] = offs[i] + lens[i];
    const uint64_t N = offs[S];
    std::unique_ptr<T[]> data(new T[N]);
    uint64_t x = 88172645463325252ull + w;
    for (uint64_t e = 0; e < N; e++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        data[e] = (T)(1 + (x >> 33) % 2);
    }
    std::vector<uint8_t> want(N, 0);
    std::vector<uint64_t> starts;  // the valid grams before the one at hand
    for (uint64_t i = 0; i < S; i++)
        for (uint64_t e = offs[i]; e + w <= offs[i + 1]; starts.push_back(e++)) {
            bool earlier = false;
            for (size_t k = 0; k < starts.size() && !earlier; k++) earlier = std::equal(&data[e], &data[e] + w, &data[starts[k]]);
            if (earlier) want[e] |= TGX_DUPSPAN_MASK_DUP;
            for (uint32_t j = 0; earlier && j < w; j++) want[e + j] |= TGX_DUPSPAN_MASK_COVERED;
        }
    int failed = 0;
    for (uint32_t key_bits : {64u, 1u}) {
        std::unique_ptr<int64_t[]> table(new int64_t[3 * S]);
        std::unique_ptr<uint8_t[]> mask(new uint8_t[N]);
        failed += tgx_dup_spans_host(data.get(), (uint32_t)sizeof(T), offs.get(), S, w, key_bits, w, table.get(), mask.get()) != TGX_OK;
        failed += tgx_dup_spans_host(data.get(), (uint32_t)sizeof(T), offs.get(), S, w, key_bits, w, table.get(), nullptr) != TGX_OK;
        failed += !std::equal(want.begin(), want.end(), mask.get());
        for (uint64_t i = 0; i < S; i++) {
            const int64_t covered = std::count_if(&want[0] + offs[i], &want[0] + offs[i + 1], [](uint8_t m) { return (m & TGX_DUPSPAN_MASK_COVERED) != 0; });
            failed += table[2 * S + i] != covered || table[i] != (int64_t)(lens[i] >= w ? lens[i] - w + 1 : 0);
        }
    }
    return failed;
}

int main() {
    int failed = 0;
    for (uint32_t w : {1u, 5u, 16u}) {  // rows of 0 .. w + 2 elements among empty ones; rows that end around a chunk's and a tile's edge
        std::vector<uint64_t> lens = {0, 0};
        for (uint64_t n = 1; n <= w + 2; n++) lens.insert(lens.end(), {n, 0});
        for (uint64_t edge : {64, 256})
            for (int d = -1; d <= 1; d++) lens.insert(lens.end(), {w, 2 * edge - w + d});
        failed += run<uint8_t>(lens, w) + run<uint32_t>(lens, w) + run<uint8_t>(lens, 4 * w);
    }
    failed += run<uint8_t>({0, 4, 1, 3}, 5) + run<uint32_t>({}, 5);  // every row shorter than w; no row
    if (failed) return fprintf(stderr, "%d checks failed\n", failed), 1;
    printf("dupspan twin: ok\n");
    return 0;
}
