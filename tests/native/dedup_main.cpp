// Stand-alone driver of the deduplication twin (include/tgx.h: tgx_first_equal_host, tgx_row_hash) for a sanitizer build:
// tests/test_dedup_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (the elements, S + 1
// offsets, S entries of first), so that reading or writing one element too many is a report.  The shapes are the edge
// shapes of tests/dedup_cases.py: rows of 0, 1, 7, 8, 9, 15, 16, 17 elements, rows one to three elements on either side
// of one tile and of four (4096 bytes, 1024 ids), runs of empty rows at the start, in the middle and at the end, rows
// that differ in their last element, in their first or in a trailing zero, and a row that owns many tiles.  Every shape
// runs at hash_bits 64, 4, 1 and 0, and is checked against a plain comparison of every row with every earlier one.
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

// a row: its length, the content it draws (equal ids mean equal rows of that length), and what is done to one element
struct Row {
    uint64_t n;
    uint32_t content;
    int change;  // 0: none; 1: the last element is another; 2: the first; 3: the last is zero
};

template <class T>
void run(uint64_t run_id, const std::vector<Row>& rows) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<T> data;
    for (const Row& r : rows) {
        for (uint64_t t = 0; t < r.n; t++) data.push_back((T)(1 + ((t + 1) * 2654435761u + r.content * 40503u) % 250));
        if (r.n && r.change == 1) data.back() = (T)251;
        if (r.n && r.change == 2) data[data.size() - r.n] = (T)252;
        if (r.n && r.change == 3) data.back() = (T)0;
        offs.push_back(data.size());
    }
    const uint64_t S = rows.size();
    std::vector<int64_t> want(S);
    uint64_t want_unique = 0;
    for (uint64_t k = 0; k < S; k++) {
        want[k] = (int64_t)k;
        for (uint64_t i = 0; i < k; i++) {
            const uint64_t n = offs[k + 1] - offs[k];
            if (offs[i + 1] - offs[i] == n && (n == 0 || memcmp(&data[offs[i]], &data[offs[k]], n * sizeof(T)) == 0)) {
                want[k] = (int64_t)i;
                break;
            }
        }
        want_unique += want[k] == (int64_t)k;
    }
    const std::unique_ptr<T[]> b_data = block_of(data);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    for (uint32_t bits : {64u, 4u, 1u, 0u}) {
        std::unique_ptr<int64_t[]> first = block<int64_t>(S);
        uint64_t n_unique = ~0ull;
        uint32_t n_rounds = ~0u;
        const tgx_status st = tgx_first_equal_host(b_data.get(), (uint32_t)sizeof(T), b_offs.get(), S, bits, first.get(), &n_unique, &n_rounds);
        expect(st == TGX_OK, "status", run_id, (uint64_t)st, bits);
        if (st != TGX_OK) continue;
        for (uint64_t k = 0; k < S; k++) expect(first[k] == want[k], "first", run_id, k, bits);
        expect(n_unique == want_unique, "n_unique", run_id, n_unique, want_unique);
        expect(bits == 0 || S == 0 ? n_rounds == want_unique : n_rounds >= 1 && n_rounds <= want_unique, "n_rounds", run_id, n_rounds, bits);
    }
}

template <class T>
void run_all(uint64_t base, uint64_t tile) {
    std::vector<Row> small = {{0, 0, 0}, {0, 0, 0}};
    uint32_t c = 1;
    for (uint64_t n : {1, 7, 8, 9, 15, 16, 17}) {
        small.push_back({n, c, 0});
        small.push_back({n, c, 1});
        small.push_back({n, c, 2});
        small.push_back({n, c, 3});
        if (n == 9) small.insert(small.end(), {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}});
    }
    small.push_back({8, 3, 0});  // (a copy of an earlier row)
    small.insert(small.end(), {{0, 0, 0}, {0, 0, 0}});
    run<T>(base + 0, small);
    for (uint64_t m : {1, 4}) {
        std::vector<Row> edge;
        for (int d = -3; d <= 3; d++) edge.push_back({m * tile + d, 7, 0});
        edge.push_back({m * tile + 1, 7, 1});
        edge.push_back({m * tile - 2, 7, 0});
        edge.push_back({m * tile + 3, 7, 2});
        edge.push_back({0, 0, 0});
        run<T>(base + m, edge);
    }
    run<T>(base + 5, {{0, 0, 0}, {5, 1, 0}, {70000, 2, 0}, {0, 0, 0}, {70000, 2, 0}, {1026, 3, 0}, {70000, 2, 1}, {70000, 2, 0}, {0, 0, 0}});
    run<T>(base + 6, std::vector<Row>(30, Row{21, 4, 0}));
    run<T>(base + 7, {});
}

}  // namespace

int main() {
    run_all<uint8_t>(100, 4096);
    run_all<uint32_t>(200, 1024);
    // tgx_row_hash: a block of exactly n bytes, and the hash must tell trailing zeros apart
    for (uint64_t n : {0, 1, 7, 8, 9, 16, 17, 4099}) {
        std::unique_ptr<uint8_t[]> b = block<uint8_t>(n + 1);
        for (uint64_t t = 0; t < n; t++) b[t] = (uint8_t)(t * 31 + 5);
        b[n] = 0;
        std::unique_ptr<uint8_t[]> exact = block<uint8_t>(n);
        if (n) memcpy(exact.get(), b.get(), n);
        const uint64_t h = tgx_row_hash(exact.get(), n, 3);
        expect(h == tgx_row_hash(b.get(), n, 3), "row hash reads n bytes", n);
        expect(h != tgx_row_hash(b.get(), n + 1, 3), "row hash of a trailing zero", n);
        expect(h != tgx_row_hash(exact.get(), n, 4), "row hash seed", n);
    }
    // refused: offsets that do not start at 0 or descend, an element size of 3, 65 bits
    {
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 2};
        const uint8_t d[3] = {1, 2, 3};
        int64_t first[2] = {-7, -7};
        expect(tgx_first_equal_host(d, 1, bad0, 2, 64, first, nullptr, nullptr) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_first_equal_host(d, 1, bad1, 2, 64, first, nullptr, nullptr) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_first_equal_host(d, 3, good, 2, 64, first, nullptr, nullptr) == TGX_ERR_INVALID, "elem_bytes", 0);
        expect(tgx_first_equal_host(d, 1, good, 2, 65, first, nullptr, nullptr) == TGX_ERR_INVALID, "hash_bits", 0);
        expect(first[0] == -7 && first[1] == -7, "a refused call writes nothing", 0);
        expect(tgx_first_equal_host(d, 1, good, 2, 64, first, nullptr, nullptr) == TGX_OK && first[0] == 0 && first[1] == 1, "NULL counts", 0);
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("dedup twin: ok\n");
    return 0;
}
