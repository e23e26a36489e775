// Stand-alone driver of the near-duplicate twins (include/tgx.h: tgx_minhash_host, tgx_minhash_bands_host,
// tgx_minhash_near_first_host, tgx_minhash_value) for a sanitizer build: tests/test_minhash_native.py compiles it with
// csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents (the elements, S + 1
// offsets, S·K signature values, S·B keys and heads, S entries of first), so that reading or writing one element too
// many is a report.  The shapes are the edge shapes of tests/minhash_cases.py: rows of 0 .. w + 2 elements for w = 1, 5
// and the widest (64 bytes, 16 ids) between runs of empty rows, rows that end one to three positions on either side of
// a chunk of 64 shingle positions, of a tile of 256 and of four tiles, a row that owns about five tiles among short
// rows, a row of one repeated element, rows that differ in trailing zeros.  Every answer is checked against the
// definitions written out plainly: every shingle of every row through tgx_row_hash and tgx_minhash_value, every key
// through tgx_row_hash, every head and every chain by a search over all earlier rows.
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

// a row: its length, the content it draws (equal numbers mean equal prefixes), and how many zero elements follow
struct Row {
    uint64_t n;
    uint32_t content;
    uint32_t zeros;
};

template <class T>
void run(uint64_t run_id, const std::vector<Row>& rows, uint32_t w, uint32_t K, uint32_t B, uint64_t seed) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<T> data;
    for (const Row& r : rows) {
        for (uint64_t t = 0; t < r.n; t++) data.push_back(r.content == 99 ? (T)7 : (T)(1 + ((t + 1) * 2654435761u + r.content * 40503u) % 250));
        for (uint32_t z = 0; z < r.zeros; z++) data.push_back((T)0);
        offs.push_back(data.size());
    }
    const uint64_t S = rows.size();
    // the definitions, plainly
    std::vector<uint32_t> want((size_t)S * K, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < S; i++) {
        const uint64_t n = offs[i + 1] - offs[i], m = n >= w ? n - w + 1 : 1, len = n < w ? n : w;
        for (uint64_t t = 0; t < m; t++) {
            const uint64_t h = tgx_row_hash(reinterpret_cast<const uint8_t*>(data.data() + offs[i] + t), len * sizeof(T), seed ^ TGX_MINHASH_SALT);
            for (uint32_t k = 0; k < K; k++) want[i * K + k] = std::min(want[i * K + k], tgx_minhash_value(h, k, seed));
        }
    }
    const std::unique_ptr<T[]> b_data = block_of(data);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    std::unique_ptr<uint32_t[]> sig = block<uint32_t>((size_t)S * K);
    tgx_status st = tgx_minhash_host(b_data.get(), (uint32_t)sizeof(T), b_offs.get(), S, w, K, seed, sig.get());
    expect(st == TGX_OK, "minhash status", run_id, (uint64_t)st);
    if (st != TGX_OK) return;
    for (uint64_t x = 0; x < S * K; x++) expect(sig[x] == want[x], "sig", run_id, x / K, x % K);
    // bands: keys and heads, together and each alone
    const uint32_t r = K / B;
    std::vector<uint64_t> want_keys((size_t)S * B);
    std::vector<int64_t> want_heads((size_t)S * B);
    for (uint64_t i = 0; i < S; i++)
        for (uint32_t b = 0; b < B; b++) {
            want_keys[i * B + b] = tgx_row_hash(reinterpret_cast<const uint8_t*>(&want[i * K + (uint64_t)b * r]), 4ull * r, (seed ^ TGX_MINHASH_SALT) + b + 1);
            uint64_t j = 0;
            while (want_keys[j * B + b] != want_keys[i * B + b]) j++;
            want_heads[i * B + b] = (int64_t)j;
        }
    std::unique_ptr<uint64_t[]> keys = block<uint64_t>((size_t)S * B), keys_only = block<uint64_t>((size_t)S * B);
    std::unique_ptr<int64_t[]> heads = block<int64_t>((size_t)S * B), heads_only = block<int64_t>((size_t)S * B);
    expect(tgx_minhash_bands_host(sig.get(), S, K, B, seed, keys.get(), heads.get()) == TGX_OK, "bands status", run_id);
    expect(tgx_minhash_bands_host(sig.get(), S, K, B, seed, keys_only.get(), nullptr) == TGX_OK, "keys status", run_id);
    expect(tgx_minhash_bands_host(sig.get(), S, K, B, seed, nullptr, heads_only.get()) == TGX_OK, "heads status", run_id);
    for (uint64_t x = 0; x < S * B; x++) {
        expect(keys[x] == want_keys[x] && keys_only[x] == want_keys[x], "key", run_id, x / B, x % B);
        expect(heads[x] == want_heads[x] && heads_only[x] == want_heads[x], "head", run_id, x / B, x % B);
    }
    // clusters
    for (uint32_t min_agree : {1u, (K + 1) / 2, K}) {
        std::vector<int64_t> first0(S), want_first(S);
        uint64_t want_clusters = 0;
        for (uint64_t i = 0; i < S; i++) {
            first0[i] = (int64_t)i;
            for (uint32_t b = 0; b < B; b++) {
                const int64_t j = want_heads[i * B + b];
                if (j >= first0[i]) continue;
                uint32_t agree = 0;
                for (uint32_t k = 0; k < K; k++) agree += want[i * K + k] == want[(uint64_t)j * K + k];
                if (agree >= min_agree) first0[i] = j;
            }
            want_first[i] = first0[i] == (int64_t)i ? (int64_t)i : want_first[first0[i]];
            want_clusters += want_first[i] == (int64_t)i;
        }
        std::unique_ptr<int64_t[]> first = block<int64_t>(S);
        uint64_t n_clusters = ~0ull;
        st = tgx_minhash_near_first_host(sig.get(), S, K, heads.get(), B, min_agree, first.get(), &n_clusters);
        expect(st == TGX_OK, "near_first status", run_id, (uint64_t)st, min_agree);
        if (st != TGX_OK) continue;
        for (uint64_t i = 0; i < S; i++) expect(first[i] == want_first[i], "first", run_id, i, min_agree);
        expect(n_clusters == want_clusters, "n_clusters", run_id, n_clusters, want_clusters);
    }
}

template <class T>
void run_all(uint64_t base, uint32_t w_max) {
    uint64_t id = base;
    for (uint32_t w : {1u, 5u, w_max}) {
        std::vector<Row> small = {{0, 0, 0}, {0, 0, 0}};
        for (uint64_t n = 1; n <= w + 2; n++) {
            small.push_back({n, 1, 0});
            if (n == 3) small.insert(small.end(), {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}});
        }
        small.insert(small.end(), {{2, 1, 0}, {2, 1, 1}, {2, 1, 2}, {w + 1, 1, 0}, {0, 0, 0}, {0, 0, 0}});
        run<T>(id++, small, w, w == 1 ? 1 : 65, w == 1 ? 1 : 13, 0);
    }
    const uint32_t w = 5;
    for (uint64_t edge : {64, 256, 1024}) {
        std::vector<Row> rows;
        uint64_t cum = 0;
        for (int d = -3; d <= 3; d++) {
            for (uint64_t n : {0, 2, 5, 6}) {
                rows.push_back({n, 2, 0});
                cum += n >= w ? n - w + 1 : 1;
            }
            const uint64_t target = (cum / edge + 2) * edge + d;
            rows.push_back({target - cum + w - 1, (uint32_t)(3 + d + 3), 0});
            cum = target;
        }
        rows.push_back({3, 2, 0});
        run<T>(id++, rows, w, 64, 16, 3);
    }
    run<T>(id++, {{0, 0, 0}, {7, 1, 0}, {5 * 256 + 37 + 4, 2, 0}, {1, 3, 0}, {0, 0, 0}, {30, 4, 0}, {700, 2, 0}, {300, 99, 0}, {77, 99, 0}, {40, 5, 0}, {40, 5, 1}, {40, 5, 2}},
           w, 128, 32, 0x9E3779B97F4A7C15ull);
    run<T>(id++, {{21, 4, 0}, {21, 4, 0}, {21, 4, 0}, {0, 0, 0}, {0, 0, 0}}, 3, 250, 25, 1);
    run<T>(id++, {}, 5, 128, 32, 0);
}

}  // namespace

int main() {
    run_all<uint8_t>(100, 64);
    run_all<uint32_t>(200, 16);
    // refused: offsets that do not start at 0 or descend, an element size of 3, the widths and counts outside their ranges
    {
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 2};
        const uint8_t d[3] = {1, 2, 3};
        uint32_t sig[4] = {7, 7, 7, 7};
        expect(tgx_minhash_host(d, 1, bad0, 2, 2, 2, 0, sig) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_minhash_host(d, 1, bad1, 2, 2, 2, 0, sig) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_minhash_host(d, 3, good, 2, 2, 2, 0, sig) == TGX_ERR_INVALID, "elem_bytes", 0);
        expect(tgx_minhash_host(d, 1, good, 2, 0, 2, 0, sig) == TGX_ERR_INVALID, "width 0", 0);
        expect(tgx_minhash_host(d, 1, good, 2, 65, 2, 0, sig) == TGX_ERR_INVALID, "width 65", 0);
        expect(tgx_minhash_host(d, 1, good, 2, 2, 0, 0, sig) == TGX_ERR_INVALID, "n_perm 0", 0);
        expect(tgx_minhash_host(d, 1, good, 2, 2, 1025, 0, sig) == TGX_ERR_INVALID, "n_perm 1025", 0);
        expect(sig[0] == 7 && sig[1] == 7 && sig[2] == 7 && sig[3] == 7, "a refused call writes nothing", 0);
        uint64_t keys[2] = {9, 9};
        expect(tgx_minhash_bands_host(sig, 2, 2, 0, 0, keys, nullptr) == TGX_ERR_INVALID, "bands 0", 0);
        expect(tgx_minhash_bands_host(sig, 1, 4, 3, 0, keys, nullptr) == TGX_ERR_INVALID, "bands 3 of 4", 0);
        expect(tgx_minhash_bands_host(sig, 2, 2, 2, 0, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
        expect(keys[0] == 9 && keys[1] == 9, "a refused call writes nothing", 1);
        int64_t heads[4] = {0, 0, 0, 0}, first[2] = {-7, -7};
        expect(tgx_minhash_near_first_host(sig, 2, 2, heads, 2, 0, first, nullptr) == TGX_ERR_INVALID, "min_agree 0", 0);
        expect(tgx_minhash_near_first_host(sig, 2, 2, heads, 2, 3, first, nullptr) == TGX_ERR_INVALID, "min_agree 3 of 2", 0);
        expect(first[0] == -7 && first[1] == -7, "a refused call writes nothing", 2);
        const int64_t wild[4] = {5, -1, 99, (int64_t)1 << 40};  // heads that are no earlier row are never followed
        expect(tgx_minhash_near_first_host(sig, 2, 2, wild, 2, 1, first, nullptr) == TGX_OK && first[0] == 0 && first[1] == 1, "wild heads", 0);
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("minhash twin: ok\n");
    return 0;
}
