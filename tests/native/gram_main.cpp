// Stand-alone driver of the shared n-gram twins (include/tgx.h: tgx_gram_keys_host, tgx_gram_hits_host,
// tgx_gram_contains_host, tgx_gram_key) for a sanitizer build: tests/test_gram_native.py compiles it with
// csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents (the elements, S + 1
// offsets, n_elems keys out, n_keys keys in, S counts, n_elems mask bytes), so that reading or writing one element too
// many is a report: an invalid position must load nothing, and the last row's last gram ends at the block's end.  The
// shapes are the edge shapes of tests/gram_cases.py: rows of 0 .. w + 2 elements for w = 1, 5, 13 and the widest (64
// bytes, 16 ids) between runs of empty rows, rows that end one to three elements on either side of a chunk of 64
// elements, of a tile of 256 and of two tiles, a row of about five tiles among short ones, a batch whose rows are all
// shorter than w.  Every answer is checked against the definitions written out plainly: every gram of every row through
// tgx_gram_key and tgx_row_hash, membership by a search over all the keys.
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

// the rows' lengths; row i draws its content from (i, t), and every third row repeats the row three before it
template <class T>
void run(uint64_t run_id, const std::vector<uint64_t>& lens, uint32_t w, uint64_t seed) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<T> data;
    for (uint64_t i = 0; i < lens.size(); i++) {
        const uint64_t c = i % 3 == 0 && i >= 3 ? i - 3 : i;
        for (uint64_t t = 0; t < lens[i]; t++) data.push_back((T)(1 + ((t + 1) * 2654435761u + c * 40503u) % 250));
        offs.push_back(data.size());
    }
    const uint64_t S = lens.size(), N = data.size();
    // the definitions, plainly: the key of every valid gram, and the set of the grams of the even rows
    std::vector<uint64_t> key(N, 0), set;
    std::vector<uint8_t> valid(N, 0);
    for (uint64_t i = 0; i < S; i++)
        for (uint64_t e = offs[i]; e + w <= offs[i + 1]; e++) {
            valid[e] = 1;
            key[e] = tgx_gram_key(reinterpret_cast<const uint8_t*>(data.data() + e), (uint64_t)w * sizeof(T), seed);
            expect(key[e] == tgx_row_hash(reinterpret_cast<const uint8_t*>(data.data() + e), (uint64_t)w * sizeof(T), seed ^ TGX_MINHASH_SALT), "gram_key", run_id, e);
            if (i % 2 == 0) set.push_back(key[e]);
        }
    std::vector<uint64_t> all;
    for (uint64_t e = 0; e < N; e++)
        if (valid[e]) all.push_back(key[e]);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    const std::unique_ptr<T[]> b_data = block_of(data);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    // keys: the source's own set
    std::unique_ptr<uint64_t[]> keys_out = block<uint64_t>(N);
    uint64_t n_keys = ~0ull;
    tgx_status st = tgx_gram_keys_host(b_data.get(), (uint32_t)sizeof(T), b_offs.get(), S, w, seed, keys_out.get(), &n_keys);
    expect(st == TGX_OK && n_keys == all.size(), "keys status / size", run_id, (uint64_t)st, n_keys);
    if (st != TGX_OK || n_keys != all.size()) return;
    for (uint64_t k = 0; k < n_keys; k++) expect(keys_out[k] == all[k], "key", run_id, k);
    // hits against the even rows' grams, handed over as they were met (unsorted, with duplicates); together and each alone
    const std::unique_ptr<uint64_t[]> b_set = block_of(set);
    std::vector<int64_t> want_count(S, 0);
    std::vector<uint8_t> want_mask(N, 0);
    for (uint64_t i = 0; i < S; i++)
        for (uint64_t e = offs[i]; e < offs[i + 1]; e++) {
            want_mask[e] = valid[e] && std::find(set.begin(), set.end(), key[e]) != set.end();
            want_count[i] += want_mask[e];
        }
    std::unique_ptr<int64_t[]> count = block<int64_t>(S), count_only = block<int64_t>(S);
    std::unique_ptr<uint8_t[]> mask = block<uint8_t>(N), mask_only = block<uint8_t>(N);
    const uint32_t eb = (uint32_t)sizeof(T);
    expect(tgx_gram_hits_host(b_data.get(), eb, b_offs.get(), S, w, seed, b_set.get(), set.size(), count.get(), mask.get()) == TGX_OK, "hits status", run_id);
    expect(tgx_gram_hits_host(b_data.get(), eb, b_offs.get(), S, w, seed, b_set.get(), set.size(), count_only.get(), nullptr) == TGX_OK, "count status", run_id);
    expect(tgx_gram_hits_host(b_data.get(), eb, b_offs.get(), S, w, seed, b_set.get(), set.size(), nullptr, mask_only.get()) == TGX_OK, "mask status", run_id);
    for (uint64_t i = 0; i < S; i++) expect(count[i] == want_count[i] && count_only[i] == want_count[i], "count", run_id, i, (uint64_t)count[i]);
    for (uint64_t e = 0; e < N; e++) expect(mask[e] == want_mask[e] && mask_only[e] == want_mask[e], "mask", run_id, e);
    // membership alone: every key of the source, and its two neighbours
    std::vector<uint64_t> probes;
    for (uint64_t k : all) probes.insert(probes.end(), {k, k + 1, k - 1});
    const std::unique_ptr<uint64_t[]> b_probes = block_of(probes);
    std::unique_ptr<uint8_t[]> found = block<uint8_t>(probes.size());
    expect(tgx_gram_contains_host(b_set.get(), set.size(), b_probes.get(), probes.size(), found.get()) == TGX_OK, "contains status", run_id);
    for (uint64_t p = 0; p < probes.size(); p++)
        expect(found[p] == (std::find(set.begin(), set.end(), probes[p]) != set.end()), "contains", run_id, p);
}

template <class T>
void run_all(uint64_t base, uint32_t w_max) {
    uint64_t id = base;
    for (uint32_t w : {1u, 5u, 13u, w_max}) {
        std::vector<uint64_t> small = {0, 0, 0};
        for (uint64_t n = 1; n <= w + 2; n++) {
            small.push_back(n);
            if (n == 3) small.insert(small.end(), {0, 0});
        }
        small.insert(small.end(), {w, w - 1, w + 1, 0, 0});
        run<T>(id++, small, w, w == 5 ? 3 : 0);
    }
    const uint32_t w = 5;
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
        run<T>(id++, lens, w, 0x9E3779B97F4A7C15ull);
    }
    run<T>(id++, {0, 7, 5 * 256 + 37, 1, 0, 30, 700, 12}, 13, 1);
    run<T>(id++, {0, 4, 1, 3, 0, 2, 4}, 5, 0);  // every row shorter than w: no key, no hit
    run<T>(id++, {}, 5, 0);
}

}  // namespace

int main() {
    run_all<uint8_t>(100, 64);
    run_all<uint32_t>(200, 16);
    // refused: offsets that do not start at 0 or descend, an element size of 3, the widths outside their ranges, no output
    {
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 3};
        const uint8_t d[3] = {1, 2, 3};
        uint64_t keys[3] = {9, 9, 9}, n_keys = 77;
        int64_t count[2] = {-7, -7};
        uint8_t mask[3] = {7, 7, 7};
        expect(tgx_gram_keys_host(d, 1, bad0, 2, 2, 0, keys, &n_keys) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_gram_keys_host(d, 1, bad1, 2, 2, 0, keys, &n_keys) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_gram_keys_host(d, 3, good, 2, 2, 0, keys, &n_keys) == TGX_ERR_INVALID, "elem_bytes", 0);
        expect(tgx_gram_keys_host(d, 1, good, 2, 0, 0, keys, &n_keys) == TGX_ERR_INVALID, "width 0", 0);
        expect(tgx_gram_keys_host(d, 1, good, 2, 65, 0, keys, &n_keys) == TGX_ERR_INVALID, "width 65", 0);
        expect(tgx_gram_keys_host(d, 4, good, 0, 17, 0, keys, &n_keys) == TGX_ERR_INVALID, "width 17 of ids", 0);
        expect(tgx_gram_hits_host(d, 1, good, 2, 0, 0, keys, 0, count, mask) == TGX_ERR_INVALID, "hits width 0", 0);
        expect(tgx_gram_hits_host(d, 1, bad1, 2, 2, 0, keys, 0, count, mask) == TGX_ERR_INVALID, "hits descending", 0);
        expect(tgx_gram_hits_host(d, 1, good, 2, 2, 0, keys, 0, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
        expect(tgx_gram_hits_host(d, 1, good, 2, 2, 0, nullptr, 2, count, mask) == TGX_ERR_INVALID, "keys NULL", 0);
        expect(keys[0] == 9 && keys[1] == 9 && keys[2] == 9 && count[0] == -7 && count[1] == -7 && mask[0] == 7 && mask[1] == 7 && mask[2] == 7,
               "a refused call writes nothing", 0);
        expect(tgx_gram_keys_host(d, 1, good, 2, 2, 0, keys, &n_keys) == TGX_OK && n_keys == 1, "one gram", 0, n_keys);
        expect(tgx_gram_hits_host(d, 1, good, 2, 2, 0, keys, 1, count, mask) == TGX_OK && count[0] == 0 && count[1] == 1 && mask[0] == 0 && mask[1] == 1 && mask[2] == 0,
               "the gram of the second row", 0);
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("gram twin: ok\n");
    return 0;
}
