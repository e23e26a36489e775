// Stand-alone driver of the selection twins (include/tgx.h: tgx_select_host, tgx_select_text_host, tgx_shuffled_rows_host)
// for a sanitizer build: tests/test_select_native.py compiles it with csrc/host_twins.cpp under
// -fsanitize=address,undefined and runs it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents (T elements and S + 1 offsets
// in, M indices; T' elements and M + 1 offsets out), so that reading or writing one element too many is a report.  The
// shapes put the end of the output one to three positions on either side of a tile (1024 ids, 4096 bytes), with empty rows
// at the start, in the middle and at the end, a row that owns whole tiles, and byte rows of 13 .. 19 bytes so that slots
// of 16 bytes straddle row boundaries at every residue.
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

tgx_status twin(const uint32_t* d, const uint64_t* o, uint64_t S, const int64_t* r, uint64_t M, uint32_t* out, uint64_t cap, uint64_t* oo) {
    return tgx_select_host(d, o, S, r, M, out, cap, oo);
}
tgx_status twin(const uint8_t* d, const uint64_t* o, uint64_t S, const int64_t* r, uint64_t M, uint8_t* out, uint64_t cap, uint64_t* oo) {
    return tgx_select_text_host(d, o, S, r, M, out, cap, oo);
}

template <class T>
void run(uint64_t run_id, const std::vector<uint64_t>& sizes, const std::vector<int64_t>& rows) {
    std::vector<uint64_t> offs(1, 0);
    for (uint64_t n : sizes) offs.push_back(offs.back() + n);
    const uint64_t S = sizes.size(), N = offs.back(), M = rows.size();
    std::vector<T> data(N);
    for (uint64_t j = 0; j < N; j++) data[j] = (T)(1 + (j * 2654435761u >> 7) % 250);
    const std::unique_ptr<T[]> b_data = block_of(data);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    const std::unique_ptr<int64_t[]> b_rows = block_of(rows);
    uint64_t T2 = 0;
    for (int64_t r : rows) T2 += sizes[(size_t)r];
    std::unique_ptr<uint64_t[]> out_offs = block<uint64_t>(M + 1);
    tgx_status st;
    if (T2 > 0) {  // one element short: refused, and the destination is not touched
        std::unique_ptr<T[]> small = block<T>(T2 - 1);
        st = twin(b_data.get(), b_offs.get(), S, b_rows.get(), M, small.get(), T2 - 1, out_offs.get());
        expect(st == TGX_ERR_INVALID, "a destination one element short", run_id, st);
    }
    std::unique_ptr<T[]> out = block<T>(T2);
    st = twin(b_data.get(), b_offs.get(), S, b_rows.get(), M, out.get(), T2, out_offs.get());
    expect(st == TGX_OK, "select", run_id, st);
    if (st != TGX_OK) return;
    expect(out_offs[0] == 0 && out_offs[M] == T2, "totals", run_id, out_offs[M], T2);
    for (uint64_t k = 0; k < M; k++) {
        const uint64_t n = sizes[(size_t)rows[k]], o = out_offs[k];
        expect(out_offs[k + 1] - o == n && (n == 0 || memcmp(out.get() + o, data.data() + offs[(size_t)rows[k]], n * sizeof(T)) == 0), "a selected row", run_id,
               k, n);
    }
}

template <class T>
int shapes(uint64_t tile) {
    int n_runs = 0;
    for (uint64_t k = 0; k < 42; k++) {
        // rows around a slot, one and four tiles of ids, a tile of bytes; empty rows at both ends and in the middle; the
        // last non-empty row is sized so that the selection ends tile·m + d, d = -3 .. 3
        std::vector<uint64_t> sizes = {0, 0, 1 + k % 3, 13 + k % 7, 1019 + k % 11, 0, 0, 0, 4090 + k % 13, 3, 17};
        const uint64_t special = sizes.size();
        sizes.push_back(1);
        sizes.push_back(0);
        if (k % 2) sizes.push_back(0);
        std::vector<int64_t> rows;
        const uint64_t S = sizes.size();
        switch (k % 6) {
            case 0: for (uint64_t i = 0; i < S; i++) rows.push_back((int64_t)i); break;
            case 1: for (uint64_t i = S; i-- > 0;) rows.push_back((int64_t)i); break;
            case 2: for (uint64_t i = 1; i < S; i += 1 + (i % 2)) rows.push_back((int64_t)i); rows.push_back((int64_t)special); break;
            case 3: for (uint64_t i = 0; i < S; i++) rows.push_back((int64_t)i); for (int q = 0; q < 3; q++) rows.push_back(3); break;
            case 4: rows = {0, 1, 5, 6, 7, 0, (int64_t)S - 1}; break;
            default: for (uint64_t q = 0; q < 2 * S; q++) rows.push_back((int64_t)((q * 7 + k) % special)); rows.insert(rows.begin() + (long)(k % rows.size()), (int64_t)special); break;
        }
        if (k % 6 == 2) {  // (the walk above may have taken the special row already: once is what is wanted)
            uint64_t c = 0;
            for (int64_t r : rows) c += (uint64_t)r == special;
            if (c == 2) rows.pop_back();
        }
        if (k % 6 != 4) {
            uint64_t cur = 0;
            for (int64_t r : rows) cur += (uint64_t)r == special ? 0 : sizes[(size_t)r];
            const int64_t d = (int64_t)(k % 7) - 3;
            const uint64_t target = (cur + 1 + 3 + tile - 1) / tile * tile + (uint64_t)d;
            sizes[special] = target - cur;
        }
        run<T>(k, sizes, rows);
        n_runs++;
    }
    run<T>(100, {0, 5, 70000, 0, 1026}, {2, 1, 2, 3, 2, 4});  // a row that owns whole tiles, three times
    run<T>(101, {7}, {0, 0, 0});
    run<T>(102, {0}, {0});
    run<T>(103, {0, 0, 0}, {2, 1, 0, 0});
    run<T>(104, {5, 6}, {});
    run<T>(105, {}, {});
    return n_runs + 6;
}

}  // namespace

int main() {
    int n_runs = shapes<uint32_t>(1024) + shapes<uint8_t>(4096);
    // arguments that are refused before anything is touched
    const uint64_t offs3[3] = {0, 2, 5};
    const std::unique_ptr<uint32_t[]> ids = block<uint32_t>(5);
    for (int j = 0; j < 5; j++) ids[j] = (uint32_t)j;
    std::unique_ptr<uint32_t[]> none = block<uint32_t>(0);
    std::unique_ptr<uint64_t[]> two = block<uint64_t>(2);
    const int64_t neg = -1, at_s = 2, big = (int64_t)1 << 62, zero = 0;
    tgx_status st = tgx_select_host(ids.get(), offs3, 2, &neg, 1, none.get(), 0, two.get());
    expect(st == TGX_ERR_INVALID, "a negative index", 0, st);
    st = tgx_select_host(ids.get(), offs3, 2, &at_s, 1, none.get(), 0, two.get());
    expect(st == TGX_ERR_INVALID, "index = S", 0, st);
    st = tgx_select_host(ids.get(), offs3, 2, &big, 1, none.get(), 0, two.get());
    expect(st == TGX_ERR_INVALID, "index 2^62", 0, st);
    const uint64_t z = 0;
    st = tgx_select_text_host(nullptr, &z, 0, &zero, 1, nullptr, 0, two.get());
    expect(st == TGX_ERR_INVALID, "no rows, one index", 0, st);
    const uint64_t bad_offs[3] = {0, 4, 3};
    st = tgx_select_host(ids.get(), bad_offs, 2, &zero, 1, none.get(), 0, two.get());
    expect(st == TGX_ERR_INVALID, "offsets that decrease", 0, st);
    // the permutation: exactly n indices, each once, ordered by (key, index)
    for (uint64_t n : {0ull, 1ull, 2ull, 255ull, 256ull, 257ull, 1025ull, 65537ull}) {
        for (uint64_t seed : {0ull, ~0ull, 0x1234567ull}) {
            std::unique_ptr<int64_t[]> rows = block<int64_t>(n);
            st = tgx_shuffled_rows_host(n, seed, rows.get());
            expect(st == TGX_OK, "shuffled rows", n, st);
            std::vector<uint8_t> seen(n, 0);
            bool ok = true;
            for (uint64_t k = 0; k < n && ok; k++) {
                ok = rows[k] >= 0 && (uint64_t)rows[k] < n && !seen[(size_t)rows[k]];
                if (ok) seen[(size_t)rows[k]] = 1;
                if (ok && k) {
                    const uint64_t a = tgx_shuffle_key(seed, (uint64_t)rows[k - 1]), b = tgx_shuffle_key(seed, (uint64_t)rows[k]);
                    ok = a < b || (a == b && rows[k - 1] < rows[k]);
                }
            }
            expect(ok, "a permutation in key order", n, seed);
            n_runs++;
        }
    }
    st = tgx_shuffled_rows_host(1ull << 31, 0, nullptr);
    expect(st == TGX_ERR_UNSUPPORTED, "2^31 rows", 0, st);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("select twin: ok (%d runs)\n", n_runs);
    return 0;
}
