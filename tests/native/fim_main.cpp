// Stand-alone driver of the fill-in-the-middle twin (include/tgx.h: tgx_fim_host) for a sanitizer build:
// tests/test_fim_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No device
// is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx.h documents (T ids and S + 1 offsets
// in; T' ids, S + 1 offsets, S modes and 2S cuts out), so that reading or writing one element too many is a report.  T' is
// taken from a first call whose destination is too small, which must be refused before anything is written.  The shapes
// put the end of the output one to three positions on either side of a tile of 1024, with empty rows at the start, in
// the middle and at the end, and a row that owns whole tiles.
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

constexpr uint32_t kV = 500, kPre = kV + 2, kSuf = kV, kMid = kV + 1;

void run(uint64_t run_id, const std::vector<uint64_t>& sizes, double rate, double spm_rate, uint64_t seed, uint64_t first_row) {
    std::vector<uint64_t> offs(1, 0);
    for (uint64_t n : sizes) offs.push_back(offs.back() + n);
    const uint64_t S = sizes.size(), T = offs.back();
    std::vector<uint32_t> ids(T);
    for (uint64_t j = 0; j < T; j++) ids[j] = (uint32_t)((j * 2654435761u >> 7) % kV);
    const std::unique_ptr<uint32_t[]> b_ids = block_of(ids);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);

    // T' from the rule itself: a row is rearranged iff it has a token and its first uniform is below the rate
    uint64_t want_applied = 0;
    for (uint64_t i = 0; i < S; i++) want_applied += sizes[i] >= 1 && tgx_fim_u01(seed, first_row + i, 0) < rate;
    const uint64_t T2 = T + 3 * want_applied;

    std::unique_ptr<uint64_t[]> out_offs = block<uint64_t>(S + 1);
    std::unique_ptr<uint8_t[]> mode = block<uint8_t>(S);
    std::unique_ptr<uint64_t[]> cuts = block<uint64_t>(2 * S);
    uint64_t n_applied = ~0ull;
    tgx_status st;
    if (T2 > 0) {  // one id short: refused, and the (empty) destination is not touched
        std::unique_ptr<uint32_t[]> small = block<uint32_t>(T2 - 1);
        st = tgx_fim_host(b_ids.get(), b_offs.get(), S, kV, kPre, kSuf, kMid, rate, spm_rate, seed, first_row, small.get(), T2 - 1, out_offs.get(),
                          mode.get(), cuts.get(), &n_applied);
        expect(st == TGX_ERR_INVALID, "a destination one id short", run_id, st);
    }
    std::unique_ptr<uint32_t[]> out = block<uint32_t>(T2);
    st = tgx_fim_host(b_ids.get(), b_offs.get(), S, kV, kPre, kSuf, kMid, rate, spm_rate, seed, first_row, out.get(), T2, out_offs.get(), mode.get(),
                      cuts.get(), &n_applied);
    expect(st == TGX_OK, "fim", run_id, st);
    if (st != TGX_OK) return;
    expect(n_applied == want_applied && out_offs[0] == 0 && out_offs[S] == T2, "totals", run_id, n_applied, out_offs[S]);
    for (uint64_t i = 0; i < S; i++) {
        const uint64_t n = sizes[i], o = out_offs[i], len = out_offs[i + 1] - o, a = cuts[2 * i], b = cuts[2 * i + 1];
        const uint32_t* src = ids.data() + offs[i];
        if (mode[i] == 0) {
            expect(len == n && a == 0 && b == 0 && (n == 0 || memcmp(out.get() + o, src, n * 4) == 0), "a copied row", run_id, i);
            continue;
        }
        expect(mode[i] <= 2 && len == n + 3 && a <= b && b <= n, "a rearranged row's shape", run_id, i, len);
        if (len != n + 3 || b > n || a > b) continue;
        // the pieces, wherever the mode puts them
        const uint32_t* row = out.get() + o;
        const uint64_t ns = n - b;
        bool ok = row[0] == kPre;
        if (mode[i] == 1) {
            ok = ok && row[a + 1] == kSuf && row[a + 2 + ns] == kMid;
            ok = ok && (a == 0 || memcmp(row + 1, src, a * 4) == 0) && (ns == 0 || memcmp(row + a + 2, src + b, ns * 4) == 0) &&
                 (b == a || memcmp(row + a + 3 + ns, src + a, (b - a) * 4) == 0);
        } else {
            ok = ok && row[1] == kSuf && row[2 + ns] == kMid;
            ok = ok && (ns == 0 || memcmp(row + 2, src + b, ns * 4) == 0) && (b == 0 || memcmp(row + 3 + ns, src, b * 4) == 0);
        }
        expect(ok, "a rearranged row's pieces", run_id, i, mode[i]);
    }
    // the optional outputs left out
    st = tgx_fim_host(b_ids.get(), b_offs.get(), S, kV, kPre, kSuf, kMid, rate, spm_rate, seed, first_row, out.get(), T2, out_offs.get(), nullptr,
                      nullptr, nullptr);
    expect(st == TGX_OK && out_offs[S] == T2, "fim, ids and offsets alone", run_id, st);
}

}  // namespace

int main() {
    int n_runs = 0;
    static const double rates[3] = {0.0, 0.5, 1.0};
    for (uint64_t k = 0; k < 63; k++) {
        const double rate = rates[k % 3], spm_rate = rates[(k / 3) % 3];
        const uint64_t seed = k < 2 ? (k ? ~0ull : 0ull) : k * 0x9E3779B97F4A7C15ULL, first_row = k % 4 == 3 ? ~0ull - 1 : k;
        // rows around one and four tiles, empty rows at both ends and in the middle; the last non-empty row is sized so
        // that the input ends 1024·m + d, d = -3 .. 3 (the output ends there too when nothing is rearranged, and three
        // per rearranged row further on otherwise: every residue of 4 occurs)
        std::vector<uint64_t> sizes = {0, 0, 1 + k % 3, 1019 + k % 11, 0, 0, 0, 4093 + k % 8, 3};
        uint64_t T = 0;
        for (uint64_t n : sizes) T += n;
        const int64_t d = (int64_t)(k % 7) - 3;
        const uint64_t target = (T + 1 + 3 + 1023) / 1024 * 1024 + (uint64_t)d;
        sizes.push_back(target - T);
        sizes.push_back(0);
        if (k % 2) sizes.push_back(0);
        run(k, sizes, rate, spm_rate, seed, first_row);
        n_runs++;
    }
    run(100, {0, 5, 70000, 0, 1026}, 1.0, 0.5, 99, 3);  // a row that owns about 69 tiles
    run(101, {7}, 1.0, 1.0, 1, 0);
    run(102, {0}, 1.0, 1.0, 1, 0);
    run(103, {0, 0, 0}, 1.0, 0.0, 1, 0);
    n_runs += 4;
    // no rows, and arguments that are refused before anything is touched
    const uint64_t zero = 0;
    std::unique_ptr<uint32_t[]> none = block<uint32_t>(0);
    std::unique_ptr<uint64_t[]> one = block<uint64_t>(1);
    uint64_t n_applied = 7;
    tgx_status st = tgx_fim_host(nullptr, &zero, 0, kV, kPre, kSuf, kMid, 1.0, 0.5, 0, 0, none.get(), 0, one.get(), nullptr, nullptr, &n_applied);
    expect(st == TGX_OK && one[0] == 0 && n_applied == 0, "no rows", 0, st, n_applied);
    st = tgx_fim_host(nullptr, &zero, 0, kV, kPre, kSuf, kMid, 1.0, 0.5, 0, 0, nullptr, 0, one.get(), nullptr, nullptr, nullptr);
    expect(st == TGX_OK, "no rows, no destination", 0, st);
    st = tgx_fim_host(nullptr, &zero, 0, kV, kPre, kPre, kMid, 1.0, 0.5, 0, 0, none.get(), 0, one.get(), nullptr, nullptr, nullptr);
    expect(st == TGX_ERR_INVALID, "equal sentinels", 0, st);
    st = tgx_fim_host(nullptr, &zero, 0, kV, kPre, kSuf, TGX_NO_ID, 1.0, 0.5, 0, 0, none.get(), 0, one.get(), nullptr, nullptr, nullptr);
    expect(st == TGX_ERR_INVALID, "a sentinel that is TGX_NO_ID", 0, st);
    st = tgx_fim_host(nullptr, &zero, 0, kV, kPre, kSuf, kMid, 1.5, 0.5, 0, 0, none.get(), 0, one.get(), nullptr, nullptr, nullptr);
    expect(st == TGX_ERR_INVALID, "rate above 1", 0, st);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("fim twin: ok (%d runs)\n", n_runs);
    return 0;
}
