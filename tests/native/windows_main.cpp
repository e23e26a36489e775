// Stand-alone driver of the two window twins (include/tgx.h: tgx_layout_windows_host, tgx_window_spans_host) for a
// sanitizer build: tests/test_windows_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined
// and runs it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents (W·L ids and mask bytes,
// W lengths / rows / first indices, W·L·2 span elements), so that reading or writing one element too many is a report.
// The shapes are those at which the window count or a window's length changes, with a row long enough to own whole
// tiles of 1024 elements, and empty rows at the start, in the middle and at the end.
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
void expect(bool ok, const char* what, uint32_t L, uint32_t stride, uint32_t flags, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (L %u, stride %u, flags %u, %llu, %llu)\n", what, L, stride, flags, (unsigned long long)a, (unsigned long long)b);
}

// 40 tokens of 1..20 bytes, every fifth with bytes that are not UTF-8, and three special tokens
constexpr uint32_t kV = 40, kSpecials = 3;
constexpr uint32_t kBos = kV, kPadId = kV + 1, kEos = kV + 2;
struct Vocab {
    std::vector<uint8_t> bytes, sp_bytes;
    std::vector<uint64_t> offs, sp_offs;
};
Vocab make_vocab() {
    Vocab v;
    v.offs.push_back(0);
    for (uint32_t i = 0; i < kV; i++) {
        const uint32_t n = 1 + (i * 7) % 20;
        for (uint32_t k = 0; k < n; k++) {
            static const uint8_t bad[4] = {0x80, 0xE4, 0xFF, 0xBF};
            v.bytes.push_back(i % 5 == 4 && k % 3 != 1 ? bad[(i + k) % 4] : (uint8_t)('a' + (i + k) % 26));
        }
        v.offs.push_back(v.bytes.size());
    }
    const char* sp[kSpecials] = {"<s>", "\xE2\x96\x81pad", "</s>"};
    v.sp_offs.push_back(0);
    for (uint32_t k = 0; k < kSpecials; k++) {
        v.sp_bytes.insert(v.sp_bytes.end(), sp[k], sp[k] + strlen(sp[k]));
        v.sp_offs.push_back(v.sp_bytes.size());
    }
    return v;
}

void run(const Vocab& v, uint32_t L, uint32_t stride, uint32_t bos, uint32_t eos, uint32_t flags) {
    const uint32_t A = (bos != TGX_NO_ID) + (eos != TGX_NO_ID), room = L - A, step = room - stride;
    const bool i64 = (flags & TGX_LAYOUT_I64) != 0;
    const uint64_t sizes[] = {0, room - 1u, room, room + 1u, 0, (uint64_t)room + step, (uint64_t)room + step + 1, 3001, 2u * room + 3u * step, 0};
    std::vector<uint64_t> offs(1, 0);
    for (uint64_t n : sizes) offs.push_back(offs.back() + n);
    const uint64_t S = offs.size() - 1, T = offs.back();
    std::vector<uint32_t> ids(T);
    for (uint64_t j = 0; j < T; j++) ids[j] = (uint32_t)((j * 2654435761u >> 7) % (kV + kSpecials));
    const std::unique_ptr<uint32_t[]> b_ids = block_of(ids);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    const std::unique_ptr<uint8_t[]> vb = block_of(v.bytes), sb = block_of(v.sp_bytes);
    const std::unique_ptr<uint64_t[]> vo = block_of(v.offs), so = block_of(v.sp_offs);

    // W first, from a call without a destination
    uint64_t W = ~0ull;
    tgx_status st = tgx_layout_windows_host(b_ids.get(), b_offs.get(), S, L, stride, kPadId, bos, eos, flags, 0, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, &W);
    expect(st == TGX_OK, "window count", L, stride, flags, st);
    uint64_t want_w = 0;
    for (uint64_t n : sizes) want_w += n <= room ? 1 : 1 + (n - room + step - 1) / step;
    expect(W == want_w, "W", L, stride, flags, W, want_w);
    if (st != TGX_OK || W != want_w) return;

    const size_t esz = i64 ? 8 : 4;
    std::unique_ptr<uint8_t[]> out = block<uint8_t>(W * L * esz);
    std::unique_ptr<uint8_t[]> mask = block<uint8_t>(W * L);
    std::unique_ptr<int32_t[]> lengths = block<int32_t>(W), row = block<int32_t>(W), first = block<int32_t>(W);
    uint64_t W2 = 0;
    st = tgx_layout_windows_host(b_ids.get(), b_offs.get(), S, L, stride, kPadId, bos, eos, flags, W, out.get(), mask.get(), lengths.get(), row.get(),
                                 first.get(), &W2);
    expect(st == TGX_OK && W2 == W, "windows", L, stride, flags, st, W2);
    // every token of every row is kept at least once, in order: the windows of a row chain from its start to its end
    uint64_t w = 0;
    for (uint64_t i = 0; i < S; i++) {
        const uint64_t n = offs[i + 1] - offs[i];
        uint64_t covered = 0, k = 0;
        for (; w < W && (uint64_t)row[w] == i; w++, k++) {
            const uint64_t keep = (uint64_t)lengths[w] - A;
            const uint64_t f = (flags & TGX_LAYOUT_TRUNC_LEFT) ? n - (uint64_t)first[w] - keep : (uint64_t)first[w];
            expect(f == k * step && f <= covered && keep <= room, "window start", L, stride, flags, w, f);
            covered = f + keep;
            uint64_t on = 0;
            for (uint32_t c = 0; c < L; c++) on += mask[w * L + c];
            expect(on == (uint64_t)lengths[w], "mask", L, stride, flags, w, on);
        }
        expect(covered == n && k >= 1, "coverage", L, stride, flags, i, covered);
    }
    expect(w == W, "window rows", L, stride, flags, w, W);
    // the optional outputs left out
    st = tgx_layout_windows_host(b_ids.get(), b_offs.get(), S, L, stride, kPadId, bos, eos, flags, W, out.get(), nullptr, nullptr, nullptr, nullptr, &W2);
    expect(st == TGX_OK, "windows, ids alone", L, stride, flags, st);
    // a count that is not the caller's: refused
    st = tgx_layout_windows_host(b_ids.get(), b_offs.get(), S, L, stride, kPadId, bos, eos, flags, W + 1, out.get(), mask.get(), lengths.get(), row.get(),
                                 first.get(), &W2);
    expect(st == TGX_ERR_INVALID, "n_windows mismatch", L, stride, flags, st);

    // the spans of the same windows, in both units: a pair is (0, 0) exactly off the kept tokens' columns
    for (uint32_t chars = 0; chars < 2; chars++) {
        const uint32_t sflags = flags | (chars ? TGX_SPAN_CHARS : 0u);
        uint64_t W3 = 0;
        st = tgx_window_spans_host(vb.get(), vo.get(), kV, sb.get(), so.get(), kSpecials, b_ids.get(), b_offs.get(), S, L, stride, bos, eos, sflags, 0,
                                   nullptr, &W3);
        expect(st == TGX_OK && W3 == W, "span window count", L, stride, sflags, st, W3);
        std::unique_ptr<uint8_t[]> spans = block<uint8_t>(W * L * 2 * esz);
        st = tgx_window_spans_host(vb.get(), vo.get(), kV, sb.get(), so.get(), kSpecials, b_ids.get(), b_offs.get(), S, L, stride, bos, eos, sflags, W,
                                   spans.get(), &W3);
        expect(st == TGX_OK, "window spans", L, stride, sflags, st);
        if (!chars)
            for (uint64_t e = 0; e < W * L; e++) {
                int64_t s0, s1;
                if (i64) {
                    s0 = reinterpret_cast<int64_t*>(spans.get())[2 * e];
                    s1 = reinterpret_cast<int64_t*>(spans.get())[2 * e + 1];
                } else {
                    s0 = reinterpret_cast<int32_t*>(spans.get())[2 * e];
                    s1 = reinterpret_cast<int32_t*>(spans.get())[2 * e + 1];
                }
                if (!mask[e]) expect(s0 == 0 && s1 == 0, "span on padding", L, stride, sflags, e);
                expect(s0 >= 0 && s1 > s0 - 1, "span order", L, stride, sflags, e);
            }
        st = tgx_window_spans_host(vb.get(), vo.get(), kV, sb.get(), so.get(), kSpecials, b_ids.get(), b_offs.get(), S, L, stride, bos, eos, sflags,
                                   W - 1, spans.get(), &W3);
        expect(st == TGX_ERR_INVALID, "span n_windows mismatch", L, stride, sflags, st);
    }
}

}  // namespace

int main() {
    const Vocab v = make_vocab();
    static const uint32_t bos_eos[4][2] = {{TGX_NO_ID, TGX_NO_ID}, {kBos, TGX_NO_ID}, {TGX_NO_ID, kEos}, {kBos, kEos}};
    int n_runs = 0;
    for (const auto& be : bos_eos) {
        const uint32_t A = (be[0] != TGX_NO_ID) + (be[1] != TGX_NO_ID);
        const uint32_t row_lens[4] = {A + 1, 5, 8, 13};
        for (uint32_t L : row_lens) {
            const uint32_t room = L - A;
            const uint32_t strides[4] = {0, 1, room / 2, room - 1};
            for (uint32_t si = 0; si < 4; si++) {
                const uint32_t stride = strides[si];
                bool seen = stride >= room;
                for (uint32_t sj = 0; sj < si; sj++) seen = seen || strides[sj] == stride;
                if (seen) continue;
                for (uint32_t flags = 0; flags < 8; flags++) {  // PAD_LEFT, TRUNC_LEFT, I64
                    run(v, L, stride, be[0], be[1], flags);
                    n_runs++;
                }
            }
        }
    }
    // no rows, and arguments that are refused before anything is touched
    uint64_t W = 7;
    const uint64_t zero = 0;
    tgx_status st = tgx_layout_windows_host(nullptr, &zero, 0, 4, 1, kPadId, TGX_NO_ID, TGX_NO_ID, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &W);
    expect(st == TGX_OK && W == 0, "no rows", 4, 1, 0, st, W);
    std::unique_ptr<int32_t[]> none = block<int32_t>(0);
    st = tgx_layout_windows_host(nullptr, &zero, 0, 4, 1, kPadId, TGX_NO_ID, TGX_NO_ID, 0, 0, none.get(), nullptr, nullptr, nullptr, nullptr, &W);
    expect(st == TGX_OK && W == 0, "no rows, a destination", 4, 1, 0, st, W);
    st = tgx_layout_windows_host(nullptr, &zero, 0, 4, 4, kPadId, TGX_NO_ID, TGX_NO_ID, 0, 0, none.get(), nullptr, nullptr, nullptr, nullptr, &W);
    expect(st == TGX_ERR_INVALID, "stride = room", 4, 4, 0, st);
    st = tgx_layout_windows_host(nullptr, &zero, 0, 2, 0, kPadId, kBos, kEos, 0, 0, none.get(), nullptr, nullptr, nullptr, nullptr, &W);
    expect(st == TGX_ERR_INVALID, "no room", 2, 0, 0, st);
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("window twins: ok (%d runs)\n", n_runs);
    return 0;
}
