// Stand-alone driver of the five *_host twins (include/tgx.h) for a sanitizer build: tests/test_host_twins_native.py
// compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents, so that reading or
// writing one element too many is a report.  The shapes are the smallest that reach every boundary of the twins'
// index arithmetic: groups of 4 elements / 16 raw bytes, tiles of 1024 elements / 4096 raw bytes.
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

uint32_t g_rng = 12345u;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

int g_failed = 0;
void expect(bool ok, const char* what, uint64_t total, int shape, uint64_t a = 0, uint64_t b = 0) {
    if (ok) return;
    g_failed++;
    fprintf(stderr, "FAILED %s (total %llu, shape %d, %llu, %llu)\n", what, (unsigned long long)total, shape, (unsigned long long)a,
            (unsigned long long)b);
}

// ---- the vocabulary: 40 tokens of 1..20 bytes (some longer than a 16-byte slot); every fifth is not valid UTF-8 -------
constexpr uint32_t kV = 40, kSpecials = 3;
struct Vocab {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offs;
    std::vector<uint8_t> sp_bytes;
    std::vector<uint64_t> sp_offs;
};
Vocab make_vocab() {
    Vocab v;
    v.offs.push_back(0);
    for (uint32_t i = 0; i < kV; i++) {
        const uint32_t n = 1 + (i * 7) % 20;
        for (uint32_t k = 0; k < n; k++) {
            uint8_t c = (uint8_t)('a' + (i + k) % 26);
            if (i % 5 == 4) {  // stray continuation bytes, a lead without its tail, bytes that never occur
                static const uint8_t bad[4] = {0x80, 0xE4, 0xFF, 0xBF};
                if (k % 3 != 1) c = bad[(i + k) % 4];
            } else if (i % 5 == 1 && n >= 3 && k < 3) {  // a CJK character
                static const uint8_t cjk[3] = {0xE4, 0xB8, 0xAD};
                c = cjk[k];
            }
            v.bytes.push_back(c);
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

// ---- rows: `total` ids as one row (0), as many rows of 0..3 ids (1), as mixed rows (2) -----------------------------------
std::vector<uint64_t> make_offs(uint64_t total, int shape) {
    std::vector<uint64_t> offs(1, 0);
    if (shape == 0) {
        offs.push_back(total);
        return offs;
    }
    static const uint64_t mixed[8] = {0, 1, 5, 300, 2, 1500, 0, 64};
    uint64_t at = 0;
    for (uint64_t i = 0; at < total || i < 3; i++) {
        uint64_t n = shape == 1 ? rnd() % 4 : mixed[i % 8];
        if (n > total - at) n = total - at;
        at += n;
        offs.push_back(at);
    }
    offs.push_back(at);  // an empty last row
    return offs;
}

constexpr uint32_t kBos = kV, kPadId = kV + 1, kEos = kV + 2;  // the three special tokens' ids

struct Case {
    uint64_t total;
    int shape;
    uint64_t n_rows;
    std::unique_ptr<uint32_t[]> ids;   // u32[total], base and special ids
    std::unique_ptr<uint64_t[]> offs;  // u64[n_rows + 1]
};

// ---- layouts, and decode / spans of the padded form over what the padded layout wrote ---------------------------------
void run_layouts(const Case& c, const uint8_t* vb, const uint64_t* vo, const uint8_t* sb, const uint64_t* so) {
    const uint64_t S = c.n_rows;
    static const uint32_t row_lens[4] = {1, 3, 7, 64};
    for (uint32_t L : row_lens)
        for (uint32_t flags = 0; flags < 8; flags++) {  // PAD_LEFT, TRUNC_LEFT, I64
            const bool i64 = (flags & TGX_LAYOUT_I64) != 0;
            const uint32_t bos = L >= 3 ? kBos : TGX_NO_ID, eos = L >= 2 ? kEos : TGX_NO_ID;
            const uint64_t A = (bos != TGX_NO_ID) + (eos != TGX_NO_ID);
            std::unique_ptr<uint8_t[]> out = block<uint8_t>(S * L * (i64 ? 8 : 4));
            std::unique_ptr<uint8_t[]> mask = block<uint8_t>(S * L);
            std::unique_ptr<int32_t[]> lengths = block<int32_t>(S);
            uint64_t n_trunc = ~0ull;
            tgx_status st = tgx_layout_pad_host(c.ids.get(), c.offs.get(), S, L, kPadId, bos, eos, flags, out.get(), mask.get(), lengths.get(), &n_trunc);
            expect(st == TGX_OK, "tgx_layout_pad_host", c.total, c.shape, L, flags);
            if (st != TGX_OK) continue;
            uint64_t want_trunc = 0, live = 0, want_live = 0;
            for (uint64_t i = 0; i < S; i++) {
                const uint64_t n = c.offs[i + 1] - c.offs[i], keep = n < L - A ? n : L - A;
                want_trunc += n > L - A;
                want_live += keep + A;
                expect((uint64_t)lengths[i] == keep + A, "pad lengths", c.total, c.shape, L, i);
            }
            for (uint64_t e = 0; e < S * L; e++) live += mask[e];
            expect(n_trunc == want_trunc && live == want_live, "pad mask / truncated", c.total, c.shape, L, flags);

            // the padded form of decode: the live elements by lengths (right padding), by mask, or by the pad id
            for (int how = 0; how < 3; how++) {
                if (how == 0 && (flags & TGX_LAYOUT_PAD_LEFT)) continue;
                uint8_t* text = nullptr;
                std::unique_ptr<uint64_t[]> toffs = block<uint64_t>(S + 1);
                uint64_t n_rep = 0, bad_s = 0, bad_id = 0;
                st = tgx_decode_rows_host(vb, vo, kV, sb, so, kSpecials, out.get(), i64 ? 2 : 1, nullptr, S, L, how == 1 ? mask.get() : nullptr,
                                          how == 0 ? lengths.get() : nullptr, how == 2 ? kPadId : TGX_NO_ID, how & 1, &text, toffs.get(), &n_rep,
                                          &bad_s, &bad_id);
                expect(st == TGX_OK && text != nullptr, "tgx_decode_rows_host (padded)", c.total, c.shape, L, flags);
                free(text);
            }
            // the padded form of the spans
            for (uint32_t chars = 0; chars < 2; chars++) {
                const uint32_t sf = flags | (chars ? TGX_SPAN_CHARS : 0u);
                std::unique_ptr<uint8_t[]> spans = block<uint8_t>(S * L * 2 * (i64 ? 8 : 4));
                st = tgx_spans_host(vb, vo, kV, sb, so, kSpecials, c.ids.get(), c.offs.get(), S, L, bos, eos, sf, spans.get());
                expect(st == TGX_OK, "tgx_spans_host (padded)", c.total, c.shape, L, sf);
            }
        }

    static const uint32_t block_lens[4] = {1, 5, 1024, 1500};
    for (uint32_t B : block_lens)
        for (uint32_t variant = 0; variant < 4; variant++) {  // I64, bos / eos
            const uint32_t flags = (variant & 1) ? TGX_LAYOUT_I64 : 0u;
            const uint32_t bos = (variant & 2) ? kBos : TGX_NO_ID, eos = (variant & 2) ? kEos : TGX_NO_ID;
            const uint64_t n_stream = c.total + S * ((variant & 2) ? 2 : 0), nb = (n_stream + B - 1) / B;
            std::unique_ptr<uint8_t[]> out = block<uint8_t>(nb * B * (flags ? 8 : 4));
            std::unique_ptr<int32_t[]> doc = block<int32_t>(nb * B), pos = block<int32_t>(nb * B);
            uint64_t n_blocks = ~0ull;
            const tgx_status st = tgx_layout_pack_host(c.ids.get(), c.offs.get(), S, B, kPadId, bos, eos, flags, out.get(), doc.get(), pos.get(), &n_blocks);
            expect(st == TGX_OK && n_blocks == nb, "tgx_layout_pack_host", c.total, c.shape, B, variant);
            if (st == TGX_OK && nb) expect(n_stream == 0 || (doc[0] >= 0 && pos[0] == 0), "pack doc / pos", c.total, c.shape, B, variant);
        }
}

// ---- decode and spans of the offsets form -------------------------------------------------------------------------------
void run_flat(const Case& c, const uint8_t* vb, const uint64_t* vo, const uint8_t* sb, const uint64_t* so) {
    const uint64_t S = c.n_rows;
    for (int include_special = 0; include_special < 2; include_special++) {
        uint8_t* text = nullptr;
        std::unique_ptr<uint64_t[]> toffs = block<uint64_t>(S + 1);
        uint64_t n_rep = 0, bad_s = 0, bad_id = 0;
        const tgx_status st = tgx_decode_rows_host(vb, vo, kV, sb, so, kSpecials, c.ids.get(), 0, c.offs.get(), S, 0, nullptr, nullptr, TGX_NO_ID,
                                                   include_special, &text, toffs.get(), &n_rep, &bad_s, &bad_id);
        expect(st == TGX_OK && text != nullptr, "tgx_decode_rows_host (offsets)", c.total, c.shape, include_special);
        if (st == TGX_OK) {
            expect(toffs[0] == 0, "decode offsets", c.total, c.shape);
            for (uint64_t i = 0; i < S; i++) expect(toffs[i] <= toffs[i + 1], "decode offsets ascend", c.total, c.shape, i);
            expect(c.total < 40 || n_rep > 0, "decode replaces", c.total, c.shape);  // (the second copy ran)
        }
        free(text);
    }
    for (uint32_t variant = 0; variant < 4; variant++) {
        const uint32_t flags = ((variant & 1) ? TGX_LAYOUT_I64 : 0u) | ((variant & 2) ? TGX_SPAN_CHARS : 0u);
        std::unique_ptr<uint8_t[]> spans = block<uint8_t>(c.total * 2 * ((variant & 1) ? 8 : 4));
        const tgx_status st = tgx_spans_host(vb, vo, kV, sb, so, kSpecials, c.ids.get(), c.offs.get(), S, 0, TGX_NO_ID, TGX_NO_ID, flags, spans.get());
        expect(st == TGX_OK, "tgx_spans_host (flat)", c.total, c.shape, flags);
    }
}

// ---- assembly: the case's rows are the encoded segments; special segments before, between and after them ----------------
void run_assemble(const Case& c) {
    const uint64_t E = c.n_rows;
    std::vector<int32_t> special;
    std::vector<uint64_t> seg_offs(1, 0);
    uint64_t e = 0;
    while (e < E) {
        const uint32_t n_enc = rnd() % 3;  // encoded segments of this sample (0: a sample of special tokens, or of nothing)
        if (rnd() % 2) special.push_back((int32_t)(rnd() % kSpecials));  // before
        for (uint32_t k = 0; k < n_enc && e < E; k++, e++) {
            special.push_back(-1 - (int32_t)(rnd() % 3));
            if (k + 1 < n_enc && rnd() % 2) special.push_back((int32_t)(rnd() % kSpecials));  // between
        }
        if (rnd() % 2) special.push_back((int32_t)(rnd() % kSpecials));  // after
        seg_offs.push_back(special.size());
    }
    seg_offs.push_back(special.size());  // a sample without segments
    const uint64_t S = seg_offs.size() - 1, K = special.size(), n_out = c.total + (K - E);
    std::unique_ptr<uint64_t[]> so = block_of(seg_offs);
    std::unique_ptr<int32_t[]> sp = block_of(special);
    std::unique_ptr<uint32_t[]> out = block<uint32_t>(n_out);
    std::unique_ptr<uint64_t[]> out_offs = block<uint64_t>(S + 1);
    const tgx_status st = tgx_assemble_host(c.ids.get(), c.offs.get(), E, so.get(), sp.get(), S, kV + kSpecials, kSpecials, out.get(), n_out, out_offs.get());
    expect(st == TGX_OK, "tgx_assemble_host", c.total, c.shape, K);
    if (st == TGX_OK) expect(out_offs[0] == 0 && out_offs[S] == n_out, "assemble offsets", c.total, c.shape, K);
}

// special tokens only: no encoded segment, ids and id_offs NULL
void run_assemble_specials_only() {
    const std::vector<uint64_t> seg_offs = {0, 2, 2, 5};
    const std::vector<int32_t> special = {0, 2, 1, 1, 0};
    std::unique_ptr<uint64_t[]> so = block_of(seg_offs);
    std::unique_ptr<int32_t[]> sp = block_of(special);
    std::unique_ptr<uint32_t[]> out = block<uint32_t>(5);
    std::unique_ptr<uint64_t[]> out_offs = block<uint64_t>(4);
    const tgx_status st = tgx_assemble_host(nullptr, nullptr, 0, so.get(), sp.get(), 3, kV, kSpecials, out.get(), 5, out_offs.get());
    expect(st == TGX_OK && out_offs[3] == 5 && out[1] == kV + 2, "tgx_assemble_host (special tokens only)", 0, 0);
}

}  // namespace

int main() {
    const Vocab v = make_vocab();
    std::unique_ptr<uint8_t[]> vb = block_of(v.bytes), sb = block_of(v.sp_bytes);
    std::unique_ptr<uint64_t[]> vo = block_of(v.offs), so = block_of(v.sp_offs);
    static const uint64_t totals[11] = {0, 1, 3, 4, 5, 1023, 1024, 1025, 2049, 4100, 9000};
    for (uint64_t total : totals)
        for (int shape = 0; shape < 3; shape++) {
            const std::vector<uint64_t> offs = make_offs(total, shape);
            Case c;
            c.total = total;
            c.shape = shape;
            c.n_rows = offs.size() - 1;
            c.offs = block_of(offs);
            c.ids = block<uint32_t>(total);
            for (uint64_t j = 0; j < total; j++) c.ids[j] = rnd() % 16 == 0 ? kV + rnd() % kSpecials : rnd() % kV;
            run_layouts(c, vb.get(), vo.get(), sb.get(), so.get());
            run_flat(c, vb.get(), vo.get(), sb.get(), so.get());
            run_assemble(c);
        }
    run_assemble_specials_only();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("host twins: ok\n");
    return 0;
}
