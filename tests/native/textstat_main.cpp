// Stand-alone driver of the text-statistics twins (include/tgx.h: tgx_text_stats_host, tgx_lines_host) for a sanitizer
// build: tests/test_textstat_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs
// it.  No device is opened.
//
// Every buffer handed to a twin is a heap block of exactly the size include/tgx.h documents (N text bytes, S + 1 offsets,
// 11 * S statistics, N line-start bytes, n_lines + 1 offsets out), so that reading or writing one element too many is a
// report: the byte before a chunk is read only where there is one, and the last row's last byte is the block's last.
// The shapes are the edge shapes of tests/textstat_cases.py: rows of 0 .. 3 bytes, rows that end one to three bytes on
// either side of a chunk of 64 bytes, of a tile of 256 and of two tiles, runs of empty rows, a line of five tiles with
// and without its '\n', a row of only '\n', a row of every byte value.  Every answer is checked against the definitions
// written out plainly: one pass per row that keeps the open line's length.
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

// mode 0: bytes drawn from (i, t) with a '\n' about every nl_every bytes (0: none) and two- and three-byte characters;
// mode 1: only '\n'; mode 2: the byte values 0, 1, 2, ... in turn
struct Row {
    uint64_t len;
    uint32_t mode, nl_every;
    bool nl_last;  // the row's last byte is a '\n'
};

void run(uint64_t run_id, const std::vector<Row>& rows_in, uint64_t limit, uint32_t flags) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<uint8_t> text;
    for (uint64_t i = 0; i < rows_in.size(); i++) {
        const Row& r = rows_in[i];
        for (uint64_t t = 0; t < r.len; t++) {
            const uint64_t h = (t + 1) * 2654435761u + i * 40503u;
            uint8_t b = (uint8_t)(32 + h % 90);
            if (r.mode == 0 && h % 11 == 0) b = (uint8_t)(0xC3 + h % 40);       // a lead byte ...
            if (r.mode == 0 && h % 11 == 1) b = (uint8_t)(0x80 + h % 64);       // ... and continuation bytes, wherever they fall
            if (r.mode == 0 && r.nl_every && h % r.nl_every == 0) b = '\n';
            if (r.mode == 1) b = '\n';
            if (r.mode == 2) b = (uint8_t)t;
            if (r.nl_last && t + 1 == r.len) b = '\n';
            text.push_back(b);
        }
        offs.push_back(text.size());
    }
    const uint64_t S = rows_in.size(), N = text.size();
    const bool chars = (flags & TGX_TEXTSTAT_CHARS) != 0;
    // the definitions, plainly
    std::vector<int64_t> want((size_t)TGX_TEXTSTAT_N * S, 0);
    std::vector<uint8_t> want_marks(N, 0);
    std::vector<uint64_t> want_offs;
    for (uint64_t i = 0; i < S; i++) {
        auto stat = [&](int k) -> int64_t& { return want[(size_t)k * S + i]; };
        uint64_t open = 0;
        bool at_start = true;
        for (uint64_t p = offs[i]; p < offs[i + 1]; p++) {
            const uint8_t b = text[p];
            const bool is_char = (b & 0xC0) != 0x80, is_space = b == 0x20 || (b >= 0x09 && b <= 0x0D);
            if (at_start) {
                want_marks[p] = 1;
                want_offs.push_back(p);
                open = 0;
                at_start = false;
            }
            stat(0)++;
            stat(1) += is_char;
            stat(6) += (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z');
            stat(7) += b >= '0' && b <= '9';
            stat(8) += is_space;
            stat(9) += b >= 0xC0;
            stat(10) += (b < 0x20 && !is_space) || b == 0x7F;
            if (b != '\n') open += chars ? is_char : 1;
            if (b == '\n' || p + 1 == offs[i + 1]) {
                stat(2) += b == '\n';
                stat(3)++;
                stat(4) = std::max<int64_t>(stat(4), (int64_t)open);
                stat(5) += open > limit;
                at_start = true;
            }
        }
    }
    want_offs.push_back(N);
    const std::unique_ptr<uint8_t[]> b_text = block_of(text);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs);
    std::unique_ptr<int64_t[]> stats = block<int64_t>((size_t)TGX_TEXTSTAT_N * S), stats_only = block<int64_t>((size_t)TGX_TEXTSTAT_N * S);
    std::unique_ptr<uint8_t[]> marks = block<uint8_t>(N), marks_only = block<uint8_t>(N);
    expect(tgx_text_stats_host(b_text.get(), b_offs.get(), S, limit, flags, stats.get(), marks.get()) == TGX_OK, "stats status", run_id);
    expect(tgx_text_stats_host(b_text.get(), b_offs.get(), S, limit, flags, stats_only.get(), nullptr) == TGX_OK, "stats-only status", run_id);
    expect(tgx_text_stats_host(b_text.get(), b_offs.get(), S, limit, flags, nullptr, marks_only.get()) == TGX_OK, "marks-only status", run_id);
    for (uint64_t k = 0; k < (uint64_t)TGX_TEXTSTAT_N * S; k++)
        expect(stats[k] == want[k] && stats_only[k] == want[k], "statistic", run_id, k / S, k % S);
    for (uint64_t p = 0; p < N; p++) expect(marks[p] == want_marks[p] && marks_only[p] == want_marks[p], "line start", run_id, p);
    uint64_t n_lines = ~0ull;
    std::unique_ptr<uint64_t[]> out_offs = block<uint64_t>(want_offs.size());
    expect(tgx_lines_host(b_text.get(), b_offs.get(), S, out_offs.get(), want_offs.size(), &n_lines) == TGX_OK && n_lines + 1 == want_offs.size(), "lines status",
           run_id, n_lines);
    if (n_lines + 1 == want_offs.size())
        for (uint64_t k = 0; k <= n_lines; k++) expect(out_offs[k] == want_offs[k], "line offset", run_id, k);
    expect(tgx_lines_host(b_text.get(), b_offs.get(), S, out_offs.get(), want_offs.size() - 1, &n_lines) == TGX_ERR_INVALID, "too little room", run_id);
}

void run_both(uint64_t id, const std::vector<Row>& rows) {
    run(id, rows, 0, 0);
    run(id + 1, rows, 5, TGX_TEXTSTAT_CHARS);
    run(id + 2, rows, 5, 0);
    run(id + 3, rows, 0, TGX_TEXTSTAT_CHARS);
}

}  // namespace

int main() {
    uint64_t id = 100;
    {  // rows of 0 .. 3 bytes between runs of empty rows, with and without a '\n' at the end
        std::vector<Row> rows = {{0, 0, 0, false}, {0, 0, 0, false}};
        for (uint64_t n = 1; n <= 3; n++) {
            rows.push_back({n, 0, 2, false});
            rows.push_back({n, 0, 0, true});
            rows.push_back({n, 1, 0, false});
            rows.push_back({0, 0, 0, false});
        }
        rows.push_back({0, 0, 0, false});
        run_both(id, rows);
        id += 10;
    }
    for (uint64_t edge : {64, 256, 512}) {  // rows that end d bytes from an edge, few '\n's: lines astride the edges
        std::vector<Row> rows;
        uint64_t cum = 0;
        for (int d = -3; d <= 3; d++) {
            for (uint64_t n : {0, 2, 5}) {
                rows.push_back({n, 0, 3, false});
                cum += n;
            }
            const uint64_t target = (cum / edge + 2) * edge + d;
            rows.push_back({target - cum, 0, 97, d == 0 || d == 2});
            cum = target;
        }
        rows.push_back({3, 0, 0, false});
        run_both(id, rows);
        id += 10;
    }
    run_both(id, {{2, 0, 0, true}, {5 * 256, 0, 0, false}, {0, 0, 0, false}, {5 * 256, 0, 0, true}, {126, 0, 0, false}, {200, 0, 0, false}});  // long lines
    id += 10;
    run_both(id, {{200, 1, 0, false}, {64, 1, 0, false}, {0, 0, 0, false}, {56, 1, 0, false}, {1, 0, 0, false}, {3, 1, 0, false}});  // only '\n'
    id += 10;
    run_both(id, {{256, 2, 0, false}, {300, 2, 0, false}, {700, 0, 7, false}});  // every byte value
    id += 10;
    run_both(id, {});
    run_both(id + 5, {{0, 0, 0, false}, {0, 0, 0, false}});
    {  // refused: offsets that do not start at 0 or descend, no text, an unknown flag, no output
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 3};
        const uint8_t d[3] = {'a', '\n', 'b'};
        int64_t stats[2 * TGX_TEXTSTAT_N];
        std::fill(stats, stats + 2 * TGX_TEXTSTAT_N, -7);
        uint8_t marks[3] = {7, 7, 7};
        uint64_t out_offs[4] = {9, 9, 9, 9}, n_lines = 77;
        expect(tgx_text_stats_host(d, bad0, 2, 5, 0, stats, marks) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_text_stats_host(d, bad1, 2, 5, 0, stats, marks) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_text_stats_host(nullptr, good, 2, 5, 0, stats, marks) == TGX_ERR_INVALID, "text NULL", 0);
        expect(tgx_text_stats_host(d, good, 2, 5, 2, stats, marks) == TGX_ERR_INVALID, "unknown flag", 0);
        expect(tgx_text_stats_host(d, good, 2, 5, 0, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
        expect(tgx_lines_host(d, bad1, 2, out_offs, 4, &n_lines) == TGX_ERR_INVALID, "lines descending", 0);
        expect(tgx_lines_host(d, good, 2, out_offs, 4, nullptr) == TGX_ERR_INVALID, "n_lines NULL", 0);
        expect(tgx_lines_host(d, good, 2, out_offs, 3, &n_lines) == TGX_ERR_INVALID && n_lines == 3, "room", 0, n_lines);
        bool untouched = marks[0] == 7 && marks[1] == 7 && marks[2] == 7 && out_offs[0] == 9 && out_offs[3] == 9;
        for (int k = 0; k < 2 * TGX_TEXTSTAT_N; k++) untouched = untouched && stats[k] == -7;
        expect(untouched, "a refused call writes nothing", 0);
        expect(tgx_lines_host(d, good, 2, out_offs, 4, &n_lines) == TGX_OK && n_lines == 3 && out_offs[1] == 1 && out_offs[2] == 2 && out_offs[3] == 3, "three lines", 0);
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("textstat twin: ok\n");
    return 0;
}
