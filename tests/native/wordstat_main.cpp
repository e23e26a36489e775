// Stand-alone driver of the word-statistics twin (include/tgx_words.h: tgx_word_stats_host) for a sanitizer build:
// tests/test_wordstat_native.py compiles it with csrc/host_twins.cpp under -fsanitize=address,undefined and runs it.  No
// device is opened.
//
// Every buffer handed to the twin is a heap block of exactly the size include/tgx_words.h documents (N text bytes, S + 1
// offsets, 14 * S statistics, N marks, the stop words' bytes and n_stop + 1 offsets), so that reading or writing one element
// too many is a report: the bytes a position looks back on are read only where the row has them, and the byte after a
// row's last is never read.  The shapes are the edge shapes of tests/wordstat_cases.py: rows of 0 .. 3 bytes, rows that
// end one to three bytes on either side of a chunk of 64 bytes, of a tile of 256 and of two tiles, runs of empty rows, a
// word of five tiles, rows of spaces only, a row of every byte value.  Every answer is checked against the definitions
// written out plainly: one pass per row that keeps the open word and the open line.  Then the carry operator of
// csrc/wordstat.h is checked for associativity and its identity over a small state space, exhaustively.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tgx_words.h"
#define TGX_HOST_ONLY
#include "../../tokengeex_amd/csrc/wordstat.h"

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
    if (g_failed < 50) fprintf(stderr, "FAILED %s (run %llu: %llu, %llu)\n", what, (unsigned long long)run, (unsigned long long)a, (unsigned long long)b);
}

bool is_space(uint8_t b) { return b == 0x20 || (b >= 0x09 && b <= 0x0D); }
uint8_t lower(uint8_t b) { return b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b; }

// mode 0: bytes drawn from (i, t): letters of both cases, digits, white space about every sp_every bytes (0: none), dots,
// '#', bullets, two- and three-byte characters, the pieces of U+2026 and U+2022, stop words; mode 1: only spaces and
// '\n'; mode 2: the byte values 0, 1, 2, ... in turn; mode 3: digits only
struct Row {
    uint64_t len;
    uint32_t mode, sp_every;
};

const char* const kPieces[] = {"the", "The", "of", "a", "absolute", "...", "....", "..", "\xE2\x80\xA6", "\xE2\x80\xA2", "-", "*", "#", "\n", "\n- ", "\n  * ",
                               "\n \xE2\x80\xA2 ", "...\n", "\"\n", "?\n", "`", "@", "\xC3\xA9", "\xE2\x82\xAC", "Zq7", "x"};

void run(uint64_t run_id, const std::vector<Row>& rows_in, uint64_t limit, uint32_t flags, const std::vector<std::string>& stops) {
    std::vector<uint64_t> offs(1, 0);
    std::vector<uint8_t> text;
    for (uint64_t i = 0; i < rows_in.size(); i++) {
        const Row& r = rows_in[i];
        const uint64_t begin = text.size();
        for (uint64_t t = 0; text.size() - begin < r.len; t++) {
            const uint64_t h = (t + 1) * 2654435761u + i * 40503u;
            if (r.mode == 0) {
                const char* piece = kPieces[(h >> 7) % (sizeof(kPieces) / sizeof(kPieces[0]))];
                for (const char* q = piece; *q && text.size() - begin < r.len; q++) text.push_back((uint8_t)*q);
                if (r.sp_every && h % r.sp_every == 0 && text.size() - begin < r.len) text.push_back(h % 5 == 0 ? '\t' : ' ');
            } else if (r.mode == 1) {
                text.push_back(h % 7 == 0 ? '\n' : ' ');
            } else if (r.mode == 2) {
                text.push_back((uint8_t)t);
            } else {
                text.push_back((uint8_t)('0' + h % 10));
            }
        }
        offs.push_back(text.size());
    }
    const uint64_t S = rows_in.size(), N = text.size();
    const bool chars = (flags & TGX_WORDSTAT_CHARS) != 0, fold = (flags & TGX_WORDSTAT_FOLD) != 0;
    // the definitions, plainly
    std::vector<int64_t> want((size_t)TGX_WORDSTAT_N * S, 0);
    std::vector<uint8_t> want_marks(N, 0);
    for (uint64_t i = 0; i < S; i++) {
        auto stat = [&](int k) -> int64_t& { return want[(size_t)k * S + i]; };
        const uint64_t begin = offs[i], end = offs[i + 1];
        uint64_t word_start = 0, word_len = 0, line_start = begin, line_nonspace = 0, dots = 0;
        bool in_word = false, word_alpha = false, word_wide = false;
        for (uint64_t p = begin; p < end; p++) {
            const uint8_t b = text[p];
            if (p == begin || text[p - 1] == '\n') {
                line_start = p;
                line_nonspace = 0;
            }
            if (!is_space(b)) {
                if (!in_word) {
                    in_word = true;
                    word_start = p;
                    word_len = 0;
                    word_alpha = word_wide = false;
                    want_marks[p] |= 1;
                }
                word_len += chars ? ((b & 0xC0) != 0x80) : 1;
                word_alpha = word_alpha || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z');
                word_wide = word_wide || b >= 0x80;
                stat(1) += chars ? ((b & 0xC0) != 0x80) : 1;
                const bool bullet = (line_nonspace == 0 && (b == '-' || b == '*')) || (line_nonspace == 2 && b == 0xA2 && text[p - 1] == 0x80 && text[p - 2] == 0xE2);
                if (bullet) {
                    stat(9)++;
                    want_marks[p] |= 8;
                }
                line_nonspace++;
                if (p + 1 == end || is_space(text[p + 1])) {  // the word ends here
                    in_word = false;
                    want_marks[p] |= 2;
                    stat(0)++;
                    stat(2) = std::max<int64_t>(stat(2), (int64_t)word_len);
                    stat(3) += word_len > limit;
                    stat(4) += word_alpha;
                    stat(5) += word_alpha || word_wide;
                    for (size_t k = 0; k < stops.size(); k++) {
                        bool same = stops[k].size() == p + 1 - word_start;
                        for (size_t j = 0; same && j < stops[k].size(); j++) same = (uint8_t)stops[k][j] == (fold ? lower(text[word_start + j]) : text[word_start + j]);
                        if (same) {
                            stat(12)++;
                            stat(13) |= (int64_t)1 << k;
                            want_marks[p] |= 4;
                        }
                    }
                }
            }
            stat(6) += b == '#';
            dots = b == '.' ? dots + 1 : 0;
            stat(7) += dots == 3;
            stat(7) += p >= begin + 2 && b == 0xA6 && text[p - 1] == 0x80 && text[p - 2] == 0xE2;
            if (b == '\n' || p + 1 == end) {
                const uint64_t content_end = b == '\n' ? p : p + 1, n = content_end - line_start;  // the content is [line_start, content_end)
                stat(8)++;
                if (n >= 3) {
                    const uint8_t* q = &text[content_end - 3];
                    stat(10) += (q[0] == '.' && q[1] == '.' && q[2] == '.') || (q[0] == 0xE2 && q[1] == 0x80 && q[2] == 0xA6);
                }
                if (n >= 1) {
                    const uint8_t q = text[content_end - 1];
                    stat(11) += q == '.' || q == '!' || q == '?' || q == '"';
                }
            }
        }
    }
    std::vector<uint8_t> stop_bytes;
    std::vector<uint64_t> stop_offs(1, 0);
    for (const std::string& w : stops) {
        stop_bytes.insert(stop_bytes.end(), w.begin(), w.end());
        stop_offs.push_back(stop_bytes.size());
    }
    const std::unique_ptr<uint8_t[]> b_text = block_of(text), b_stop = block_of(stop_bytes);
    const std::unique_ptr<uint64_t[]> b_offs = block_of(offs), b_stop_offs = block_of(stop_offs);
    const uint32_t n_stop = (uint32_t)stops.size();
    std::unique_ptr<int64_t[]> stats = block<int64_t>((size_t)TGX_WORDSTAT_N * S), stats_only = block<int64_t>((size_t)TGX_WORDSTAT_N * S);
    std::unique_ptr<uint8_t[]> marks = block<uint8_t>(N), marks_only = block<uint8_t>(N);
    auto call = [&](int64_t* st, uint8_t* mk) {
        return tgx_word_stats_host(b_text.get(), b_offs.get(), S, limit, n_stop ? b_stop.get() : nullptr, n_stop ? b_stop_offs.get() : nullptr, n_stop, flags, st, mk);
    };
    expect(call(stats.get(), marks.get()) == TGX_OK, "status", run_id);
    expect(call(stats_only.get(), nullptr) == TGX_OK, "stats-only status", run_id);
    expect(call(nullptr, marks_only.get()) == TGX_OK, "marks-only status", run_id);
    for (uint64_t k = 0; k < (uint64_t)TGX_WORDSTAT_N * S; k++) expect(stats[k] == want[k] && stats_only[k] == want[k], "statistic", run_id, k / S, k % S);
    for (uint64_t p = 0; p < N; p++) expect(marks[p] == want_marks[p] && marks_only[p] == want_marks[p], "mark", run_id, p, marks[p]);
}

void run_all(uint64_t id, const std::vector<Row>& rows) {
    const std::vector<std::string> table = {"a", "the", "`", "absolute", "of"}, with_upper = {"The", "a", "absolute"}, none;
    run(id, rows, 0, 0, none);
    run(id + 1, rows, 5, TGX_WORDSTAT_CHARS | TGX_WORDSTAT_FOLD, table);
    run(id + 2, rows, 5, TGX_WORDSTAT_FOLD, none);
    run(id + 3, rows, 0, TGX_WORDSTAT_CHARS, with_upper);
    run(id + 4, rows, 5, 0, table);
}

// (a after b) after c = a after (b after c), and 0 is the identity, over every state of: units 0, 1, 5; the two flags;
// the word state's reset; nsb 0 .. 3; the line state's reset
void carry_op_is_associative() {
    std::vector<uint64_t> states;
    for (uint64_t units : {0, 1, 5})
        for (uint64_t bits = 0; bits < 16; bits++)
            for (uint64_t nsb = 0; nsb < 4; nsb++)
                states.push_back(units | ((bits & 1) ? tgx::kWordAlpha : 0) | ((bits & 2) ? tgx::kWordWide : 0) | ((bits & 4) ? tgx::kWordReset : 0) |
                                 ((bits & 8) ? tgx::kLineReset : 0) | (nsb << tgx::kLineNsbShift));
    const tgx::WordstatCarryOp op;
    uint64_t bad = 0;
    for (uint64_t a : states) {
        bad += op(0, a) != a || op(a, 0) != a;
        for (uint64_t b : states) {
            const uint64_t ab = op(a, b);
            for (uint64_t c : states) bad += op(ab, c) != op(a, op(b, c));
        }
    }
    expect(bad == 0, "the carry operator is associative with identity 0", 0, bad, states.size());
}

}  // namespace

int main() {
    uint64_t id = 100;
    {  // rows of 0 .. 3 bytes between runs of empty rows
        std::vector<Row> rows = {{0, 0, 0}, {0, 0, 0}};
        for (uint64_t n = 1; n <= 3; n++) {
            rows.push_back({n, 0, 2});
            rows.push_back({n, 1, 0});
            rows.push_back({n, 3, 0});
            rows.push_back({0, 0, 0});
        }
        rows.push_back({0, 0, 0});
        run_all(id, rows);
        id += 10;
    }
    for (uint64_t edge : {64, 256, 512}) {  // rows that end d bytes from an edge, little white space: words astride the edges
        std::vector<Row> rows;
        uint64_t cum = 0;
        for (int d = -3; d <= 3; d++) {
            for (uint64_t n : {0, 2, 5}) {
                rows.push_back({n, 0, 3});
                cum += n;
            }
            const uint64_t target = (cum / edge + 2) * edge + d;
            rows.push_back({target - cum, 0, d % 2 ? 2u : 37u});
            cum = target;
        }
        rows.push_back({3, 0, 0});
        run_all(id, rows);
        id += 10;
    }
    run_all(id, {{2, 0, 0}, {5 * 256, 3, 0}, {0, 0, 0}, {5 * 256, 0, 0}, {126, 0, 4}, {200, 3, 0}});  // words of five tiles
    id += 10;
    run_all(id, {{200, 1, 0}, {64, 1, 0}, {0, 0, 0}, {56, 1, 0}, {1, 0, 0}, {3, 1, 0}});  // only white space
    id += 10;
    run_all(id, {{256, 2, 0}, {300, 2, 0}, {700, 0, 3}});  // every byte value
    id += 10;
    run_all(id, {});
    run_all(id + 5, {{0, 0, 0}, {0, 0, 0}});
    {  // refused: bad offsets, no text, an unknown flag, no output, bad tables; a refused call writes nothing
        const uint64_t bad0[3] = {1, 2, 3}, bad1[3] = {0, 3, 2}, good[3] = {0, 1, 3};
        const uint8_t d[3] = {'a', ' ', 'b'};
        int64_t stats[2 * TGX_WORDSTAT_N];
        std::fill(stats, stats + 2 * TGX_WORDSTAT_N, -7);
        uint8_t marks[3] = {7, 7, 7};
        const uint8_t w[] = "theTheof the";
        const uint64_t ok2[3] = {0, 3, 8}, upper[2] = {3, 6}, empty[3] = {0, 3, 3}, nine[2] = {0, 9}, space[2] = {6, 12}, twice[3] = {0, 3, 3 + 3};
        uint8_t dup[6] = {'t', 'h', 'e', 't', 'h', 'e'};
        expect(tgx_word_stats_host(d, bad0, 2, 5, nullptr, nullptr, 0, 0, stats, marks) == TGX_ERR_INVALID, "offs[0]", 0);
        expect(tgx_word_stats_host(d, bad1, 2, 5, nullptr, nullptr, 0, 0, stats, marks) == TGX_ERR_INVALID, "descending", 0);
        expect(tgx_word_stats_host(nullptr, good, 2, 5, nullptr, nullptr, 0, 0, stats, marks) == TGX_ERR_INVALID, "text NULL", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, nullptr, nullptr, 0, 4, stats, marks) == TGX_ERR_INVALID, "unknown flag", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, nullptr, nullptr, 0, 0, nullptr, nullptr) == TGX_ERR_INVALID, "no output", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, nullptr, 1, 0, stats, marks) == TGX_ERR_INVALID, "stop_offs NULL", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, upper, 1, TGX_WORDSTAT_FOLD, stats, marks) == TGX_ERR_INVALID, "A-Z under the fold", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, empty, 2, 0, stats, marks) == TGX_ERR_INVALID, "an empty entry", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, nine, 1, 0, stats, marks) == TGX_ERR_INVALID, "nine bytes", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, space, 1, 0, stats, marks) == TGX_ERR_INVALID, "a space byte", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, dup, twice, 2, 0, stats, marks) == TGX_ERR_INVALID, "an entry twice", 0);
        {
            std::vector<uint8_t> many;
            std::vector<uint64_t> many_offs(1, 0);
            for (int k = 0; k < 64; k++) {
                many.push_back((uint8_t)('a' + k % 26));
                many.push_back((uint8_t)('a' + k / 26));
                many_offs.push_back(many.size());
            }
            expect(tgx_word_stats_host(d, good, 2, 5, many.data(), many_offs.data(), 64, 0, stats, marks) == TGX_ERR_INVALID, "64 entries", 0);
            std::fill(stats, stats + 2 * TGX_WORDSTAT_N, -7);
            expect(tgx_word_stats_host(d, good, 2, 5, many.data(), many_offs.data(), 63, 0, stats, nullptr) == TGX_OK && stats[0] == 1 && stats[1] == 1, "63 entries", 0);
            std::fill(stats, stats + 2 * TGX_WORDSTAT_N, -7);
        }
        bool untouched = marks[0] == 7 && marks[1] == 7 && marks[2] == 7;
        for (int k = 0; k < 2 * TGX_WORDSTAT_N; k++) untouched = untouched && stats[k] == -7;
        expect(untouched, "a refused call writes nothing", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, upper, 1, 0, stats, marks) == TGX_OK && marks[0] == 3 && marks[1] == 0 && marks[2] == 3, "A-Z without the fold", 0);
        expect(tgx_word_stats_host(d, good, 2, 5, w, ok2, 2, TGX_WORDSTAT_FOLD, stats, nullptr) == TGX_ERR_INVALID, "the second entry holds A-Z", 0);
    }
    carry_op_is_associative();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("wordstat twin: ok\n");
    return 0;
}
