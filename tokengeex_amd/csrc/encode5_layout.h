// The LDS of an encode5_kernel block (encode5.hip), as plain host arithmetic: what the launcher lays out, what the geometry
// (encode_pass.cpp: choose_encode5) sizes the table of hot score values by, and what tests/native/top_table_main.cpp checks.
//
//   [0, 8 (n_hot + 1))   the score table: entry 0 = -inf ("no token"), then the n_hot hottest values (16-aligned)
//   LONG builds          the waves' lists of long matches
//   2 048 bytes          a copy of the root's 256 records — absent in the TOP builds, whose walks take their first two
//                        levels from the top table in HBM / L2 (top_table.h)
//   512-aligned          waves x ppl match-index buffers of kE5GroupBytes
#pragma once
#include <stdint.h>

namespace tgx {

// match-index buffer of one 16-position group: four sample rows of 16 columns x 16 start positions x 2 bytes
constexpr uint32_t kE5RowStride = 512;
constexpr uint32_t kE5GroupBytes = 4 * kE5RowStride;  // 2048
constexpr uint32_t kE5RootBytes = 256u * 8u;          // the root's 256 records
constexpr uint32_t kE5TopBytes = 8u << 16;            // the top table in HBM (top_table.h): 65 536 records
constexpr uint32_t kE5LongCap = 62;                         // list entries per wave and iteration
constexpr uint32_t kE5LongBytes = 8u + kE5LongCap * 4u;     // {count, pad} + entries {lane | group << 6 | depth << 8 | rank << 16}

// LDS of one block of `waves` waves: score table (-inf and n_hot values), the waves' lists of long matches (LONG
// builds), root records (not in the TOP builds), match indices
inline uint32_t encode5_lds_layout(uint32_t n_hot, bool long_tokens, int waves, int ppl, uint32_t* list_off, uint32_t* root_off, uint32_t* idx_off,
                                   bool top = false) {
    const uint32_t lo = (8u * (n_hot + 1u) + 15u) & ~15u;
    const uint32_t score_bytes = lo + (long_tokens ? (uint32_t)waves * ((kE5LongBytes + 15u) & ~15u) : 0u);
    if (list_off) *list_off = lo;
    const uint32_t ro = (score_bytes + 15u) & ~15u;
    const uint32_t io = (ro + (top ? 0u : kE5RootBytes) + 511u) & ~511u;  // 512-byte aligned: see kE5RowStride
    if (root_off) *root_off = ro;
    if (idx_off) *idx_off = io;
    return io + (uint32_t)waves * (uint32_t)ppl * kE5GroupBytes;
}

// The largest table that leaves a block of `waves` waves within `budget` bytes of LDS.
// TOP layout: exact — the largest n_hot whose layout fits (n_hot + 1 does not).  The layout with the root copy keeps the
// estimate it always had (512 bytes of alignment slack, up to 127 values short): TGX_E5_TOP=0, the LONG and DROPOUT builds
// and the E-step's forward kernel run the geometry they ran before the top table.
inline uint32_t encode5_max_hot(bool long_tokens, int waves, int ppl, uint32_t budget, bool top = false) {
    if (!top) {
        const uint32_t fixed = encode5_lds_layout(0u, long_tokens, waves, ppl, nullptr, nullptr, nullptr) + 512u;  // alignment slack
        return budget > fixed + 64u ? (budget - fixed) / 8u : 0u;
    }
    const uint32_t idx_bytes = (uint32_t)waves * (uint32_t)ppl * kE5GroupBytes;
    if (budget < idx_bytes) return 0u;
    const uint32_t io_max = (budget - idx_bytes) & ~511u;  // the highest start of the index buffers
    const uint32_t lists = long_tokens ? (uint32_t)waves * ((kE5LongBytes + 15u) & ~15u) : 0u;
    // io = round512(round16(8 (n_hot + 1)) + lists) <= io_max  <=>  8 (n_hot + 1) <= io_max - lists (both multiples of 16)
    return io_max >= lists + 16u ? (io_max - lists) / 8u - 1u : 0u;
}

}  // namespace tgx
