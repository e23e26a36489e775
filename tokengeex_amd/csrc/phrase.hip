// Literal phrase matching on the device (include/tgx_phrases.h: tgx_*_phrase_hits_device; phrase.h has the definitions,
// the record format, the walk and the rules).  One kernel walks the elements of all rows laid end
// to end, a lane a start position, on the tiling of gram_walk.h.  A block copies the set's first-level filter (8 KiB) into
// LDS once and, per tile, the tile's bytes with a halo of the longest phrase, folded as they are staged.  A lane reads its
// first two bytes from LDS and ends there unless some phrase begins with them; the others walk the label-checked records
// in HBM / L2, one 8-byte gather and one compare per byte, reading the text from LDS.  The surviving lanes are not
// compacted (profiles/phrases/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gram.h"
#include "phrase.h"

namespace tgx {

namespace {

constexpr uint32_t kPhraseBlock = 256;
static_assert(kPhraseBlock == kGramTile && kGramTile == 4 * kGramChunk && kGramChunk == 64, "the host twin walks the kernel's tiles and chunks");
constexpr uint64_t kPhraseMaxBlocks = 2048;  // a capped grid; a block takes a run of consecutive tiles

// count[i] = the occurrences in row i, longest[e] = the longest occurrence that begins at element e (0: none),
// per_phrase[p] += 1 per occurrence of p.  For the counts the lanes' numbers are summed over the chunk's stretches of one
// row: the lane at which a stretch begins takes the stretch's part of the wave's prefix sums and, by the rule of gram.h,
// stores it plainly when the row lies inside the chunk and else adds it to the row's count (pre-set to 0 by the launcher).
template <uint32_t EB>
__global__ __launch_bounds__(kPhraseBlock) void phrase_hits_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                   const PhraseRec* __restrict__ table, const uint32_t* __restrict__ filter,
                                                                   uint32_t root_base, uint32_t max_bytes, uint32_t flags, unsigned long long* count,
                                                                   uint8_t* __restrict__ longest, unsigned long long* per_phrase) {
    __shared__ uint32_t s_filter[kPhraseFilterWords];
    __shared__ uint32_t s_words[(kPhraseStageBytes + 3) / 4];
    uint8_t* s_text = reinterpret_cast<uint8_t*>(s_words);
    const bool fold = flags & kPhraseFoldCase, whole = flags & kPhraseWholeWord;
    const uint64_t M = offs[n_rows], n_bytes = M * EB;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_tiles = (M + kGramTile - 1) / kGramTile, per_block = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_begin = blockIdx.x * per_block, tile_end = tile_begin + per_block < n_tiles ? tile_begin + per_block : n_tiles;
    for (uint32_t w = threadIdx.x; w < kPhraseFilterWords; w += kPhraseBlock) s_filter[w] = filter[w];
    const bool aligned = (reinterpret_cast<uintptr_t>(data) & 3u) == 0;
    const uint32_t stage_words = (kPhraseLead + kGramTile * EB + max_bytes + 3) / 4;  // <= the array: max_bytes <= kPhraseMaxBytes
    uint64_t hi = 0;
    for (uint64_t tile = tile_begin; tile < tile_end; tile++) {  // (block-uniform: every wave reaches both barriers)
        // stage word w holds the bytes g0 + 4 w .. + 3 of the source, g0 = the tile's first byte - kPhraseLead; bytes
        // outside the source read as 0
        const uint64_t t_byte = tile * kGramTile * EB;
        __syncthreads();  // the tile before has been read (and, the first time, nothing)
        for (uint32_t w = threadIdx.x; w < stage_words; w += kPhraseBlock) {
            const uint64_t g = t_byte + 4ull * w;  // = the word's first byte + kPhraseLead
            uint32_t v = 0;
            if (g >= kPhraseLead && g - kPhraseLead + 4 <= n_bytes && aligned) {
                v = *reinterpret_cast<const uint32_t*>(data + (g - kPhraseLead));
            } else {
                for (uint32_t j = 0; j < 4; j++) {
                    const uint64_t b = g + j;
                    if (b >= kPhraseLead && b - kPhraseLead < n_bytes) v |= (uint32_t)data[b - kPhraseLead] << (8 * j);
                }
            }
            s_words[w] = phrase_fold4(v, fold);
        }
        __syncthreads();
        const uint64_t c0 = tile * kGramTile + (uint64_t)wave * kGramChunk;
        if (c0 >= M) continue;  // (the last tile: the chunks after this one are empty too; the loop ends with it)
        const uint64_t c_last = tile_last(c0, kGramChunk, M);
        const uint64_t lo = tile == tile_begin ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
        hi = dedup_find_from(offs, lo, n_rows - 1, c_last);
        const uint64_t pos = c0 + lane;
        const bool in = pos <= c_last;
        uint32_t row = (uint32_t)lo;
        PhraseHit h = {0, 0};
        if (in) {
            row = (uint32_t)pack_find_row(offs, 0, lo, hi, pos);
            const uint64_t left = (offs[row + 1] - pos) * EB;
            const uint32_t avail = left > max_bytes ? max_bytes + 1 : (uint32_t)left;
            const uint8_t* s = s_text + kPhraseLead + (uint32_t)(pos - tile * kGramTile) * EB;
            const uint32_t b0 = s[0], b1 = avail >= 2 ? s[1] : 0u;
            bool go = phrase_filter_pass(s_filter, b0, b1);
            if (whole && go) go = pos == offs[row] || !phrase_word_byte(s[-1]);
            if (go)
                h = phrase_walk(table, root_base, EB, avail, max_bytes, whole, [=](uint32_t k) { return (uint32_t)s[k]; },
                                [=](uint32_t p) {
                                    // the lanes that credit the same phrase in this step add once: text repeats, and a hot
                                    // phrase is one address
                                    if (!per_phrase) return;
                                    for (bool done = false; !done;) {
                                        const uint32_t lead = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
                                        const uint64_t same = __ballot(p == lead);  // (of the lanes still in this loop)
                                        if (p == lead) {
                                            if (lane == (uint32_t)__builtin_ctzll(same)) atomicAdd(&per_phrase[lead], (unsigned long long)__popcll(same));
                                            done = true;
                                        }
                                    }
                                });
            if (longest) longest[pos] = (uint8_t)h.longest;
        }
        if (!count) continue;
        const uint32_t n_in = (uint32_t)(c_last - c0) + 1;
        uint32_t sum = h.count;  // the wave's inclusive prefix sums (at most 64 * 255)
        for (uint32_t d = 1; d < 64; d *= 2) {
            const uint32_t up = (uint32_t)__shfl_up((int)sum, d, 64);
            if (lane >= d) sum += up;
        }
        const uint32_t row_before = (uint32_t)__shfl_up((int)row, 1, 64);
        const uint32_t sum_up = (uint32_t)__shfl_up((int)sum, 1, 64);
        const uint32_t sum_before = lane ? sum_up : 0u;
        const bool begins = in && (lane == 0 || row != row_before);
        const uint64_t heads = __ballot(begins);
        const uint64_t above = heads & ~((2ull << lane) - 1);  // the stretches that begin after this lane
        const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;  // (>= 1 in every lane)
        const uint32_t sum_end = (uint32_t)__shfl((int)sum, (int)end - 1, 64);
        if (begins) {
            const unsigned long long n_hits = sum_end - sum_before;
            if (gram_row_inside(offs, row, c0))
                count[row] = n_hits;
            else if (gram_adds(n_hits))
                atomicAdd(&count[row], n_hits);
        }
    }
}

}  // namespace

hipError_t launch_phrase_hits(const DedupRows& rows, const PhraseRec* table, const uint32_t* filter, uint32_t root_base, uint32_t max_len,
                              uint32_t flags, uint32_t n_phrases, int64_t* count, uint8_t* longest, int64_t* per_phrase, hipStream_t stream) {
    if (count && rows.n_rows) {
        const hipError_t e = hipMemsetAsync(count, 0, (size_t)rows.n_rows * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (per_phrase && n_phrases) {
        const hipError_t e = hipMemsetAsync(per_phrase, 0, (size_t)n_phrases * 8, stream);
        if (e != hipSuccess) return e;
    }
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(grid_for(rows.n_elems, kGramTile, kPhraseMaxBlocks)), block(kPhraseBlock);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
    unsigned long long* per = reinterpret_cast<unsigned long long*>(per_phrase);
    const uint8_t* data = static_cast<const uint8_t*>(rows.data);
    if (rows.elem_bytes == 1)
        hipLaunchKernelGGL(phrase_hits_kernel<1>, grid, block, 0, stream, data, rows.offs, rows.n_rows, table, filter, root_base, max_len, flags, cnt,
                           longest, per);
    else
        hipLaunchKernelGGL(phrase_hits_kernel<4>, grid, block, 0, stream, data, rows.offs, rows.n_rows, table, filter, root_base, max_len * 4, flags,
                           cnt, longest, per);
    return hipGetLastError();
}

}  // namespace tgx
