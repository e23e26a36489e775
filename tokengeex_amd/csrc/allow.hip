// The window stage of the document-frequency pass under an allow automaton (include/tgx_allow.h: tgx_substring_df_allow;
// allow.h has the walk's trip, the mask and the geometry).  generate.hip's window kernels hash and
// emit every char-aligned window and leave the allow regex to the host; here the automaton is walked from every start byte
// first and only the windows it accepts are hashed, sorted and counted.
//
//   allow_mask_kernel, a lane per START byte, a wave per chunk of 64 positions, a run of chunks per wave.  The block copies
//     the automaton's table (find.h's: state, tagged and dead in one byte, 16 KiB) into LDS once.  A wave holds its chunk's
//     64 bytes and the 64 behind them in ONE register, a lane two bytes; at trip t lane j reads byte j + t from lane
//     (j + t) & 63 with one ds_bpermute and takes its low or its high byte, settles the window of t bytes that trip t - 1
//     left pending (the byte is no continuation byte: a character boundary), and advances its walk with one ds_read_u8.
//     The loop runs while a ballot of the busy lanes is non-empty: max_len + 1 trips at most, the last only settling; on
//     ordinary text most lanes are dead within a few bytes, so the time depends on the text and the automaton.  No byte
//     is loaded from global memory inside the loop and there is no barrier after the table's copy.  It stores a 32-bit
//     mask per position and the chunk's number of set bits.
//   allow_emit_kernel, the same geometry and the same text register, no table.  A lane hashes its bytes up to its mask's
//     highest bit — generate.h's two chains, exactly window_kernel's keys — and writes {key, sample | position | length}
//     for the set bits from the chunk's offset plus the wave's prefix of popcounts: position order.  It neither walks nor
//     draws, so a collision retry repeats this kernel alone.
// Integer and byte work; no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "allow.h"

namespace tgx {

namespace {

constexpr uint32_t kAllowBlockWaves = 4;
constexpr uint32_t kAllowBlock = kAllowBlockWaves * 64;
constexpr uint32_t kAllowMinRun = 4;        // chunks a wave takes at least
constexpr uint32_t kAllowMaxBlocks = 2048;  // beyond it the runs grow: a block's copy of the table serves more text

struct alignas(16) AllowLds {
    uint8_t next[kFindTableBytes];
};

// the wave's run of consecutive chunks, [begin, end)
struct AllowRun {
    uint64_t begin, end;
};
__device__ inline AllowRun allow_run(uint64_t n_chunks) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t waves = (uint64_t)gridDim.x * kAllowBlockWaves, per = (n_chunks + waves - 1) / waves;
    const uint64_t begin = ((uint64_t)blockIdx.x * kAllowBlockWaves + wave) * per;
    return {begin < n_chunks ? begin : n_chunks, begin + per < n_chunks ? begin + per : n_chunks};
}

// the chunk's byte of this lane in the low byte and the one 64 behind it in the high one; 0 past the text
__device__ inline uint32_t allow_two(const uint8_t* __restrict__ text, uint64_t n_bytes, uint64_t p) {
    const uint64_t behind = p + kAllowChunk;
    return (p < n_bytes ? (uint32_t)text[p] : 0u) | (behind < n_bytes ? (uint32_t)text[behind] << 8 : 0u);
}
// byte lane + t of the chunk, t <= kAllowMaxLen; every lane of the wave calls it
__device__ inline uint32_t allow_byte(uint32_t two, uint32_t lane, uint32_t t) {
    const uint32_t v = (uint32_t)__shfl((int)two, (int)((lane + t) & 63u), 64);
    return lane + t < kAllowChunk ? v & 255u : v >> 8;
}

// the part of position p, found as window_kernel finds it: -> its index, or n_parts when p lies in none
__device__ inline uint64_t allow_part(const AllowParams& P, uint64_t chunk, uint64_t p) {
    uint64_t k = P.blk_part[chunk / kAllowBlockChunks];
    while (k < P.n_parts && P.part_end[k] <= p) k++;
    return k < P.n_parts && P.part_begin[k] <= p ? k : P.n_parts;
}

__global__ __launch_bounds__(kAllowBlock) void allow_mask_kernel(AllowParams P) {
    __shared__ AllowLds lds;
    {
        const uint4* src = reinterpret_cast<const uint4*>(P.table);
        uint4* dst = reinterpret_cast<uint4*>(&lds);
        for (uint32_t i = threadIdx.x; i < kFindTableBytes / 16; i += kAllowBlock) dst[i] = src[i];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    const AllowRun run = allow_run(allow_chunks(P.n_bytes));
    for (uint64_t chunk = run.begin; chunk < run.end; chunk++) {
        const uint64_t p = chunk * kAllowChunk + lane;
        const uint32_t two = allow_two(P.text, P.n_bytes, p);
        uint64_t end = 0;  // of this position's part; 0: the position starts no window
        AllowDraw d = {P.prob, P.seed, 0u, 0ull};
        if (p < P.n_bytes && (two & 0xC0u) != 0x80u) {  // a character start
            const uint64_t k = allow_part(P, chunk, p);
            if (k < P.n_parts) {
                end = P.part_end[k];
                d.sample = P.part_sample[k];
                d.offset = p - P.part_origin[k];
            }
        }
        const uint32_t limit = end ? find_limit(p, end, P.max_len) : 0u;
        const bool ends_part = p + limit == end;
        AllowWalk w = allow_begin(P.start, limit);
        for (uint32_t t = 0; __ballot(allow_busy(w)) != 0; t++) {
            const uint32_t b = allow_byte(two, lane, t);
            if (allow_busy(w)) allow_trip(lds.next, b, t, limit, ends_part, d, w);
        }
        if (p < P.n_bytes) P.mask[p] = w.mask;
        uint32_t kept = (uint32_t)__popc(w.mask);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kept += (uint32_t)__shfl_xor((int)kept, off, 64);
        if (lane == 0) P.chunk_count[chunk] = kept;
    }
}

__global__ __launch_bounds__(kAllowBlock) void allow_emit_kernel(AllowParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const AllowRun run = allow_run(allow_chunks(P.n_bytes));
    for (uint64_t chunk = run.begin; chunk < run.end; chunk++) {
        const uint64_t p = chunk * kAllowChunk + lane;
        const uint32_t two = allow_two(P.text, P.n_bytes, p);
        uint32_t m = p < P.n_bytes ? P.mask[p] : 0u;
        uint32_t sample = 0;
        if (m) {
            const uint64_t k = allow_part(P, chunk, p);
            if (k < P.n_parts)
                sample = P.part_sample[k];
            else
                m = 0;  // (a set bit outside every part cannot come out of allow_mask_kernel)
        }
        const uint32_t kept = (uint32_t)__popc(m), top = 32u - (uint32_t)__clz(m);  // the bytes to hash: 0 for an empty mask
        // wave-level exclusive prefix of `kept` (position order)
        uint32_t incl = kept;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64);
            if ((int)lane >= off) incl += y;
        }
        uint64_t at = P.chunk_offs[chunk] + (incl - kept);
        uint64_t h = kFnvOffset, g = kFnvOffset ^ P.salt;
        for (uint32_t t = 0; __ballot(t < top) != 0; t++) {
            const uint64_t c = allow_byte(two, lane, t);
            generate_hash_byte(c, P.salt, h, g);
            if ((m >> t) & 1u) {
                P.keys[at] = (P.salt ? g : h) & P.key_mask;
                P.vals[at] = generate_value(sample, p, t + 1);
                at++;
            }
        }
    }
}

inline dim3 allow_grid(uint64_t n_bytes) {
    const uint64_t per_block = (uint64_t)kAllowBlockWaves * kAllowMinRun, blocks = (allow_chunks(n_bytes) + per_block - 1) / per_block;
    return dim3((uint32_t)(blocks < kAllowMaxBlocks ? blocks : kAllowMaxBlocks));
}

}  // namespace

hipError_t launch_allow_mask(const AllowParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(allow_mask_kernel, allow_grid(P.n_bytes), dim3(kAllowBlock), 0, stream, P);
    return hipGetLastError();
}

hipError_t launch_allow_emit(const AllowParams& P, hipStream_t stream) {
    hipLaunchKernelGGL(allow_emit_kernel, allow_grid(P.n_bytes), dim3(kAllowBlock), 0, stream, P);
    return hipGetLastError();
}

}  // namespace tgx
