// A deterministic automaton of up to 64 states over the bytes of every row on the device (include/tgx_patterns64.h:
// tgx_corpus_dfa64_hits_device; dfa64.h has the table, the step, the maps and the units).  The
// nibble maps of dfa.hip cannot grow past sixteen states, so this family divides the work the other classical way.  It
// speculates wide and replays narrow:
//
//   dfa64_map_kernel, a lane per STATE.  A wave owns whole segments.  It loads a chunk's 64 bytes a lane a byte, and then
//     reads them back one at a time as a wave-uniform value while lane s advances the run that began in state s: one
//     v_readlane, one add and one ds_read_u8 at byte * 64 + state per byte.  After 64 bytes the lanes hold the chunk's
//     map, one coalesced store; `a then b` of two maps is one ds_bpermute (lane s fetches b from lane a[s]), which folds
//     the chunk into the segment's record.
//   dfa64_scan: the segments' records fold into their group's (dfa64_fold_kernel), one wave chains the groups' records
//     from `start` (dfa64_chain_kernel, carried), and a wave per group chains its segments' records from the group's
//     entry state.  A chain is 64 dependent v_readlane, the state an SGPR.
//   dfa64_replay_kernel, a lane per CHUNK.  A segment's wave chains its 64 chunk maps from the segment's entry state,
//     and lane k then walks chunk k from its entry with 16-byte loads and stores: 64 chunks side by side.
//   dfa64_count_kernel: the tags per row on textstat_walk's tiling, by dfa_kernel's rule.
//
// The table, 16 448 bytes, is copied into LDS once by every block of the map and replay kernels in front of its run of
// segments.  Plain C++ and builtins; no LDS beyond the table, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfa64.h"
#include "scan_helpers.h"
#include "textstat_walk.h"

namespace tgx {

namespace {

constexpr uint32_t kDfa64Block = kDfa64BlockWaves * 64;

struct alignas(16) Dfa64Lds {
    uint8_t next[256 * kDfa64MaxStates];
    uint8_t tag[kDfa64MaxStates];
};
static_assert(sizeof(Dfa64Lds) == kDfa64TableBytes && kDfa64TableBytes % 16 == 0, "the table is copied sixteen bytes a thread");

__device__ inline void dfa64_load_table(const uint8_t* __restrict__ table, Dfa64Lds& lds) {
    const uint4* src = reinterpret_cast<const uint4*>(table);
    uint4* dst = reinterpret_cast<uint4*>(&lds);
    for (uint32_t i = threadIdx.x; i < kDfa64TableBytes / 16; i += kDfa64Block) dst[i] = src[i];
    __syncthreads();
}

// the wave's run of consecutive segments, [begin, end)
struct Dfa64Run {
    uint64_t begin, end;
};
__device__ inline Dfa64Run dfa64_run(uint64_t n_segs) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t waves = (uint64_t)gridDim.x * kDfa64BlockWaves, per = (n_segs + waves - 1) / waves;
    const uint64_t begin = ((uint64_t)blockIdx.x * kDfa64BlockWaves + wave) * per;
    return {begin < n_segs ? begin : n_segs, begin + per < n_segs ? begin + per : n_segs};
}

// `a` then `b`, a lane a state: lane s fetches b from lane a[s]
__device__ inline uint32_t dfa64_then(uint32_t a, uint32_t b) { return (uint32_t)__shfl((int)b, (int)a, 64); }

// ---- a lane per state -------------------------------------------------------------------------------------------------
// The map of a full chunk at lane s: the run from state s over the chunk's 64 bytes.  b64: the lane's byte * 64; byte j
// is read from lane j as a wave-uniform value.  mask: the chunk's row starts, where every run takes `start` first.
template <bool kStarts>
__device__ inline uint32_t dfa64_walk_full(const Dfa64Lds& lds, uint32_t b64, uint64_t mask, uint32_t start, uint32_t s) {
#pragma unroll
    for (uint32_t j = 0; j < kDfa64Chunk; j++) {
        if (kStarts && ((mask >> j) & 1ull)) s = start;
        s = dfa64_step_at(lds.next, (uint32_t)__builtin_amdgcn_readlane((int)b64, (int)j), s);
    }
    return s;
}
// the corpus's last chunk, n_in < 64 bytes: the bytes past the end leave the map alone
__device__ inline uint32_t dfa64_walk_short(const Dfa64Lds& lds, uint32_t b64, uint64_t mask, uint32_t n_in, uint32_t start, uint32_t s) {
    for (uint32_t j = 0; j < n_in; j++) {
        if ((mask >> j) & 1ull) s = start;
        s = dfa64_step_at(lds.next, (uint32_t)__builtin_amdgcn_readlane((int)b64, (int)j), s);
    }
    return s;
}

// cmap, cmask of every chunk of every segment (the identity and 0 past the corpus's end) and srec of every segment
__global__ __launch_bounds__(kDfa64Block) void dfa64_map_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows, uint64_t N,
                                                                uint32_t start, const uint8_t* __restrict__ table, uint8_t* __restrict__ cmap,
                                                                uint64_t* __restrict__ cmask, uint8_t* __restrict__ srec) {
    __shared__ Dfa64Lds lds;
    dfa64_load_table(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const Dfa64Run run = dfa64_run(dfa64_segs(N));
    uint64_t hi = 0;
    bool first = true;
    for (uint64_t seg = run.begin; seg < run.end; seg++) {
        uint32_t seg_map = lane;
        for (uint32_t k = 0; k < kDfa64SegChunks; k++) {
            const uint64_t chunk = seg * kDfa64SegChunks + k, c0 = chunk * kDfa64Chunk;
            const uint32_t n_in = dfa64_chunk_bytes(c0, N);
            uint32_t m = lane;
            uint64_t mask = 0;
            if (n_in) {
                // the owners of the chunk's ends, galloped from the chunk before as in textstat_walk, and a lane's between them
                const uint64_t lo = first ? pack_find_row(offs, 0, 0, n_rows - 1, c0) : dedup_find_from(offs, hi, n_rows - 1, c0);
                hi = dedup_find_from(offs, lo, n_rows - 1, c0 + n_in - 1);
                first = false;
                uint32_t b64 = 0;
                bool row_first = false;
                if (lane < n_in) {
                    const uint64_t pos = c0 + lane;
                    row_first = offs[pack_find_row(offs, 0, lo, hi, pos)] == pos;
                    b64 = (uint32_t)text[pos] * kDfa64MaxStates;
                }
                mask = __ballot(row_first);
                if (n_in < kDfa64Chunk)
                    m = dfa64_walk_short(lds, b64, mask, n_in, start, lane);
                else if (mask)
                    m = dfa64_walk_full<true>(lds, b64, mask, start, lane);
                else
                    m = dfa64_walk_full<false>(lds, b64, mask, start, lane);
            }
            cmap[chunk * kDfa64Map + lane] = (uint8_t)m;
            if (lane == 0) cmask[chunk] = mask;
            seg_map = dfa64_then(seg_map, m);
        }
        srec[seg * kDfa64Map + lane] = (uint8_t)seg_map;
    }
}

// ---- the scan ---------------------------------------------------------------------------------------------------------
// grec of group blockIdx.x: its segments' records folded, a wave a group
__global__ __launch_bounds__(64) void dfa64_fold_kernel(const uint8_t* __restrict__ srec, uint64_t n_segs, uint8_t* __restrict__ grec) {
    const uint32_t lane = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kDfa64Group;
    const uint32_t n = n_segs - first < kDfa64Group ? (uint32_t)(n_segs - first) : kDfa64Group;
    uint32_t r[kDfa64Group];
#pragma unroll
    for (uint32_t k = 0; k < kDfa64Group; k++) r[k] = k < n ? (uint32_t)srec[(first + k) * kDfa64Map + lane] : lane;
    uint32_t acc = lane;
#pragma unroll
    for (uint32_t k = 0; k < kDfa64Group; k++) acc = dfa64_then(acc, r[k]);
    grec[(uint64_t)blockIdx.x * kDfa64Map + lane] = (uint8_t)acc;
}

// dfa64_chain_host on a wave: n <= 64 consecutive maps, a lane a state, loaded at once; e, wave-uniform, is the state in
// front of the first and becomes the state behind the last.  -> at lane k the state in front of map k.
__device__ inline uint32_t dfa64_chain(const uint8_t* __restrict__ maps, uint32_t n, uint32_t lane, uint32_t& e) {
    uint32_t m[64];
#pragma unroll
    for (uint32_t k = 0; k < 64; k++) m[k] = k < n ? (uint32_t)maps[k * kDfa64Map + lane] : lane;
    uint32_t mine = e;
#pragma unroll
    for (uint32_t k = 0; k < 64; k++) {
        if (lane == k) mine = e;
        e = (uint32_t)__builtin_amdgcn_readlane((int)m[k], (int)e);
    }
    return mine;
}

// out[k] = the state in front of map k.  kCarried: one wave takes all the maps from `start`, 64 at a time; else a wave
// takes the 64 maps of batch b from entry[b].
template <bool kCarried>
__global__ __launch_bounds__(64) void dfa64_chain_kernel(const uint8_t* __restrict__ maps, uint64_t n_maps, const uint8_t* __restrict__ entry, uint32_t start,
                                                         uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t n_batches = (n_maps + 63) / 64;
    uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
    for (uint64_t b = kCarried ? 0 : blockIdx.x; b < n_batches; b += kCarried ? 1 : gridDim.x) {
        if (!kCarried) e = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry[b]);
        const uint32_t n = n_maps - b * 64 < 64 ? (uint32_t)(n_maps - b * 64) : 64u;
        const uint32_t mine = dfa64_chain(maps + b * 64 * kDfa64Map, n, lane, e);
        if (lane < n) out[b * 64 + lane] = (uint8_t)mine;
    }
}

// ---- a lane per chunk -------------------------------------------------------------------------------------------------
// The tags of the n bytes of the chunk at c0, walked from state s.  wide: text and tags are 16-byte aligned.
__device__ inline void dfa64_replay_chunk(const Dfa64Lds& lds, const uint8_t* __restrict__ text, uint64_t c0, uint32_t n, uint64_t mask, uint32_t s,
                                          uint32_t start, uint8_t* __restrict__ tags, bool wide) {
    if (n == kDfa64Chunk && wide) {
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint4 w = reinterpret_cast<const uint4*>(text + c0)[q];
            const uint32_t in[4] = {w.x, w.y, w.z, w.w};
            uint32_t out[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                out[i] = 0;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    s = dfa64_step(lds.next, s, (in[i] >> (8 * j)) & 255u, (mask >> (16 * q + 4 * i + j)) & 1ull, start);
                    out[i] |= (uint32_t)lds.tag[s] << (8 * j);
                }
            }
            reinterpret_cast<uint4*>(tags + c0)[q] = make_uint4(out[0], out[1], out[2], out[3]);
        }
    } else {
        for (uint32_t j = 0; j < n; j++) {
            s = dfa64_step(lds.next, s, text[c0 + j], (mask >> j) & 1ull, start);
            tags[c0 + j] = lds.tag[s];
        }
    }
}

// tags[p] of every byte
__global__ __launch_bounds__(kDfa64Block) void dfa64_replay_kernel(const uint8_t* __restrict__ text, uint64_t N, uint32_t start, const uint8_t* __restrict__ table,
                                                                   const uint8_t* __restrict__ cmap, const uint64_t* __restrict__ cmask,
                                                                   const uint8_t* __restrict__ sentry, uint8_t* __restrict__ tags, bool wide) {
    __shared__ Dfa64Lds lds;
    dfa64_load_table(table, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const Dfa64Run run = dfa64_run(dfa64_segs(N));
    for (uint64_t seg = run.begin; seg < run.end; seg++) {
        uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)sentry[seg]);
        const uint32_t s = dfa64_chain(cmap + seg * kDfa64SegChunks * kDfa64Map, kDfa64SegChunks, lane, e);
        const uint64_t chunk = seg * kDfa64SegChunks + lane, c0 = chunk * kDfa64Chunk;
        const uint32_t n = dfa64_chunk_bytes(c0, N);
        if (n) dfa64_replay_chunk(lds, text, c0, n, cmask[chunk], s, start, tags, wide);
    }
}

// ---- the counts -------------------------------------------------------------------------------------------------------
// count[i] of every nonempty row i (the launcher pre-set the counts to 0, which empty rows keep), dfa_kernel's rule to
// the letter: the ballot of the tagged lanes is cut into the chunk's stretches of one row; the lane at which a stretch
// begins popcounts the stretch's part and stores it plainly when the row lies inside the chunk, else adds it.
__global__ __launch_bounds__(kTextstatBlock) void dfa64_count_kernel(const uint8_t* __restrict__ text, const uint64_t* __restrict__ offs, uint64_t n_rows,
                                                                     const uint8_t* __restrict__ tags, unsigned long long* count) {
    const uint32_t lane = threadIdx.x & 63u;
    textstat_walk(text, offs, n_rows, [=](uint64_t c0, uint32_t n_in, uint64_t, const TextLane& t) {
        const uint64_t tagged = __ballot(t.in && tags[t.pos] != 0);
        const uint32_t row_before = (uint32_t)__shfl_up((int)t.row, 1, 64);
        const bool begins = t.in && (lane == 0 || t.row != row_before);
        const uint64_t heads = __ballot(begins);
        if (begins) {
            const uint64_t above = heads & ~textstat_below(lane + 1);  // the stretches that begin after this lane
            const uint32_t end = above ? (uint32_t)__builtin_ctzll(above) : n_in;
            const unsigned long long v = textstat_popc(tagged & textstat_span(lane, end - 1));
            if (textstat_row_inside(offs, t.row, c0))
                count[t.row] = v;
            else if (textstat_adds(v))
                atomicAdd(&count[t.row], v);
        }
    });
}

bool dfa64_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_dfa64_map(const DedupRows& rows, uint32_t start, const uint8_t* table, uint8_t* cmap, uint64_t* cmask, uint8_t* srec, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(dfa64_grid(dfa64_segs(rows.n_elems), kTextstatMaxBlocks)), block(kDfa64Block);
    hipLaunchKernelGGL(dfa64_map_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, rows.n_elems, start, table, cmap,
                       cmask, srec);
    return hipGetLastError();
}

hipError_t launch_dfa64_scan(uint32_t start, const uint8_t* srec, uint64_t n_segs, uint8_t* grec, uint8_t* gentry, uint8_t* sentry, hipStream_t stream) {
    if (n_segs == 0) return hipSuccess;
    const uint64_t n_groups = dfa64_groups(n_segs);
    hipLaunchKernelGGL(dfa64_fold_kernel, dim3((uint32_t)n_groups), dim3(64), 0, stream, srec, n_segs, grec);
    hipLaunchKernelGGL(dfa64_chain_kernel<true>, dim3(1), dim3(64), 0, stream, static_cast<const uint8_t*>(grec), n_groups, nullptr, start, gentry);
    hipLaunchKernelGGL(dfa64_chain_kernel<false>, dim3(capped_grid(n_groups, 1u << 20)), dim3(64), 0, stream, srec, n_segs, static_cast<const uint8_t*>(gentry),
                       start, sentry);
    return hipGetLastError();
}

hipError_t launch_dfa64_replay(const DedupRows& rows, uint32_t start, const uint8_t* table, const uint8_t* cmap, const uint64_t* cmask, const uint8_t* sentry,
                               uint8_t* tags, hipStream_t stream) {
    if (rows.n_rows == 0 || rows.n_elems == 0) return hipSuccess;
    const dim3 grid(dfa64_grid(dfa64_segs(rows.n_elems), kTextstatMaxBlocks)), block(kDfa64Block);
    hipLaunchKernelGGL(dfa64_replay_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.n_elems, start, table, cmap, cmask, sentry, tags,
                       dfa64_aligned16(rows.data) && dfa64_aligned16(tags));
    return hipGetLastError();
}

hipError_t launch_dfa64_count(const DedupRows& rows, const uint8_t* tags, int64_t* count, hipStream_t stream) {
    if (rows.n_rows == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(count, 0, (size_t)rows.n_rows * 8, stream);
    if (e != hipSuccess || rows.n_elems == 0) return e;
    const dim3 grid(grid_for(rows.n_elems, kTextstatTile, kTextstatMaxBlocks)), block(kTextstatBlock);
    hipLaunchKernelGGL(dfa64_count_kernel, grid, block, 0, stream, static_cast<const uint8_t*>(rows.data), rows.offs, rows.n_rows, tags,
                       reinterpret_cast<unsigned long long*>(count));
    return hipGetLastError();
}

}  // namespace tgx
