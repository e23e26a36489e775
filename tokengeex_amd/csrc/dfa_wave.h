// The in-wave scans of state maps that the kernels of dfa.hip and cover.hip share (dfa.h has the map, its composition
// and the constant map of a row's edge; textstat_walk.h the walk and a lane's byte): the block's copy of an automaton's
// table in LDS, the forward scan in six doubling steps, and the same scan from right to left.  Device code only, for a
// translation unit with kernels.  DESIGN.md, sections L.18 and L.19.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfa.h"
#include "textstat_walk.h"

namespace tgx {

// The block's copy of the table: thread t takes map t, the first sixteen threads a tag each.
template <uint32_t NS>
struct DfaLds {
    DfaMap<NS> map[256];
    uint8_t tag[kDfaMaxStates];
};
template <uint32_t NS>
__device__ inline void dfa_load_table(const uint64_t* __restrict__ table, DfaLds<NS>& lds) {
    static_assert(kTextstatBlock == 256, "a thread a map");
    lds.map[threadIdx.x] = reinterpret_cast<const DfaMap<NS>*>(table)[threadIdx.x];
    if (threadIdx.x < kDfaMaxStates) lds.tag[threadIdx.x] = reinterpret_cast<const uint8_t*>(table + kDfaMapWords<NS>)[threadIdx.x];
    __syncthreads();
}

template <uint32_t NS, uint32_t D>
__device__ inline DfaMap<NS> dfa_step(DfaMap<NS> mine, uint32_t lane) {
    const DfaMap<NS> below = __shfl_up(mine, D, 64);
    return lane >= D ? dfa_compose<NS>(below, mine) : mine;
}
// every lane's scanned map: that of the chunk's bytes up to and including its own (the identity in a lane without a byte)
template <uint32_t NS>
__device__ inline DfaMap<NS> dfa_chunk(const DfaLds<NS>& lds, const TextLane& t, uint32_t lane, uint32_t start) {
    DfaMap<NS> m = dfa_identity<NS>();
    if (t.in) m = dfa_lane_map<NS>(lds.map[t.b], t.pos == t.row_begin, start);
    m = dfa_step<NS, 1>(m, lane);
    m = dfa_step<NS, 2>(m, lane);
    m = dfa_step<NS, 4>(m, lane);
    m = dfa_step<NS, 8>(m, lane);
    m = dfa_step<NS, 16>(m, lane);
    m = dfa_step<NS, 32>(m, lane);
    return m;
}

// ---- right to left (cover.hip) ---------------------------------------------------------------------------------------
// A backward automaton consumes the bytes to a lane's right first, so in step d a lane i < 64 - d composes the map of
// lane i + d IN FRONT of its own.  A lane without a byte holds the identity, so a short chunk needs no bound of its own.
template <uint32_t NS, uint32_t D>
__device__ inline DfaMap<NS> dfa_step_back(DfaMap<NS> mine, uint32_t lane) {
    const DfaMap<NS> above = __shfl_down(mine, D, 64);
    return lane < 64u - D ? dfa_compose<NS>(above, mine) : mine;
}
// Every lane's scanned map: that of the chunk's bytes from its last down to and including the lane's own.  maps: the
// backward automaton's 256 maps in LDS.  A row's LAST byte has the constant map, which drops whatever lies to its right
// as the constant map of a row's first byte drops what precedes it in dfa_chunk.
template <uint32_t NS>
__device__ inline DfaMap<NS> dfa_chunk_back(const DfaMap<NS>* maps, const TextLane& t, uint32_t lane, uint32_t start) {
    DfaMap<NS> m = dfa_identity<NS>();
    if (t.in) m = dfa_lane_map<NS>(maps[t.b], t.pos + 1 == t.row_end, start);
    m = dfa_step_back<NS, 1>(m, lane);
    m = dfa_step_back<NS, 2>(m, lane);
    m = dfa_step_back<NS, 4>(m, lane);
    m = dfa_step_back<NS, 8>(m, lane);
    m = dfa_step_back<NS, 16>(m, lane);
    m = dfa_step_back<NS, 32>(m, lane);
    return m;
}

}  // namespace tgx
