// rrt_tree_dev.h -- device building blocks of the tree-call kernels (rrt_routes.h, rrt_keep.h, rrt_seed.h, rrt_reroot.h, rrt_relax.h and the pose
// calls of unit 9; kernels_tu.hip units 0, 6, 7, 8, 9).  No expansion kernel includes this file.
//
//   wg_scan_step        the cross-wave step of an exclusive scan by ONE workgroup of TPB threads
//   jump_round          one round of pointer jumping, with or without the depth
//   wave_each_key       the walk over the distinct keys of a wavefront
//   wave_place_by_key   on top of it: stable placement behind per-key cursors in the wavefront's own LDS
#pragma once

#include "rrt_device.h"

namespace rrtdev {

// One pass of an exclusive scan over TPB values a pass by one workgroup of TPB threads.  wave_total: the sum over this wavefront's
// lanes, as lane 63 holds it (the last lane of wave_incl_sum_u32).  before: the totals of the
// lower wavefronts; total: of all of them, the pass total, which the caller adds to the carry it keeps in a register.  One barrier a
// pass: the wave totals live in [2][NWAVE] LDS words, `par` (0 in front of the first pass) names the half this pass writes, and the
// next pass writes the other half -- a wavefront still reading pass p cannot meet the writes of pass p + 2, whose writers have passed
// the barrier of pass p + 1.  Every thread of the workgroup calls it, the same number of times.  (rrt_keep_compact_kernel, rrt_keep.h,
// holds the one copy of this step written out, and says why.)
struct WgScan {
    uint32_t before, total;
};
__device__ __forceinline__ WgScan wg_scan_step(uint32_t wave_total, int &par) {
    __shared__ uint32_t wsum[2][NWAVE];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if (lane == 63) wsum[par][wave] = wave_total;
    __syncthreads();
    WgScan s{0u, 0u};
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) {
        const uint32_t v = wsum[par][w];
        s.before += w < wave ? v : 0u;
        s.total += v;
    }
    par ^= 1;
    return s;
}

// One round of pointer jumping, one vertex per lane: ok2[k] = ok[k] & ok[anc[k]], anc2[k] = anc[anc[k]] and, with DEPTH,
// dep2[k] = dep[k] + dep[anc[k]], the number of edges between k and anc2[k].  Every anc[k] is in [0, j) (the kernel in front wrote it
// so, and a round keeps it so).  After r rounds ok[k] covers the 2^r vertices from k towards the root, so ceil(log2(max(j, 2)))
// rounds cover any depth below j: the host queues that many launches, ping-ponging two sets of buffers (jump_rounds,
// rrt_tree_calls.hip).  parent[k] < k is not assumed.  Nothing is read back and nothing waits across workgroups.
template <bool DEPTH>
__device__ __forceinline__ void jump_round(const uint8_t *ok, const int32_t *anc, const int32_t *dep, uint8_t *ok2, int32_t *anc2, int32_t *dep2, int32_t j) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= j) return;
    const int a = anc[k];
    ok2[k] = ok[k] & ok[a];
    anc2[k] = anc[a];
    // (of a vertex on a cycle the depth may wrap: such a vertex never reaches the root)
    if (DEPTH) dep2[k] = (int32_t)((uint32_t)dep[k] + (uint32_t)dep[a]);
}

// The distinct keys among the lanes with `in`, one after the other: f(key, same, here) with key and same uniform, `same` the ballot of
// the lanes that hold the key and `here` this lane's bit of it.  Called by the whole wavefront (lanes without `in` take part in the ballots).
template <typename F>
__device__ __forceinline__ void wave_each_key(bool in, int key, F f) {
    unsigned long long m = __ballot(in);
    while (m) {
        const int kl = __builtin_amdgcn_readlane(key, (int)__builtin_ctzll(m));
        const bool here = in && key == kl;
        const unsigned long long same = __ballot(here);
        f(kl, same, here);
        m &= ~same;
    }
}

// Stable placement by an OWNED key.  The wavefront numbered gw of OWNERS owns the keys with key % OWNERS == gw (`mine`: this lane's item
// has such a key) and walks the items in ascending index, 64 a step, lane l the l-th: the items of a key go behind the key's cursor
// cur[key / OWNERS], lanes in ascending order -- store(key, pos) in the lanes that hold it -- and lane 0 advances the cursor.  A key is
// placed by one wavefront only, in ascending index, with its cursors in that wavefront's own LDS words (volatile: read and written in
// program order by the one wavefront): ordered placement without a barrier, without atomics and without a wait across wavefronts or
// workgroups.  store checks pos against the room it has.
template <int OWNERS, typename T, typename F>
__device__ __forceinline__ void wave_place_by_key(bool mine, int key, volatile RRT_LDS T *cur, F store) {
    const int lane = (int)threadIdx.x & 63;
    wave_each_key(mine, key, [&](int kl, unsigned long long same, bool here) {
        const int slot = kl / OWNERS;
        const T before = cur[slot];
        if (here) store(kl, before + (T)__builtin_popcountll(same & ((1ull << lane) - 1ull)));
        if (lane == 0) cur[slot] = before + (T)__builtin_popcountll(same);
    });
}

}  // namespace rrtdev
