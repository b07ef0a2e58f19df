// rrt_keep.h -- keep a finished tree when the map changes: which vertices still hang on the root through free edges, as a view.
//
// A finished query left nodes / parent / vcost of its vertices [0, j) on the device, root 0.  On a new map og' of the same shape
//
//   edge_ok[0] = the root's cell is free in og'
//   edge_ok[k] = collisionfree(og', nodes[parent[k]], nodes[k])   for k > 0, the line walked from the parent to the child
//   alive[k]   = edge_ok[k] and alive[parent[k]]                  every edge on the way to the root is free
//
// and the alive vertices, in their original order, are copied into three dense arrays (live_nodes, live_vcost, live_id): the view.
// The tree arrays themselves are never written.  rrt_goals_kernel runs go2goal's decision over the view -- dense indices order like
// the original ones, so the stable (cost, index) order is the original one --, rrt_keep_remap_kernel turns its answers back into
// original vertex numbers, and the route kernels walk the original parent array: every ancestor of an alive vertex is alive.
// Costs are not recomputed: a surviving vertex keeps its vcost bit for bit.
//
// The direction of the walk.  The Bresenham walk of rrt.py:202-229 is not symmetric.  plan() tested every edge of a reference-mode
// tree from the parent to the child (rrt_serial.h, the nearest / choose-parent test), so on an unchanged map every such edge is
// free here too and the view is the whole tree.  The rewire of rewire="correct" tests its new edges from the child to the new
// parent: on such a tree a rewired edge may be cut on an unchanged map, where the walk from the parent's side crosses an occupied
// cell that the walk from the child's side misses.  Only the one direction is tested.
//
//   1. rrt_keep_edge_kernel        one wavefront per vertex, grid-stride: edge_ok by los_wave (los_wave_large for a batch created with
//                                  RRT_FLAG_LARGE_GRID), and anc[k] = parent[k] (anc[0] = 0).  A parent outside [0, j): not ok.
//   2. rrt_keep_jump_kernel        one round of pointer jumping (jump_round, rrt_tree_dev.h); ceil(log2(max(j, 2))) rounds.
//   3. rrt_keep_compact_kernel     one workgroup walks [0, j) TPB vertices a pass: ballot / popcount prefixes inside a wave, the
//                                  waves' counts through LDS, the carry in a register -- wg_scan_step (rrt_tree_dev.h) written out: with
//                                  the function the compiler moves the wave counts through scalar registers, 16 readfirstlanes a
//                                  pass, and the stage measured 18 % slower (profiles/tree_kernels_shared_wall.json).  alive[k] = ok[k]
//                                  and anc[k] == 0 (a walk that is not at the root after j steps belongs to no tree: not alive).
//   4. rrt_keep_remap_kernel       vertex[g] = vertex[g] < 0 ? -1 : live_id[vertex[g]], behind the goals kernel.
// (The views, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_tree_dev.h"

namespace rrtdev {

template <bool LARGE>
__device__ __forceinline__ void keep_edge_body(const KeepView &kv) {
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = kv.j;
    for (int k = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); k < j; k += (int)gridDim.x * waves) {  // (k is wave-uniform)
        const int p = k == 0 ? 0 : kv.parent[k];
        bool ok = false;
        if (p >= 0 && p < j) {
            int cells;
            const uint32_t a = kv.nodes[p], b = kv.nodes[k];  // (k == 0: the walk root -> root is the root's cell)
            ok = LARGE ? los_wave_large(kv.og, kv.H, a, b, lane, cells) : los_wave(kv.og, kv.H, a, b, lane, cells);
        }
        if (lane == 0) {
            kv.ok[k] = ok ? (uint8_t)1 : (uint8_t)0;
            kv.anc[k] = (p >= 0 && p < j) ? p : k;
        }
    }
}

__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_edge_kernel(KeepView kv) {
    keep_edge_body<false>(kv);
}

// grids up to 4096 x 4096 (a batch created with RRT_FLAG_LARGE_GRID): the lines of sight by los_wave_large
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_edge_large_kernel(KeepView kv) {
    keep_edge_body<true>(kv);
}

__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_jump_kernel(const uint8_t *ok, const int32_t *anc, uint8_t *ok2, int32_t *anc2, int32_t j) {
    jump_round<false>(ok, anc, nullptr, ok2, anc2, nullptr, j);
}

// order-preserving compaction of the alive vertices by ONE workgroup of TPB threads
__global__ __launch_bounds__(TPB) void rrt_keep_compact_kernel(KeepCompact kc) {
    __shared__ uint32_t wcnt[2][NWAVE];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = kc.j;
    uint32_t carry = 0;
    int par = 0;
    for (int base = 0; base < j; base += TPB) {
        const int k = base + t;
        const bool live = k < j && kc.ok[k] != 0 && kc.anc[k] == 0;
        const unsigned long long m = __ballot(live);
        if (lane == 0) wcnt[par][wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) {
            const uint32_t s = wcnt[par][w];
            before += w < wave ? s : 0u;
            total += s;
        }
        par ^= 1;  // (the next pass writes the other half: no second barrier)
        if (k < j) kc.alive[k] = live ? (uint8_t)1 : (uint8_t)0;
        if (live) {
            const uint32_t dst = carry + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            kc.live_nodes[dst] = kc.nodes[k];
            kc.live_vcost[dst] = kc.vcost[k];
            kc.live_id[dst] = k;
        }
        carry += total;
    }
    if (t == 0) *kc.count = (int32_t)carry;
}

// the goals kernel answered in indices of the view: back to the original vertex numbers
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_remap_kernel(int32_t *vertex, const int32_t *live_id, int32_t m, int32_t count) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= m) return;
    const int v = vertex[g];
    vertex[g] = (v < 0 || v >= count) ? -1 : live_id[v];
}

}  // namespace rrtdev
