// rrt_pose_keep.h -- keep a finished DUBINS tree when the map changes: which of its edges, Dubins words between poses, are still free.
//
// rrt_keep.h serves the straight-line planners; its semantics are this file's with another edge.  A finished Dubins query left nodes /
// heading / parent / vcost of its vertices [0, j) on the device, root 0, pose[k] = (nodes[k], heading[k]).  On a new map og' of the
// same shape
//
//   edge_ok[0] = the root's cell is free in og'
//   edge_ok[k] = the sweep of dub_between(pose[parent[k]], pose[k]) from the parent's pose is free on og'   for k > 0
//                (include/rrt_dubins.h: every sample k * DUB_DS inside the grid and on a free cell, then the child's cell;
//                 a parent outside [0, j) or the word DUB_NONE: not ok)
//   alive[k]   = edge_ok[k] and alive[parent[k]]
//
// plan() accepted every edge parent -> child by this very sweep of this very word (rrt_dubins_block.h, rrt_serial.h), and the Dubins
// loop has no rewire: on an unchanged map the view is the whole tree, with no exception.  What follows the edge test does not care
// what an edge is: rrt_keep_jump_kernel, rrt_keep_compact_kernel and rrt_keep_remap_kernel (rrt_keep.h) are used as they are, and the
// view gains one array, the heading byte of every alive vertex, which rrt_pose_goals_kernel then prices and sweeps from.
//
//   1. rrt_pose_keep_edge_kernel    NOT one wavefront per vertex: a word evaluation is some 2000 instructions, and 64 lanes would
//                                   compute the same word.  A wavefront takes 64 consecutive vertices a round, grid-stride, as a round
//                                   of pose_goal_bounded (rrt_pose_goals.h) does: every lane evaluates the word of ITS edge once
//                                   (dub_between_dev); then the wavefront sweeps the edges of the round one after the other
//                                   (dub_sweep_wave), word and poses handed from the edge's lane by dub_path_from_lane / readlane.  Every lane
//                                   keeps the answer of its own edge and writes ok[k] and anc[k] = parent[k] (anc[0] = 0, k itself for
//                                   a parent outside [0, j)) once, behind the round.  DubCfg and its heading table are dub_cfg_fill's
//                                   (rrt_dubins_dev.h): the words are the planner's bits.  Nothing waits across workgroups.
//                                   (Tree edges are short -- at most r_rewire --, so a sweep round of 128 samples is mostly empty lanes;
//                                   packing several edges into one round is left to a measurement: profiles/pose_keep_wall.json.)
//   2. rrt_pose_keep_gather_kernel  behind rrt_keep_compact_kernel, one alive vertex per lane: live_heading[i] = heading[live_id[i]]
//                                   for i < *count.
// (The view, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_dubins_dev.h"

namespace rrtdev {

__global__ __launch_bounds__(POSE_KEEP_TPB) void rrt_pose_keep_edge_kernel(PoseKeepView kv) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    RRT_LDS double *htab = (RRT_LDS double *)htab_s;
    const int t = (int)threadIdx.x, lane = t & 63;
    const DubCfg dc = dub_cfg_fill<POSE_KEEP_TPB>(htab, kv.rho, kv.nh, kv.W, kv.H);
    __syncthreads();
    const uint8_t *og = kv.og;
    const int j = kv.j;
    const int waves = (int)(blockDim.x >> 6);
    const int stride = (int)gridDim.x * waves * 64;
    for (int base = ((int)blockIdx.x * waves + (t >> 6)) * 64; base < j; base += stride) {  // (base is wave-uniform)
        const int k = base + lane;
        int p = -1, hp = 0;
        uint32_t np = 0, nk = 0;
        dub_path_t pth = dub_no_path();
        if (k < j) {
            p = k == 0 ? 0 : kv.parent[k];
            if (p >= 0 && p < j) {
                np = kv.nodes[p];
                hp = (int)kv.heading[p];
                nk = kv.nodes[k];
                if (k > 0) pth = dub_between_dev(np, hp, nk, (int)kv.heading[k], dc);
            } else {
                p = -1;
            }
        }
        // the root: its cell (no word: the word of a pose to itself may be a full turn)
        bool mine = k == 0 && p == 0 && og[(uint32_t)(ux(nk) * kv.H + uy(nk))] == 0;
        const int cnt = j - base < 64 ? j - base : 64;
        for (int l = 0; l < cnt; ++l) {  // (l is wave-uniform)
            const dub_path_t wp = dub_path_from_lane(pth, l);
            if (wp.word == DUB_NONE) continue;  // the root (decided above), a parent outside the tree, or no word: not ok
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)np, l), b = (uint32_t)__builtin_amdgcn_readlane((int)nk, l);
            const int ha = __builtin_amdgcn_readlane(hp, l);
            int cc = 0;
            const bool ok = dub_sweep_wave(og, dc, a, ha, b, wp, lane, cc);
            if (lane == l) mine = ok;
        }
        if (k < j) {
            kv.ok[k] = mine ? (uint8_t)1 : (uint8_t)0;
            kv.anc[k] = p >= 0 ? p : k;
        }
    }
}

// the heading bytes of the view, behind the compaction that wrote live_id and *count
__global__ __launch_bounds__(POSE_KEEP_TPB) void rrt_pose_keep_gather_kernel(const uint8_t *heading, const int32_t *live_id, const int32_t *count,
                                                                            uint8_t *live_heading, int32_t j) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= j || i >= *count) return;
    const int k = live_id[i];
    if (k >= 0 && k < j) live_heading[i] = heading[k];
}

}  // namespace rrtdev
