// rrt_goals.h -- connect many goals to a finished tree: rrt_goals_kernel and its form for grids up to 4096 x 4096.
//
// go2goal (rrt.py:311-319) attaches ONE goal to a tree, inside the expansion kernels.  A tree grown from xstart serves every goal,
// so these kernels run the same decision for M goals against the tree a finished query left on the device:
//
//   cost[k] = vcost[k] + sqrt(d2(k, goal)) in f64 for the vertices k in [0, j) -- the tree before its own goal row: row j of a query
//   whose go2goal succeeded is a copy of xgoal, not a vertex -- tried in stable (cost, index) order; the first vertex with a free line
//   of sight to the goal wins.  No vertex connects (every line blocked, the goal on an obstacle cell, j == 0): vertex -1, cost +inf.
//   The reference's fall-backs for that case (vgoal = 0, the IndexError) belong to plan() and are not reproduced.
//
// One workgroup of TPB threads decides one goal at a time, goals g = blockIdx.x, blockIdx.x + gridDim.x, ..., by go2goal_phase
// (rrt_go2goal.h), the decision plan() itself takes; its `order` scratch is this workgroup's slab.
// (A first stage in front of it -- one pass for the (cost, index)-smallest vertex and one line of sight, the answer if that line is
// free -- was measured and lost: 17.4 ms against 15.9 ms per 4096 goals at bench scale, where the cheapest vertex sees one goal in
// eight.  profiles/goals_wall.json has both numbers, tools/archive/goals_first_stage.patch the code.)
// (The views, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_go2goal.h"

namespace rrtdev {

template <bool LARGE>
__device__ __forceinline__ void goals_body(const GoalsView &gv, RRT_LDS uint32_t *lds16k, BSlot *bslots) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint8_t *og = gv.og;
    const int H = gv.H, j = gv.j;
    const uint32_t *nodes = gv.nodes;
    const double *vcost = gv.vcost;
    uint32_t *order = gv.order + (size_t)blockIdx.x * (size_t)gv.slab_words;
    for (int g = (int)blockIdx.x; g < gv.m; g += (int)gridDim.x) {
        const uint32_t xg = gv.goals[g];
        double pc = f64_inf();
        uint32_t pi = NONE;
        // a goal on an obstacle cell: every walk ends on it, so no vertex sees it (uniform branch: the barriers inside are safe).
        // (j == 0 is only guarded: no query produces it, the start is always vertex 0)
        if (j > 0 && og[(uint32_t)ux(xg) * (uint32_t)H + (uint32_t)uy(xg)] == 0) {
            go2goal_phase<false, TPB, LARGE>(og, H, nodes, vcost, 0, 1, j, xg, order, lds16k, bslots, t, lane, wave, pc, pi);
        }
        if (t == 0) {
            gv.vertex[g] = pi == NONE ? -1 : (int32_t)pi;
            gv.cost[g] = pc;
        }
        __syncthreads();  // the next goal rewrites the slots and tables that slower waves may still be reading
    }
}

__global__ __launch_bounds__(TPB) void rrt_goals_kernel(GoalsView gv) {
    __shared__ __attribute__((aligned(16))) uint32_t lds16k[2 * G2G_NB];
    __shared__ __attribute__((aligned(16))) BSlot bslots[2 * NWAVE];
    goals_body<false>(gv, (RRT_LDS uint32_t *)lds16k, bslots);
}

// grids up to 4096 x 4096 (a batch created with RRT_FLAG_LARGE_GRID): the lines of sight by los_wave_large
__global__ __launch_bounds__(TPB) void rrt_goals_large_kernel(GoalsView gv) {
    __shared__ __attribute__((aligned(16))) uint32_t lds16k[2 * G2G_NB];
    __shared__ __attribute__((aligned(16))) BSlot bslots[2 * NWAVE];
    goals_body<true>(gv, (RRT_LDS uint32_t *)lds16k, bslots);
}

}  // namespace rrtdev
