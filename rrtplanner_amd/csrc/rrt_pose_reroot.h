// rrt_pose_reroot.h -- re-root a finished DUBINS tree at one of its poses: the shortest-path tree from that pose over the directed
// graph of the tree's own poses.
//
// rrt_reroot.h reverses the parent pointers on the way from the new root to the old one, and a Dubins word is not reversible.  The
// goal needs no reversal: rrt_pose_relax.h builds the shortest-path tree from vertex 0, and from any other vertex it is the same
// computation with another root, costs that do not start as bounds the old tree guarantees, and vertices that may not be reached.
//
//   dense input   the input vertices with `root` moved to the front as number 0, the others in their order.  So relax_poses' tie rule
//                 (c[u], u) < (c[v], v) stays well-founded when another vertex duplicates the root's pose (a word of length 0).
//   edges         into v != 0: the u != v with d2(u, v) < R whose shortest word u -> v is finite and sweeps free, and the old parent
//                 edge, not swept again.  The new root has no edge into it; the old root has no old parent edge.  R = 0: old edges only.
//   costs         c[0] = 0, c[v] = min c[u] + len(u -> v) in f64: rrt_pose_relax.h's fixpoint.  The rounds start from 0 for the root,
//                 the sums of the old edges' words from the root down for what hangs below it in the old tree, and +inf elsewhere:
//                 every start value is +inf or the f64 sum along a path of edges from the root, so the monotone iteration reaches
//                 the least fixpoint.
//   cut           a vertex whose cost is +inf at the fixpoint.  The others get parents by relax_poses' rule, then rrt_reroot.h's
//                 numbering by (depth, previous number), the costs summed again from the root down, and the pose seed.
//
// The kernels, between the buckets of rrt_relax.h (scan, fill), the item kernel of rrt_pose_relax.h and the order of rrt_reroot.h:
//
//   1. rrt_pose_reroot_front_kernel   one input vertex per lane: its point, heading, renumbered parent and caller's number at its place
//                                     in the root-first order; its cell and the cell's count (rrt_relax_cell_kernel's part); cost = +inf.
//   2. the start: rrt_reroot_link_kernel over the OLD parents in the new numbers, the pointer jumping (jump_round, rrt_tree_dev.h) and
//      the order by depth of rrt_reroot.h mark and level the root's descendants, then
//      rrt_pose_reroot_start_kernel   reroot_cost_levels over plen[] (rrt_pose_relax_item_kernel evaluated each old edge's word): the
//                                     sums level by level, scattered to cost[] of the descendants.
//   3. rrt_pose_reroot_round_kernel, rrt_pose_reroot_parent_kernel   the round and the parent pass of rrt_pose_relax.h with OPEN set.
//   4. rrt_pose_reroot_check_kernel   behind the cost stage: every reached vertex was placed, and its cost summed from the root down
//                                     has the bits of the fixpoint's.
// Every index is checked before it is used; what cannot be placed raises err and is not stored.  No kernel waits for another workgroup.
// (The view and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_pose_relax.h"

namespace rrtdev {

// the number of input vertex k once `root` stands in front
__device__ __forceinline__ int pose_reroot_front(int k, int root) { return k == root ? 0 : k < root ? k + 1 : k; }

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_front_kernel(PoseRerootView fv, RelaxView xv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int j = fv.j, root = fv.root;
    if (k >= j || j != xv.j) return;
    if (root < 0 || root >= j) {  // (the host refuses such a root before it launches)
        atomicOr(xv.err, 1);
        return;
    }
    const int n = pose_reroot_front(k, root);
    // input vertex 0 is the old root, whatever parent[0] holds: it has no old parent edge; the new root's is dropped
    const int p = k == 0 || k == root ? -1 : fv.parent[k];
    if (k != 0 && k != root && (p < 0 || p >= j)) atomicOr(xv.err, 1);
    const uint32_t xy = fv.nodes[k];
    fv.f_nodes[n] = xy;
    fv.f_heading[n] = fv.heading[k];
    fv.f_parent[n] = p >= 0 && p < j ? pose_reroot_front(p, root) : -1;
    fv.f_id[n] = fv.id ? fv.id[k] : k;
    const int cell = relax_cell(xv, xy);
    if (cell < 0) atomicOr(xv.err, 1);
    xv.cell_of[n] = cell;
    xv.cost[n] = f64_inf();
    if (cell >= 0) atomicAdd(&xv.cell_fill[cell], 1);
}

// Behind rrt_reroot_parent_kernel over the old parents (rv: the root's descendants in the old tree placed by depth): their costs along
// the old edges, level by level, to cost[] in the numbers of the dense input.  One workgroup of TPB threads.
__global__ __launch_bounds__(TPB) void rrt_pose_reroot_start_kernel(RerootView rv, const double *plen, double *cost) {
    const int j = rv.j;
    reroot_cost_levels(rv, [&](int, int pos) {
        const int k = rv.src[pos];
        return k >= 0 && k < j ? plen[k] : f64_inf();
    });
    __syncthreads();
    const int count = rv.head[REROOT_COUNT];
    if (count < 1 || count > j || rv.head[REROOT_ERR] != 0) return;  // (uniform)
    for (int pos = (int)threadIdx.x; pos < count; pos += TPB) {
        const int k = rv.src[pos];
        if (k >= 0 && k < j && (pos == 0) == (k == 0)) cost[k] = pos == 0 ? 0.0 : rv.out_vcost[pos];
        else atomicOr(&rv.head[REROOT_ERR], 1);
    }
}

// the LDS of the two kernels below: the heading table and one list per wavefront, as the round and parent kernels of rrt_pose_relax.h have them
#define RRT_POSE_REROOT_LDS(ls, dc)                                                                                                 \
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];                                                                 \
    __shared__ double lc_lds[RELAX_TPB / 64][POSE_RELAX_LIST];                                                                      \
    __shared__ uint32_t lu_lds[RELAX_TPB / 64][POSE_RELAX_LIST];                                                                    \
    __shared__ uint32_t lp_lds[RELAX_TPB / 64][POSE_RELAX_LIST];                                                                    \
    __shared__ uint8_t lh_lds[RELAX_TPB / 64][POSE_RELAX_LIST];                                                                     \
    const int wave_ = ((int)threadIdx.x >> 6) & (RELAX_TPB / 64 - 1);                                                               \
    const PoseRelaxList ls{(volatile RRT_LDS double *)&lc_lds[wave_][0], (volatile RRT_LDS uint32_t *)&lu_lds[wave_][0],            \
                           (volatile RRT_LDS uint32_t *)&lp_lds[wave_][0], (volatile RRT_LDS uint8_t *)&lh_lds[wave_][0]}; /* of this wavefront alone */ \
    const DubCfg dc = dub_cfg_fill<RELAX_TPB>((RRT_LDS double *)htab_s, pv.rho, pv.nh, pv.W, pv.xv.H);                              \
    __syncthreads()

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_round_kernel(PoseRelaxView pv, const uint8_t *dirty_in, uint8_t *dirty_out, const uint8_t *changed_in,
                                                                          uint8_t *changed_out, int32_t first) {
    RRT_POSE_REROOT_LDS(ls, dc);
    pose_relax_round<true>(pv, dc, ls, dirty_in, dirty_out, changed_in, changed_out, first);
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_parent_kernel(PoseRelaxView pv) {
    RRT_POSE_REROOT_LDS(ls, dc);
    pose_relax_parents<true>(pv, dc, ls);
}
#undef RRT_POSE_REROOT_LDS

// rrt_relax_check_kernel over the reached vertices: as many were placed as the parent pass counted (RELAX_FELL), and the cost of every
// new number, summed from the root down, has the bits of the fixpoint's
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_check_kernel(RelaxView xv, const int32_t *src, const double *out_vcost, const int32_t *count) {
    const int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int n = *count;
    if (n < 1 || n > xv.j) {
        if (pos == 0) atomicOr(xv.err, 1);
        return;
    }
    if (pos == 0 && (unsigned long long)n != xv.stats[RELAX_FELL]) atomicOr(xv.err, 1);
    if (pos >= n) return;
    const int k = src[pos];
    if (k < 0 || k >= xv.j || __double_as_longlong(out_vcost[pos]) != __double_as_longlong(xv.cost[k])) atomicOr(xv.err, 1);
}

}  // namespace rrtdev
