/*
 * rrt_hip_moving.h -- the part of the C ABI (rrt_hip.h, which includes this file at its end) that moves the start of a Dubins query:
 * re-root a finished Dubins tree at one of its poses.  Bound by rrtplanner_amd/moving.py.
 */
#ifndef RRT_HIP_MOVING_H
#define RRT_HIP_MOVING_H

#ifndef RRT_HIP_H
#error "include rrt_hip.h: it declares the handles and includes this file"
#endif

/* Re-root the finished Dubins tree of query q at its vertex `root`, then rrt_batch_grow_poses from the result (rrt_pose_reroot.h).
 * rrt_batch_reroot reverses parent pointers, and a Dubins word is not reversible; this call builds the shortest-path tree from the
 * root's pose over the directed graph of the tree's own poses instead, as rrt_batch_relax_poses builds it from vertex 0.
 *   input    the whole tree [0, j), or with a view (rrt_batch_keep_pose_tree) its alive vertices with their heading bytes.  `root` is
 *            a number of the tree as the caller holds it; with a view it must be alive.  The rules below speak in the numbers of the
 *            dense input with `root` moved to the front as number 0 and every other vertex in its order.
 *   edges    into v != 0: every u != v with d2(u, v) < r2 whose shortest Dubins word from pose u to pose v is finite and sweeps free on
 *            the context's current grid (the sweep of rrt_batch_connect_poses), and the old parent edge parent[v] -> v, which is not
 *            swept again and may be longer than the radius.  The new root has no edge into it, the old root no old parent edge.
 *            r2 == 0: the old edges alone, i.e. what hangs below `root` in the old tree.
 *   costs    cost[0] = 0, cost[v] = min cost[u] + len(u -> v) in f64, the least fixpoint.  The rounds start from 0 for the root, the
 *            sums of the old edges' words for its descendants in the old tree, and +inf for every other vertex.
 *   cut      the vertices whose cost is +inf at the fixpoint: nothing reaches them from the new root.
 *   parents  of the others, as rrt_batch_relax_poses chooses them: the smallest (cost[u], u) among the edges that give the vertex its
 *            cost, the old parent without a sweep.
 *   then     the numbering of rrt_batch_reroot by (depth, previous number), old_id as there (the caller's old numbers), the costs summed
 *            again from the root down (RRT_E_HIP unless they equal the fixpoint bit for bit), the pose seed, and rrt_batch_grow_poses'
 *            arming with the m pose samples (x, y, heading index).  The query's start becomes the root's pose, cell and heading: every
 *            pose tree call and a later rrt_batch_rearm + rrt_batch_launch work from it.
 * Refusals: all of rrt_batch_grow_poses' in its order (a straight-line batch: use rrt_batch_reroot), then RRT_E_UNSUPPORTED for a batch
 * beyond the capacity of the placement by depth, RRT_E_ARG for a root outside [0, j), for one that is not alive in the kept view, and for
 * r2 < 0, then the samples'.  A refusal changes nothing; a call that fails later leaves the query without a tree.  RRT_E_INTERNAL as
 * rrt_batch_relax. */
int rrt_batch_reroot_poses(rrt_batch *b, int32_t q, int32_t root, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id,
                           int32_t *log0);
/* time in ms on the stream of the stages of the last successful rrt_batch_reroot_poses on this batch: ms[0] the root-first input and the
 * buckets, ms[1] the start costs (the root's descendants and their sums), ms[2] the rounds, ms[3] the parents, ms[4] alive and depth,
 * ms[5] the order, ms[6] the costs, then ms[7 .. 9] the seed's stages as rrt_batch_grow_ms reports them; the first `count` (1 .. 10) are
 * written.  RRT_E_ARG when there is none, or after a later grow, reroot or relax call. */
int rrt_batch_reroot_poses_ms(rrt_batch *b, float *ms, int32_t count);
/* of the same call: out[0] rounds run (the last one changed nothing), out[1] vertices reached (the root among them), out[2] sweeps run
 * and out[3] words evaluated in the rounds (both depend on the order in which the rounds' wavefronts ran) */
int rrt_batch_reroot_poses_stats(rrt_batch *b, int64_t out[4]);
/* rrt_batch_reroot_poses on the Dubins tree of the context's last rrt_plan, launch, sync and result (headings included) as
 * rrt_plan_grow_poses; rrt_plan_reroot_poses_ms, rrt_plan_reroot_poses_stats: those of that batch. */
int rrt_plan_reroot_poses(rrt_ctx *ctx, int32_t root, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
int rrt_plan_reroot_poses_ms(rrt_ctx *ctx, float *ms, int32_t count);
int rrt_plan_reroot_poses_stats(rrt_ctx *ctx, int64_t out[4]);

#endif /* RRT_HIP_MOVING_H */
