/*
 * rrt_hip_pose_field.h -- the part of the C ABI that answers for the whole map of a Dubins planner: the pose cost field of a finished
 * Dubins tree.  Include it behind rrt_hip.h, which declares the handles.  Bound by rrtplanner_amd/posefield.py.
 */
#ifndef RRT_HIP_POSE_FIELD_H
#define RRT_HIP_POSE_FIELD_H

#ifndef RRT_HIP_H
#error "include rrt_hip.h first: it declares the handles"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* For every cell of the window [x0, x0 + w) x [y0, y0 + h) of the context's current grid, what rrt_batch_connect_poses answers for goal
 * poses on that one cell against the tree of query q (rrt_pose_field.h):
 *   heading in [0, nh)   the pose (x, y, heading): over the vertices k in [0, j), cost = vcost[k] + the length of the shortest Dubins word
 *                        from pose k to it, the smallest (cost, k) among those whose sweep is free.
 *   heading == -1        any arrival heading: over all pairs (heading a, vertex k) whose sweep is free, the smallest (cost, a, k) --
 *                        per heading the (cost, k)-first vertex, then the (cost, heading)-first heading.
 * vertex, cost and heading_out are (w, h) arrays, cell (x, y) at (x - x0) * h + (y - y0): the order of the grid.  heading_out holds the
 * arrival heading of the answer.  A blocked cell, or a free one that nothing reaches: vertex -1, cost +inf, heading_out -1
 * (rrt_batch_connect_poses has no heading output; the field writes -1 also when one heading was asked for).
 * After rrt_batch_keep_pose_tree the field runs over the alive vertices on the new map and answers in the numbers of the tree the
 * caller holds; after a grow_poses, a relax_poses or a reroot_poses, on the new tree.  The tree is not written.
 * Refusals: RRT_E_ARG for a NULL batch; RRT_E_UNSUPPORTED for a batch that is not a Dubins batch (use rrt_batch_cost_field); then
 * rrt_batch_connect_poses' in its order (q, an unfinished query, a grid that changed shape or was replaced); then RRT_E_ARG for a window
 * with w < 1 or h < 1, for one that is not inside the grid, for NULL outputs, and for a heading < -1 or >= the query's nh.  A refusal
 * changes nothing. */
int rrt_batch_pose_field(rrt_batch *b, int32_t q, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t heading, int32_t *vertex, double *cost,
                         int32_t *heading_out);
/* time in ms on the stream of the stages of the last successful rrt_batch_pose_field on this batch: ms[0] the buckets, ms[1] the decision,
 * ms[2] the remap to the caller's numbers (0 without a kept view), ms[3] the copies to the host.  RRT_E_ARG when there is none. */
int rrt_batch_pose_field_ms(rrt_batch *b, float ms[4]);
/* of the same call: out[0] free cells decided, out[1] buckets visited, out[2] words evaluated, out[3] sweeps run */
int rrt_batch_pose_field_stats(rrt_batch *b, int64_t out[4]);
/* the same on the tree of the context's last rrt_plan */
int rrt_plan_pose_field(rrt_ctx *ctx, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t heading, int32_t *vertex, double *cost, int32_t *heading_out);
int rrt_plan_pose_field_ms(rrt_ctx *ctx, float ms[4]);
int rrt_plan_pose_field_stats(rrt_ctx *ctx, int64_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* RRT_HIP_POSE_FIELD_H */
