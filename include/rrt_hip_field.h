/*
 * rrt_hip_field.h -- the part of the C ABI that answers for the whole map: the cost-to-come field of a finished straight-line tree.
 * Include it behind rrt_hip.h, which declares the handles.  Bound by rrtplanner_amd/field.py.
 */
#ifndef RRT_HIP_FIELD_H
#define RRT_HIP_FIELD_H

#ifndef RRT_HIP_H
#error "include rrt_hip.h first: it declares the handles"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* For every cell of the window [x0, x0 + w) x [y0, y0 + h) of the context's current grid, what rrt_batch_connect_goals answers for that
 * one cell as a goal of query q (rrt_field.h): over the vertices k in [0, j), cost = vcost[k] + sqrt((double)d2(k, cell)) in f64, the
 * smallest (cost, k) among those whose line k -> cell is free, walked from the vertex to the cell.  A blocked cell, or a free one that no
 * vertex sees: vertex -1, cost +inf.  vertex and cost are (w, h) arrays, cell (x, y) at (x - x0) * h + (y - y0): the order of the grid.
 * After rrt_batch_keep_tree the field runs over the alive vertices on the new map and answers in the numbers of the tree the caller
 * holds; after a grow, a reroot or a relax, on the new tree.  The tree is not written.
 * Refusals: RRT_E_ARG for a NULL batch; RRT_E_UNSUPPORTED for a Dubins batch (its goal is a pose, and there is no field of poses here);
 * then rrt_batch_connect_goals' in its order (q, an unfinished query, a grid that changed shape or was replaced); then RRT_E_ARG for a
 * window with w < 1 or h < 1, for one that is not inside the grid, and for NULL outputs.  A refusal changes nothing. */
int rrt_batch_cost_field(rrt_batch *b, int32_t q, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t *vertex, double *cost);
/* time in ms on the stream of the stages of the last successful rrt_batch_cost_field on this batch: ms[0] the buckets, ms[1] the decision,
 * ms[2] the remap to the caller's numbers (0 without a kept view), ms[3] the copies to the host.  RRT_E_ARG when there is none. */
int rrt_batch_cost_field_ms(rrt_batch *b, float ms[4]);
/* of the same call: out[0] free cells decided, out[1] buckets visited, out[2] vertices priced, out[3] lines of sight walked */
int rrt_batch_cost_field_stats(rrt_batch *b, int64_t out[4]);
/* the same on the tree of the context's last rrt_plan */
int rrt_plan_cost_field(rrt_ctx *ctx, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t *vertex, double *cost);
int rrt_plan_cost_field_ms(rrt_ctx *ctx, float ms[4]);
int rrt_plan_cost_field_stats(rrt_ctx *ctx, int64_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* RRT_HIP_FIELD_H */
