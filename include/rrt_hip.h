/*
 * rrt_hip.h -- C ABI of the MI355X (gfx950) RRT / RRT* tree-expansion engine.
 *
 * The reference (rland93/rrtplanner) has no FFI: its boundary is the body of
 * RRTStandard.plan / RRTStar.plan / RRTStarInformed.plan (rrtplanner/rrt.py:386-447,
 * :466-556, :653-758).  This header is the boundary a maintainer binds instead of those
 * loops (INTEGRATION.md shows the ctypes stub).  Plain C: pointers and sizes only, no
 * torch / numpy types.  All functions return 0 (RRT_OK) or a positive "host action
 * needed" status or a negative error; no exception crosses the boundary.
 * rrt_last_error_string() describes the last failure.
 *
 * Threading: a ctx (and the batches made from it) is used by one host thread at a
 * time; distinct ctxs may be used by distinct host threads at the same time (each owns
 * a HIP stream).  They share the device: a launch sizes its teams of compute units by
 * what the launches in flight of the same process have left free (rrt_batch_team_info),
 * so concurrent batches slow each other down but never wait for CUs they cannot get.
 * Kernels of OTHER processes on the same GPU are not seen by that registry; there the
 * bounded hand-off wait (0.5 s, then one CU per query) remains the safety net.
 */
#ifndef RRT_HIP_H
#define RRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_OK 0
#define RRT_NEED_UNITBALL 1        /* Informed: query reached ellipse sampling (rrt.py:697) without unit-ball data */
#define RRT_E_ARG (-1)
#define RRT_E_GOAL_UNREACHABLE (-2) /* rrt.py:317-318 would index og[INT64_MIN,..]: no line of sight, j < n */
#define RRT_E_HIP (-3)
#define RRT_E_NOGRID (-4)
#define RRT_E_UNSUPPORTED (-5)     /* rrt_batch_create / rrt_plan: grid larger than 2048 x 2048 (4096 x 4096 with RRT_FLAG_LARGE_GRID) or n > 262143 (the
                                      expansion kernels' packed keys; such a planner runs host-driven over rrt_tree_query instead, slower, same results);
                                      RRT_FLAG_LARGE_GRID with a planner or flag it does not take; rrt_set_grid: more than 32767 cells per axis */
#define RRT_E_COMM (-6)            /* multi-GPU gather: librccl missing, no communicator, RCCL error, unequal slabs */
#define RRT_E_INTERNAL (-7)        /* rrt_batch_relax, rrt_batch_relax_poses: an iteration went past the bound that its own reasoning sets */

#define RRT_ALG_STANDARD 0 /* RRTStandard.plan     rrt.py:386 */
#define RRT_ALG_STAR 1     /* RRTStar.plan         rrt.py:466 */
#define RRT_ALG_INFORMED 2 /* RRTStarInformed.plan rrt.py:653 */
/* Dubins-vehicle planners (BASELINE.json configs[4]).  The reference only advertises them (README.md:12,18-19) and ships no
 * module: NO REFERENCE PARITY, semantics defined in include/rrt_dubins.h (state = cell + discrete heading, edge = shortest
 * Dubins word of turning radius rho, cost = its arc length, collision = its sampled sweep; nearest / within / accept /
 * choose-parent exactly as rrt.py:418-437 / :498-548).  Need a batch created with RRT_FLAG_DUBINS. */
#define RRT_ALG_DUBINS 3      /* parent = nearest */
#define RRT_ALG_DUBINS_STAR 4 /* choose parent within r_rewire */

#define RRT_FLAG_LOGS 1u   /* keep per-iteration logs (nearest, accept, ellipse cost, j) on the device */
#define RRT_FLAG_SERIAL 2u /* use the one-sample-per-iteration kernel instead of the 16-sample block kernel */
#define RRT_FLAG_NOTEAM 4u /* block kernel on ONE workgroup (CU) per query.  Default: a team of up to 64 CUs per query, the
                              largest for which all teams of the batch are resident on the device together */
#define RRT_FLAG_TEAM_FAULT 8u /* testing: one member of every team leaves at once; the hand-offs of the others time out
                                  and the batch must finish with one CU per query */
#define RRT_FLAG_NOPIPE 16u /* teams of 8 and more CUs: do not pipeline super-blocks (the commit of block s under the resolution
                              of block s + 1; RRTStandard / RRTStar only) */
#define RRT_FLAG_REWIRE 32u /* opt-in TRUE RRT* rewire with cost propagation -- NOT the reference's behaviour: its
                              rewire step never fires (rrt.py:532-536 prices the rewire with vcosts[vn] + d, never below vcosts[vn]).
                              Semantics: oracle/rrt_oracle.c; runs on the one-sample-per-iteration kernel.  Default off. */
#define RRT_FLAG_DUBINS 64u /* the batch runs Dubins queries (RRT_ALG_DUBINS / RRT_ALG_DUBINS_STAR) only, one CU per query: 16 samples per
                              round on per-node headings and cell records (rrt_dubins_block.h); with RRT_FLAG_SERIAL the
                              one-sample-per-iteration kernel, kept as a cross-check.  rrt_plan sets it by itself for such a query. */
#define RRT_FLAG_ONEBODY 128u /* pipelined teams of 8 and more workers, RRTStandard / RRTStar: committer and workers as ONE kernel
                                (rrt_expand_block_kernel) instead of rrt_block_commit_kernel (8 waves, 256 vector registers) next to
                                rrt_block_work_kernel on two streams of the context; kept as a cross-check, the results are the same */
#define RRT_FLAG_NOPIPE1 32768u /* one CU per query, RRTStandard / RRTStar: the 16-samples-per-pass block kernel instead of the barrier-free
                                  pipeline (rrt_pipe.h); kept as a cross-check, the results are the same */
#define RRT_FLAG_LARGE_GRID 65536u /* opt-in: grids up to 4096 x 4096 (default: 2048 x 2048).  RRTStandard / RRTStar only, ONE CU per query on
                                     rrt_pipe_large_kernel (rrt_pipe.h, LARGE: 25-bit squared distances), whatever the size of the grid or of
                                     the batch; no teams.  RRT_E_UNSUPPORTED together with RRT_ALG_INFORMED, the Dubins planners,
                                     RRT_FLAG_REWIRE, RRT_FLAG_DUBINS, RRT_FLAG_SERIAL or RRT_FLAG_NOPIPE1.  A query of 4096 x 4096 cells keeps
                                     268 MB of cell records on the device.  Should the pipeline stall (a bounded wait inside the kernel), the
                                     query ends with RRT_E_HIP: no other kernel takes such a grid. */
#define RRT_FLAG_TEAM_MAX(g) ((uint32_t)(g) << 8) /* cap the team size at g CUs per query (g = 2, 4, ... 64; 0 = no cap) */

typedef struct rrt_ctx rrt_ctx;
typedef struct rrt_batch rrt_batch;

/* One planning query == the arguments of plan() plus the planner's state that the loop
 * reads (rrt.py:51-85, :454-464, :563-577). */
typedef struct rrt_query {
    int32_t alg;            /* RRT_ALG_* */
    int32_t n;              /* self.n: attempted samples and node capacity (rrt.py:62) */
    int32_t xs[2];          /* xstart */
    int32_t xg[2];          /* xgoal */
    int64_t r2_rewire;      /* smallest integer R with (d2 < r_rewire*r_rewire) <=> (d2 < R)   (rrt.py:180) */
    int64_t goal_d2;        /* smallest integer G with (r2norm(d) < r_goal) <=> (d2 < G)      (rrt.py:744) */
    const int32_t *samples; /* host (n,2): free[rand_gen.choice(F)] for iteration i (rrt.py:240) */
    double C[4];            /* Informed: rotation_to_world_frame(xstart,xgoal), row-major (rrt.py:601-613) */
    /* Dubins planners only (ignored otherwise) */
    const int32_t *headings; /* host (n): heading index of sample i, 0 <= h < nh */
    double rho;              /* turning radius in cells, > 0 */
    int32_t nh;              /* number of discrete headings, 1 .. 256 */
    int32_t hs, hg;          /* heading index of the start / goal pose */
    int32_t pad_;
    /* optional: the same samples already packed, x | y << 16 per sample (n words).  When non-NULL it is used instead of
     * `samples` (which may then be NULL): a host that keeps its free cells packed saves the (n,2) int64 gather of rrt.py:240 */
    const uint32_t *samples_packed;
} rrt_query;

/* Result of one query: the arrays plan() hands to build_graph (rrt.py:334-369).
 * pts/vcost/parent are caller-allocated with n+1 rows; rows [0, rows) are written.
 * Optional logs (NULL to skip, need RRT_FLAG_LOGS) have n rows. */
typedef struct rrt_result {
    int32_t *pts;         /* (n+1,2) */
    double *vcost;        /* (n+1)   */
    int32_t *parent;      /* (n+1)   -1 = root / none */
    int32_t *nearest_log; /* (n) vnearest of iteration i */
    uint8_t *accept_log;  /* (n) 1 if iteration i inserted a node */
    double *cbest_log;    /* (n) ellipse cost c of iteration i (rrt.py:698-699), NaN when free-sampled */
    int32_t *j_log;       /* (n) j at the top of iteration i (key of self.ellipses, rrt.py:701) */
    int32_t status;       /* RRT_OK / RRT_NEED_UNITBALL / RRT_E_GOAL_UNREACHABLE */
    int32_t j;            /* tree nodes before go2goal */
    int32_t vgoal;        /* rrt.py:319 / :331 */
    int32_t found;        /* go2goal connected the goal */
    int32_t i_switch;     /* first iteration sampled from the ellipse (n if none) */
    int32_t rows;         /* len(points) after go2goal: j+1 live rows are valid; n+1 if found else n in the reference */
    int64_t sum_j;        /* statistics for the algorithmic-byte model */
    int64_t sum_cells_nn;
    int64_t sum_near;
    int64_t sum_cells_cand;
    int64_t n_los_cand;
    int64_t n_rewired;    /* RRT_FLAG_REWIRE: nodes re-parented / descendant costs recomputed (0 otherwise: rrt.py:536 is never true) */
    int64_t n_propagated;
    int32_t *head;        /* Dubins planners: (n+1) heading index of every node; NULL to skip */
    int64_t n_words;      /* Dubins planners: shortest-word evaluations the device made (0 otherwise) */
} rrt_result;

/* ---- context / grid -------------------------------------------------------------- */
int rrt_ctx_create(int32_t device_id, rrt_ctx **out);
int rrt_ctx_destroy(rrt_ctx *ctx); /* destroy the batches created on a context before the context itself */
const char *rrt_last_error_string(rrt_ctx *ctx); /* ctx may be NULL */
/* RRT.__init__ / set_og (rrt.py:64-65, :261-272): og_nonzero is (W,H) C-order, 1 = obstacle.  Up to 32767 cells per axis; the
 * expansion kernels (rrt_batch_*, rrt_plan*) take grids up to 2048 x 2048, with RRT_FLAG_LARGE_GRID up to 4096 x 4096; larger ones
 * serve rrt_tree_query and rrt_prim_collisionfree only. */
int rrt_set_grid(rrt_ctx *ctx, const uint8_t *og_nonzero, int32_t W, int32_t H);

/* Device-resident noise grids (counterpart of oggen.perlin_occupancygrid, oggen.py:7-45: fractal gradient noise, min-max
 * normalised over all frames, obstacle where value < thresh).  `octaves` lattices of unit gradients (host-drawn, seeded):
 * octave o has dims[3*o..3*o+2] = (nz, nx, ny) lattice points, cell edge cells[o] pixels and amplitude amps[o]; grads holds
 * the lattices back to back, 3 doubles per point.  All `frames` grids stay in HBM; frame 0 becomes the active grid.
 * og_out (optional, host, frames*W*H bytes) receives a copy (the host needs it for free = argwhere(og == 0)). */
int rrt_noise_grids(rrt_ctx *ctx, int32_t W, int32_t H, int32_t frames, float thresh, int32_t octaves, const int32_t *dims,
                    const double *cells, const double *amps, const double *grads, uint8_t *og_out);
/* make frame k of the resident noise grids the active grid (no upload; anim.py:92-93 style replanning) */
int rrt_select_frame(rrt_ctx *ctx, int32_t frame);
/* counts the calls that rewrote the context's grid storage (rrt_set_grid, rrt_noise_grids).  A caller that keeps frames
 * resident records it after rrt_noise_grids and compares before rrt_select_frame: a different value means the frames are gone. */
int rrt_grid_generation(rrt_ctx *ctx, uint64_t *generation);
/* wait for everything queued on the context's stream and on its device */
int rrt_ctx_sync(rrt_ctx *ctx);

/* ---- resident batches: Q independent queries on the ctx's grid ------------------------- */
int rrt_batch_create(rrt_ctx *ctx, int32_t Q, int32_t n_cap, uint32_t flags, rrt_batch **out);
int rrt_batch_destroy(rrt_batch *b);
int rrt_batch_set_query(rrt_batch *b, int32_t q, const rrt_query *query); /* uploads samples, arms query q */
/* Informed: unit-ball points (rrt.py:582-586) for iterations ub_offset .. ub_offset+count-1 */
int rrt_batch_set_unitball(rrt_batch *b, int32_t q, const double *unitball, int32_t count, int32_t ub_offset);
int rrt_batch_rearm(rrt_batch *b);  /* reset every query's tree, keep the uploaded inputs */
int rrt_batch_launch(rrt_batch *b); /* asynchronous on the ctx stream; runs / resumes every unfinished query */
int rrt_batch_sync(rrt_batch *b);
/* CUs working on each query (the team size chosen at rrt_batch_create) and how often a team hand-off timed out: such a launch
 * is continued once with one CU per query, the next launch uses the team again */
int rrt_batch_team(rrt_batch *b, int32_t *cus_per_query, int32_t *fallbacks);
/* out = {workers per query the batch was created with (the shape on an otherwise idle device), workers per query of the last
 * launch, launches continued with one CU per query after a hand-off timed out, launches that ran a SMALLER team because other
 * launches of this process held compute units of the device}.  The members of a team wait for each other, so all of them must be
 * resident at once: every launch claims its compute units in a per-device registry of the library and, when they are not all
 * free, takes the largest team that fits next to the launches in flight (rrt_batch_sync returns the claim). */
int rrt_batch_team_info(rrt_batch *b, int32_t out[4]);
/* 1 if the last launch ran the pipelined team kernel (one more CU per query, which only commits) */
int rrt_batch_pipelined(rrt_batch *b, int32_t *pipelined);
/* name of the expansion kernel the last launch ran (the one before it, for a batch not launched yet: the one it would run),
 * as rocprofv3 prints it: "rrt_expand_block_kernel<64, 1, true, false>"; buf receives at most len - 1 characters */
int rrt_batch_kernel_name(rrt_batch *b, char *buf, int32_t len);
int rrt_batch_elapsed_ms(rrt_batch *b, float *ms); /* HIP events around the last launch's kernels (incl. a launch that timed out) */
int rrt_batch_get_result(rrt_batch *b, int32_t q, rrt_result *out);
/* Connect m goals to the tree that query q left on the device, in one launch (rrt_goals_kernel): "plan once, route everywhere".
 * goals_xy is host (m,2).  Per goal the decision of go2goal (rrt.py:311-319) over the vertices [0, j) of the query -- rrt_result.j:
 * the tree BEFORE its own goal row; row j of a query whose go2goal succeeded is a copy of xgoal, not a vertex --
 *   cost[k] = vcost[k] + sqrt(d2(k, goal)) in f64, the vertices tried in stable (cost, index) order, the first one with a free line
 *   of sight to the goal wins:  vertex[g] = that vertex, cost[g] = its cost[k]
 * (for the query's own xgoal: parent[vgoal] and vcost[vgoal] of its result).  No vertex connects (every line blocked, or the goal on
 * an obstacle cell): vertex[g] = -1, cost[g] = +inf.  The reference's fall-backs for that case (vgoal = 0, the IndexError of
 * rrt.py:317-318) belong to plan() and are NOT reproduced: for unreachable goals this call is outside reference parity.
 * Synchronous on the context's stream; the batch is left as it was (rrt_batch_get_result, rrt_batch_rearm + rrt_batch_launch give
 * what they gave before).  m == 0: RRT_OK, nothing is launched.
 * RRT_E_ARG: NULL; q out of range; m < 0 or m > 2^20; a goal outside the grid; a query that has not finished (none set, not launched
 * or not synchronised, waiting for its unit-ball stream, failed); a context whose grid changed shape, or was rewritten
 * (rrt_grid_generation) or switched to another frame, since the query last ran.  RRT_E_UNSUPPORTED: a batch created with
 * RRT_FLAG_DUBINS.  The first call allocates scratch on the batch (at most 512 slabs of n_cap words and 128 MiB, at least one slab),
 * freed with the batch. */
int rrt_batch_connect_goals(rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, int32_t *vertex, double *cost);
/* The same for a batch created with RRT_FLAG_DUBINS (rrt_pose_goals_kernel): connect m goal POSES to the tree that query q left on
 * the device.  poses_xyh is host (m,3): cell and heading index, 0 <= h < the query's nh.  Per pose the decision the Dubins planners
 * take for their own goal pose, over the vertices [0, j), with the rho and nh of query q:
 *   c[k] = vcost[k] + the length of the shortest Dubins word from the pose of vertex k to the goal pose (include/rrt_dubins.h), the
 *   vertices tried in stable (c, index) order, the first one whose sweep is free -- every sample k * DUB_DS of the word inside the
 *   grid and on a free cell, the goal cell free -- wins:  vertex[g] = that vertex, cost[g] = its c[k]
 * (for the query's own goal pose: parent[vgoal] and vcost[vgoal] of its result when found).  Nothing connects, or the goal on an
 * obstacle cell: vertex[g] = -1, cost[g] = +inf; the fall-backs of plan() are not reproduced.  A query that ended with
 * RRT_E_GOAL_UNREACHABLE is accepted: its tree is complete.
 * Synchronous on the context's stream; the batch is left as it was.  m == 0: RRT_OK, nothing is launched.
 * RRT_E_ARG: NULL; q out of range; m < 0 or m > 2^20; a cell outside the grid; a heading outside [0, nh) of query q; a query that
 * has not finished; a context whose grid changed shape or was replaced since the query ran (the conditions of
 * rrt_batch_connect_goals).  RRT_E_UNSUPPORTED: a batch created without RRT_FLAG_DUBINS (rrt_batch_connect_goals is its call).
 * The first call allocates scratch on the batch (at most 512 slabs of n_cap words and 128 MiB, 25 bytes a goal), later calls grow
 * it, the batch frees it. */
int rrt_batch_connect_poses(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, int32_t *vertex, double *cost);
/* diagnostic: out[0] = Dubins words evaluated, out[1] = sweeps run, summed over the goals of the last successful
 * rrt_batch_connect_poses on this batch (per-goal counters the kernel writes).  RRT_E_ARG when there is none. */
int rrt_batch_connect_poses_counts(rrt_batch *b, int64_t out[2]);
/* Finished routes from the start to m goals over the tree that query q left on the device, in one call and without leaving the
 * device until the answer is read back (rrt_routes.h); optionally shortened by greedy line-of-sight shortcuts.
 *   vertex[g], cost[g]: exactly what rrt_batch_connect_goals gives (the same kernel decides them).
 *   vertex[g] == -1: the route of g has 0 rows and length[g] = +inf.
 *   Otherwise the raw route P is root = vertex 0, ..., vertex[g] along the parent pointers, then the goal: k rows (x, y, id), id the
 *   tree vertex, -1 for the goal row.
 *   flags & RRT_ROUTES_SHORTCUT: row 0 is emitted, and from the anchor a = 0, while a < k-1, the next row is the LARGEST b in
 *   (a, k-1] with b == a+1 or collisionfree(P[a], P[b]) -- the line walked from P[a] to P[b], start side to goal side (the walk of
 *   rrt.py:202-229 is not symmetric); then a = b.  "Largest visible", not "up to the first blocked one": the visible rows need not
 *   be contiguous.  b == a+1 is taken without a test (a tree edge, or the goal edge go2goal tested).
 *   length[g]: the f64 sum, left to right from the root, of sqrt((double)d2) over the legs that were emitted, d2 the exact integer
 *   squared distance.  Without shortcuts it can differ from cost[g] in the last bits (another order of summation; RRT* prices a
 *   vertex when it is inserted).
 *   offsets[0..m]: CSR offsets into the rows of all goals, in goal order; offsets[m] is the row count.
 * The rows stay on the batch: rrt_batch_routes_rows copies them out.  Refusals, and the batch afterwards, as for
 * rrt_batch_connect_goals (one validation serves both calls); RRT_E_ARG also for flags other than RRT_ROUTES_SHORTCUT and for goals
 * whose raw routes have more than 2^28 rows together (pass fewer goals per call).  m == 0: RRT_OK, offsets[0] = 0, nothing is launched.
 * The parent walks are bounded by j steps: one that is not at vertex 0 by then fails the whole call with RRT_E_HIP, before any row
 * is written.  The first call allocates scratch on the batch (32 bytes a goal, 20 bytes a raw row), later calls grow it, the batch
 * frees it.  Synchronous on the context's stream: it waits once for the row count (which sizes the rows) and once for the answer. */
#define RRT_ROUTES_SHORTCUT 0x1u
int rrt_batch_routes(rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                     int64_t *offsets);
/* The rows of the last rrt_batch_routes on this batch: xy is host (rows, 2) int32, id host int32[rows], rows == its offsets[m].
 * RRT_E_ARG: NULL (with rows > 0); no rrt_batch_routes on this batch yet, or its last one failed; rows differs from that call's
 * total; an rrt_batch_launch or rrt_batch_rearm since (the tree the rows belong to is being replaced). */
int rrt_batch_routes_rows(rrt_batch *b, int32_t *xy, int32_t *id, int64_t rows);
/* Keep the finished tree of query q when the map changed (rrt_keep.h): the context's CURRENT grid og' -- same shape as the batch's,
 * set by rrt_set_grid / rrt_noise_grids / rrt_select_frame since the query ran -- is adopted for query q, and the vertices that
 * still hang on the root through free edges become a view next to the tree:
 *   edge_ok[0] = the root's cell is free in og';  edge_ok[k] = collisionfree(og', nodes[parent[k]], nodes[k]) for k > 0, the line
 *   walked from the parent to the child;  alive[k] = edge_ok[k] and alive[parent[k]].
 * *n_alive = number of alive vertices; alive (host, j bytes, may be NULL) = the flags.  The tree arrays are not modified and no cost
 * changes: rrt_batch_get_result gives what it gave before.  Afterwards rrt_batch_connect_goals / rrt_batch_routes accept the new
 * grid for query q, take every line of sight on it and consider only the alive vertices, in stable (cost, original index) order;
 * the vertex numbers and route ids they return are the original ones.  No alive vertex (the root blocked): every goal answers
 * -1 / +inf with 0 rows.  Every call starts from the whole tree, it is not cumulative: keeping the tree for the original map again
 * restores every vertex.  Other queries of the batch stay refused until they are kept themselves.  rrt_batch_rearm,
 * rrt_batch_launch and rrt_batch_set_query (a new rrt_plan) drop the view.
 * The walk is not symmetric (rrt.py:202-229).  plan() tested the edges of a reference-mode tree from the parent's side, so on an
 * unchanged map all of its vertices stay alive; the rewire of RRT_FLAG_REWIRE tests child to parent, so on such a tree an edge may
 * be cut even on an unchanged map.  Only the parent-to-child direction is tested.
 * Synchronous on the context's stream.  RRT_E_ARG: NULL; q out of range; a query that has not finished; a context grid of another
 * shape than the batch's.  RRT_E_UNSUPPORTED: a batch created with RRT_FLAG_DUBINS.  Such a refusal changes nothing.  A call that
 * fails later (an allocation, a device error) drops a view query q had together with the grid that view was built for: the query
 * is then refused by the goals and routes calls until it is kept or launched again, never answered from its whole tree on a grid
 * that cut it.  An rrt_batch_set_query that is refused leaves the query and its view as they were.  The first call allocates
 * scratch on the batch (10 bytes a vertex of capacity, and 16 for each query that is kept), freed with the batch. */
int rrt_batch_keep_tree(rrt_batch *b, int32_t q, int32_t *n_alive, uint8_t *alive);
/* kernel time in ms of the three stages of the last successful rrt_batch_keep_tree (or rrt_batch_keep_pose_tree) on this batch, from
 * events on the stream: edge test, pointer jumping, compaction.  RRT_E_ARG when there is none (or its tree had no vertex). */
int rrt_batch_keep_tree_ms(rrt_batch *b, float ms[3]);
/* rrt_batch_keep_tree for a batch created with RRT_FLAG_DUBINS (rrt_pose_keep.h): the same call with a Dubins edge.  With
 * pose[k] = (nodes[k], heading[k]):
 *   edge_ok[0] = the root's cell is free in og';  edge_ok[k] = the sweep of the shortest word from pose[parent[k]] to pose[k] is free
 *   on og' for k > 0 (include/rrt_dubins.h: every sample k * DUB_DS inside the grid and on a free cell, then the child's cell);
 *   alive[k] = edge_ok[k] and alive[parent[k]].
 * That is the test plan() accepted the edge by, and the Dubins loop has no rewire: on an unchanged map every vertex stays alive.
 * Afterwards rrt_batch_connect_poses accepts the new grid for query q, sweeps on it, considers only the alive vertices (the view
 * carries their heading bytes) and answers in the original vertex numbers.  Everything else -- *n_alive, alive, no cost changes, the
 * tree arrays untouched, not cumulative, the other queries, what drops the view, what a failure half way leaves, the three stage
 * times of rrt_batch_keep_tree_ms -- is rrt_batch_keep_tree's.  RRT_E_ARG as there.  RRT_E_UNSUPPORTED: not a Dubins batch (its call
 * is rrt_batch_keep_tree).  The scratch: 10 bytes a vertex of capacity, and 17 for each query that is kept. */
int rrt_batch_keep_pose_tree(rrt_batch *b, int32_t q, int32_t *n_alive, uint8_t *alive);
/* Finished routes from the start pose to m goal poses over the Dubins tree that query q left on the device, and optionally the path
 * the vehicle drives along them, in one call (rrt_pose_routes.h).  rrt_batch_routes for a batch created with RRT_FLAG_DUBINS; the
 * shortcuts are a call of their own, rrt_batch_pose_shortcuts below.
 *   vertex[g], cost[g]: exactly what rrt_batch_connect_poses gives (the same kernel decides them; after rrt_batch_keep_pose_tree over
 *   the same view, in the original vertex numbers).
 *   vertex[g] == -1: the route of g has 0 rows, no points, and length[g] = +inf.
 *   Otherwise the route is root = vertex 0, ..., vertex[g] along the parent pointers, then the goal pose: k rows (x, y, h, id), id the
 *   tree vertex, -1 for the goal row.
 *   length[g]: the f64 sum, left to right from 0.0, of the lengths of the shortest Dubins words between consecutive rows.  The Dubins
 *   loop prices vcost[child] = vcost[parent] + len and never rewires: length[g] == cost[g] bit for bit.
 *   offsets[0..m]: CSR offsets into the rows of all goals, in goal order; offsets[m] is the row count.
 *   flags & RRT_POSE_ROUTES_POINTS: the points of the routes as well.  Per leg, row r to row r + 1, the samples k * DUB_DS,
 *   k = 0 .. floor(len / DUB_DS), of its word, in order: the f64 pair whose round-half-up is the cell the planner tested for that sample
 *   (include/rrt_dubins_points.h); behind the last leg one more point, the goal cell.  Sample 0 of a leg is its start pose exactly; the
 *   end pose of a leg is the next leg's sample 0 and is not repeated, except on a leg whose length is an exact multiple of DUB_DS,
 *   whose last sample is its end pose: that point appears twice.  point_offsets[0..m]: CSR offsets into the points of all goals;
 *   point_offsets[m] is the point count.  Without the flag point_offsets may be NULL and is not written.
 * The rows and points stay on the batch: rrt_batch_pose_routes_rows and rrt_batch_pose_routes_points copy them out.  Refusals, and
 * the batch afterwards, as for rrt_batch_connect_poses (one validation serves both calls; RRT_E_UNSUPPORTED for a batch created
 * without RRT_FLAG_DUBINS, whose call is rrt_batch_routes); RRT_E_ARG also for flags other than RRT_POSE_ROUTES_POINTS, for poses whose
 * routes have more than 2^24 rows or 2^27 points together (pass fewer poses per call).  m == 0: RRT_OK, offsets[0] = 0, nothing is
 * launched.  RRT_E_HIP, before any row is written: a parent walk that is not at vertex 0 after j steps; before any point is written:
 * a leg without a word or with a length that is not finite.  The first call allocates scratch on the batch (28 bytes a pose, 29 a
 * row; with points 176 more a row and 16 a point), later calls grow it, the batch frees it.  Synchronous on the context's stream: it
 * waits for the row count, for the answer and the point count, and with points for the points kernel. */
#define RRT_POSE_ROUTES_POINTS 0x1u
int rrt_batch_pose_routes(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                          int64_t *offsets, int64_t *point_offsets);
/* rrt_batch_pose_routes with shortcuts: the same arguments, validation, budgets (2^24 on the rows of the walks, 2^27 on the points of
 * the kept legs) and scratch, flags RRT_POSE_ROUTES_POINTS or 0.  Per goal with vertex[g] >= 0, over the rows P[0..k) that
 * rrt_batch_pose_routes gives: from the anchor a = 0 the next kept row is the LARGEST b in (a, k-1] with b == a + 1 (never tested) or
 * for which the shortest Dubins word from pose P[a] to pose P[b], swept from P[a] on the context's active grid as
 * rrt_batch_connect_poses sweeps (every sample k * DUB_DS inside the grid and on a free cell, then the end cell), is free; on from
 * a = b until a == k - 1.  The kept rows are a subsequence of the raw rows with their ids, the first row and the goal row (id -1)
 * always among them; both poses of a shortcut stay as they are, the legs between them become that one word.
 *   vertex[g], cost[g]: rrt_batch_connect_poses' answers, unchanged.  length[g]: the f64 sum, left to right from 0.0, of the kept
 *   legs' word lengths; the shortest word is never longer than the legs it replaces, so length[g] <= cost[g] up to rounding, and no
 *   longer equal.  offsets, point_offsets and the points: those of the kept rows and the kept legs' words, under the rules above;
 *   every point is a sample whose cell the shortcut kernel or the planner tested.
 * It adds 12 bytes a pose and 9 a row of scratch, and one more wait (for the number of kept rows).  Its refusals name it.  The rows and
 * points stay on the batch exactly as rrt_batch_pose_routes leaves its own: one pair of read-back calls serves both. */
int rrt_batch_pose_shortcuts(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                             int64_t *offsets, int64_t *point_offsets);
/* The rows of the last rrt_batch_pose_routes or rrt_batch_pose_shortcuts on this batch, whichever ran last: xyh is host (rows, 3)
 * int32, id host int32[rows], rows == its offsets[m].  RRT_E_ARG: NULL (with rows > 0); no such call on this batch yet, or the last
 * one failed; rows differs from that call's total; an rrt_batch_launch, rrt_batch_rearm, rrt_batch_keep_pose_tree since. */
int rrt_batch_pose_routes_rows(rrt_batch *b, int32_t *xyh, int32_t *id, int64_t rows);
/* The points of the last rrt_batch_pose_routes or rrt_batch_pose_shortcuts on this batch, if it ran with RRT_POSE_ROUTES_POINTS: xy
 * is host (points, 2) f64, points == its point_offsets[m].  RRT_E_ARG as for the rows, and when that call did not ask for points. */
int rrt_batch_pose_routes_points(rrt_batch *b, double *xy, int64_t points);
/* kernel time in ms of the stages of the last successful rrt_batch_pose_routes (m > 0) on this batch, from events on the stream: the
 * decision (the kernel of rrt_batch_connect_poses), depth and scan, rows + legs + lengths (+ the scan of the point counts), the points
 * kernel (0 without points).  RRT_E_ARG when there is none. */
int rrt_batch_pose_routes_ms(rrt_batch *b, float ms[4]);
/* ... and of the last successful rrt_batch_pose_shortcuts (m > 0), which rrt_batch_pose_routes_ms does not report: the decision, depth
 * and scan, rows + shortcuts + scan + pack, legs + lengths (+ the scan of the point counts), the points kernel (0 without points). */
int rrt_batch_pose_shortcuts_ms(rrt_batch *b, float ms[5]);
/* Grow the finished tree of query q with m more samples (rrt_seed.h): seed + arm, then rrt_batch_launch / rrt_batch_sync /
 * rrt_batch_get_result as after rrt_batch_set_query.  RRTStandard and RRTStar, the default cost, the reference's rewire.
 *   seed   the alive vertices of the query's view (rrt_batch_keep_tree), in their original order, become vertices 0 .. *j0-1 of a new
 *          tree; without a view the whole tree [0, j), *j0 = j.  Points and costs are copied bit for bit, parents renumbered (the
 *          root keeps -1).  old_id (host, *j0 int32, may be NULL; give it room for the query's n) = the original number of each.
 *   sampled = the cells of the seed vertices 1 .. *j0-1 and nothing else: xstart is never in it (rrt.py:407-413), the cell of a
 *          vertex that was cut can be sampled again; with nothing cut it is the set the query's own run left.
 *   loop   m iterations of rrt.py:418-437 / :498-548 on the context's CURRENT grid with j starting at *j0, samples_xy (host, (m, 2)
 *          int32) their samples; lowest index among equal distances, stable (cost, index) order.  j0 + m <= n (the query's own n)
 *          is required, so the capacity rule j != n never binds.
 *   goal   go2goal to the query's xgoal on the current grid, both fall-backs of the reference included (against the query's n).
 * Afterwards the batch holds an ordinary finished query of n samples on the current grid, in the new numbering and with no view:
 * rrt_batch_get_result (rows follow n; status, j, vgoal, found of the grown tree; the statistics count the m iterations alone),
 * the goals and routes calls, rrt_batch_keep_tree and a further rrt_batch_grow all work on it.  *log0 = the log row of the first of
 * the m iterations (RRT_FLAG_LOGS): rows [*log0, *log0 + m) hold the grow, the rows below it are those of earlier runs.  The m samples
 * replace rows [*j0, *j0 + m) of the query's sample buffer: an rrt_batch_rearm replays the buffer as it then stands.
 * The seed belongs to the grid of this call: rrt_batch_launch is refused with RRT_E_ARG, before anything is queued or dropped, while
 * a query is armed so and the context's grid is another one (rrt_set_grid, even of the same cells: a new generation; rrt_select_frame
 * to another frame); rrt_batch_rearm or an rrt_batch_set_query in its place lifts the refusal, the seeded frame selected again too.
 * The launch is an ordinary one: it drops the views of ALL queries of the batch, so the other queries that had one are refused by
 * the goals calls until they are kept again; finished queries are not run again, their results stay.  m == 0: the seed, then go2goal.
 * The call itself is synchronous on the context's stream.  RRT_E_ARG: NULL (b, j0, log0, or samples_xy with m > 0); q out of
 * range; a query that has not finished; m < 0 or *j0 + m > n; a sample outside the grid; a view without an alive vertex (the root is
 * blocked); a context grid of another shape, or one replaced since the query ran without an rrt_batch_keep_tree for it (the
 * validation of rrt_batch_connect_goals).  RRT_E_UNSUPPORTED: an Informed query; a batch created with RRT_FLAG_DUBINS,
 * RRT_FLAG_REWIRE or RRT_FLAG_LARGE_GRID.  Such a refusal changes nothing.  A call that fails later (an allocation, a device
 * error) leaves the query without a tree (as before any rrt_batch_set_query). */
int rrt_batch_grow(rrt_batch *b, int32_t q, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0);
/* kernel time in ms of the seed's stages of the last successful rrt_batch_grow on this batch, from events on the stream: ms[0]
 * renumbering and node slots, ms[1] the `sampled` bitmap, ms[2] the cell records; the first `count` (1 .. 3) are written.
 * RRT_E_ARG when there is none, or after a later rrt_batch_reroot or rrt_batch_relax (their seed's times are theirs to report): of
 * the three timing calls only the one of the last seed call that ran answers. */
int rrt_batch_grow_ms(rrt_batch *b, float *ms, int32_t count);
/* rrt_batch_grow for a batch created with RRT_FLAG_DUBINS (Dubins-RRT and Dubins-RRT*): samples_xyh holds m rows (x, y, h) of int32, a
 * cell and a heading index in [0, nh) of the query.  The seed is rrt_batch_grow's -- the alive vertices of the view that
 * rrt_batch_keep_pose_tree installed, else the whole tree -- and keeps every vertex's heading beside its point and cost; `sampled` is
 * keyed on the cell, as the Dubins loop keys it, so the cell of a cut vertex and the start's can be drawn again; the loop is the Dubins
 * planners' (nearest on (x, y), the shortest word nearest -> sample and its sweep, choose parent in ascending index with strict <), the
 * goal decision the one for the query's own goal pose.  Afterwards rrt_batch_connect_poses, rrt_batch_pose_routes,
 * rrt_batch_keep_pose_tree and a further rrt_batch_grow_poses work on the grown tree in its new numbering.  The stage times are
 * rrt_batch_grow_ms's (the heading bytes are part of ms[0]).  Refusals as rrt_batch_grow, and RRT_E_ARG for a heading outside
 * [0, nh); RRT_E_UNSUPPORTED for a batch created without RRT_FLAG_DUBINS (rrt_batch_grow is its call).  rrt_batch_grow keeps
 * refusing a Dubins batch. */
int rrt_batch_grow_poses(rrt_batch *b, int32_t q, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0);
/* Re-root the finished tree of query q at its vertex `root`, then rrt_batch_grow from the re-rooted tree (rrt_reroot.h): for a start
 * that moved along a route, whose rows carry vertex numbers.  RRTStandard and RRTStar, the default cost, the reference's rewire.
 *   input    the whole tree [0, j), or with a view (rrt_batch_keep_tree) its alive vertices; `root` is a number of the tree as
 *            rrt_batch_get_result gave it, and with a view it must be alive.
 *   parents  with p_0 = root, p_1 = parent[root], ..., p_d = 0: new_parent[p_{i+1}] = p_i, new_parent[root] = -1, every other vertex
 *            keeps its parent.
 *   edges    the line walk is not symmetric and a valid edge is walked from the parent to the child, so each of the d reversed edges
 *            is walked again on the context's CURRENT grid from its new parent to its new child.  The other edges stand tested on
 *            this grid.  A vertex is alive iff every edge on its new way to `root` holds: a blocked reversed edge cuts everything
 *            that hangs behind it, *j0 reports what is left, and the m samples can repair the gap.
 *   numbers  the alive vertices ordered by (depth below `root`, previous number): `root` is vertex 0 and every parent is below its
 *            child, also for root == 0.  old_id (host, *j0 int32, may be NULL; give it room for the query's n) = the number each
 *            had before the call.
 *   costs    cost[0] = 0, cost[k] = cost[parent[k]] + sqrt((double)d2) accumulated from the root down: the bits of the loop's own
 *            sum along the new path, not old cost - cost[root].
 *   then     rrt_batch_grow's seed from these arrays (`sampled` = the cells of vertices 1 .. *j0-1), its arming with the m samples,
 *            and everything rrt_batch_grow says about the launch, the logs, *log0 and the query afterwards.  The query's start
 *            becomes the cell of `root`: an rrt_batch_rearm + rrt_batch_launch plans from it.  m == 0: the plain re-root, then go2goal.
 * j + m <= n is required with the vertices the call starts from (the view's, else the tree's), before any is cut.  Refusals: all of
 * rrt_batch_grow's in its order (a batch created with RRT_FLAG_DUBINS: a Dubins word is not reversible), then RRT_E_ARG for `root`
 * outside [0, j) and for a `root` that is not alive in the view.  A refusal changes nothing; a call that fails later leaves the
 * query without a tree. */
int rrt_batch_reroot(rrt_batch *b, int32_t q, int32_t root, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0);
/* kernel time in ms of the stages of the last successful rrt_batch_reroot on this batch: ms[0] the path, ms[1] the reversed edges'
 * test, ms[2] alive and depth (pointer jumping), ms[3] the order, ms[4] the costs, then ms[5 .. 7] the seed's stages as
 * rrt_batch_grow_ms reports them; the first `count` (1 .. 8) are written.  RRT_E_ARG when there is none, or after a later rrt_batch_grow. */
int rrt_batch_reroot_ms(rrt_batch *b, float *ms, int32_t count);
/* Relax the finished tree of query q to the shortest-path tree from its root over the graph of its own vertices, then rrt_batch_grow
 * from it (rrt_relax.h): the vertices stay and every parent is chosen again -- the limit the rewire of RRT* approaches.  RRTStandard
 * and RRTStar, the default cost.
 *   input    the whole tree [0, j), or with a view (rrt_batch_keep_tree) its alive vertices.
 *   edges    E(v), v != 0: every u != v with d2(u, v) < r2 (integer d2; r2 as rrt_query.r2_rewire is formed) whose line u -> v is free
 *            on the context's CURRENT grid -- the walk is not symmetric and runs from the parent to the child --, and the old parent
 *            of v, which is not walked again (it stands tested on this grid) and may be longer than the radius.  No vertex is cut.
 *   costs    cost[0] = 0, cost[v] = min over u in E(v) of cost[u] + sqrt((double)d2(u, v)) in f64: the unique fixpoint, what Dijkstra
 *            from the root gives with these sums.
 *   parents  chosen over the final costs: the u in E(v) with cost[u] + d == cost[v] and (cost[u], u) < (cost[v], v), the smallest
 *            (cost[u], u) of them.
 *   then     the numbering of rrt_batch_reroot, by (depth, previous number), old_id as there, the costs summed from the root down
 *            (they must equal the fixpoint bit for bit: RRT_E_HIP otherwise), and rrt_batch_grow's seed, arming and launch with
 *            the m samples.  The query's start stays.  m == 0: the plain relaxation, then go2goal.
 * Refusals: all of rrt_batch_grow's in its order (a batch created with RRT_FLAG_DUBINS: the cost of a word depends on the headings
 * at its ends), then RRT_E_ARG for r2 <= 0.  A refusal changes nothing; a call that fails later leaves the query without a tree.
 * RRT_E_INTERNAL: the costs still fell after j rounds, which no shortest path needs. */
int rrt_batch_relax(rrt_batch *b, int32_t q, int64_t r2, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0);
/* time in ms on the stream of the stages of the last successful rrt_batch_relax on this batch: ms[0] the buckets, ms[1] the rounds (the
 * host's read of every round's count of changes included), ms[2] the parents, ms[3] alive and depth, ms[4] the order, ms[5] the costs,
 * then ms[6 .. 8] the seed's stages as rrt_batch_grow_ms reports them; the first `count` (1 .. 9) are written.  RRT_E_ARG when there is
 * none, or after a later rrt_batch_grow or rrt_batch_reroot. */
int rrt_batch_relax_ms(rrt_batch *b, float *ms, int32_t count);
/* of the same call: out[0] rounds run (the last one changed nothing), out[1] vertices whose cost fell, out[2] lines of sight walked,
 * out[3] candidate pairs priced (the last two depend on the order in which the rounds' wavefronts ran) */
int rrt_batch_relax_stats(rrt_batch *b, int64_t out[4]);
/* rrt_batch_relax for a batch created with RRT_FLAG_DUBINS (rrt_pose_relax.h): the finished Dubins tree of query q relaxed to the
 * shortest-path tree from its root over the directed graph of its own poses, then rrt_batch_grow_poses from it.  A vertex's pose
 * (x, y, h) is fixed and the shortest word u -> v is a function of the two poses alone, so every parent can be chosen again.
 *   input    the whole tree [0, j), or with a view (rrt_batch_keep_pose_tree) its alive vertices with their heading bytes.
 *   edges    E(v), v != 0: every u != v with d2(u, v) < r2 whose shortest Dubins word from pose u to pose v is finite and sweeps free
 *            on the context's current grid -- the sweep of rrt_batch_connect_poses and rrt_batch_keep_pose_tree: every sample inside the
 *            grid and on a free cell, then v's cell --, and the edge parent[v] -> v, which is not swept again and may be longer than
 *            the radius: no vertex is ever cut.
 *   costs    cost[0] = 0, cost[v] = min over u in E(v) of cost[u] + len(u -> v) in f64, the expansion loop's own sum.
 *   parents, then: as rrt_batch_relax, the costs summed again from the root down as cost[parent] + word (RRT_E_HIP unless they equal
 *            the fixpoint bit for bit), the headings gathered into the new order, rrt_batch_grow_poses' seed, arming and launch with
 *            the m pose samples (x, y, heading index).
 * Refusals: all of rrt_batch_grow_poses' in its order (a straight-line batch: use rrt_batch_relax), then RRT_E_ARG for r2 <= 0.
 * A refusal changes nothing; a call that fails later leaves the query without a tree.  RRT_E_INTERNAL as rrt_batch_relax. */
int rrt_batch_relax_poses(rrt_batch *b, int32_t q, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0);
/* as rrt_batch_relax_ms, of the last successful rrt_batch_relax_poses: the buckets (with the items' headings and the old parent edges'
 * lengths), the rounds, the parents, alive and depth, the order, the costs (words, then sums), then the seed's three stages */
int rrt_batch_relax_poses_ms(rrt_batch *b, float *ms, int32_t count);
/* of the same call: out[0] rounds run, out[1] vertices whose cost fell, out[2] sweeps run and out[3] words evaluated in the rounds (a
 * round meets a pair at most once; the parent pass is not counted; both depend on the order in which the rounds' wavefronts ran) */
int rrt_batch_relax_poses_stats(rrt_batch *b, int64_t out[4]);
/* diagnostic builds (-DRRT_STAMPS): shader cycles wave 0 of query q spent in scan / barrier / nearest+line of sight /
 * choose parent / insert / go2goal; zeros in the product build */
int rrt_batch_debug_cycles(rrt_batch *b, int32_t q, uint64_t out[38]); /* [0..5] phases, [6..37] per-wave owner-phase cycles */
/* device-resident result slab of the batch: [vcost f64 | nodes u32 (x | y<<16) | parent i32], each [Q][stride], then
 * {status, j, vgoal, found} i32 per query (filled by rrt_gather); stride = (bytes - 16 Q) / (16 Q) */
int rrt_batch_result_block(rrt_batch *b, void **dev_ptr, int64_t *bytes);

/* ---- multi-GPU: one process per GPU, query q on rank q mod world (no data-path collective), one all-gather of the result
 * slabs over RCCL / xGMI at the end of a batch.  The reference has no counterpart (single process).
 * librccl is opened on the first of these calls; the single-GPU path never loads it. ---- */
#define RRT_COMM_ID_BYTES 128
/* Optional, before the first rrt_comm_* call of the process: the collective library to open instead of librccl.so.1 -- any library
 * that exports ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather / ncclAllReduce / ncclGetErrorString with RCCL's
 * signatures.  tests/fake_rccl is one for ranks that share ONE GPU (RCCL itself refuses two ranks on a device), so that the
 * world > 1 path can run on a one-GPU box.  RRT_E_COMM once a library has been opened; path NULL = back to the default. */
int rrt_comm_use_library(const char *path);
/* rank 0: a fresh communicator id (ncclGetUniqueId); the host ships the bytes to the other ranks over any side channel */
int rrt_comm_unique_id(uint8_t id[RRT_COMM_ID_BYTES]);
/* collective over all `world` ranks (ncclCommInitRank on the context's device) */
int rrt_comm_init(rrt_ctx *ctx, int32_t rank, int32_t world, const uint8_t id[RRT_COMM_ID_BYTES]);
int rrt_comm_destroy(rrt_ctx *ctx);
/* vals[0..count) := reduction over all ranks (op 0 sum, 1 max, 2 min), count <= 64; synchronous: also the barrier */
int rrt_comm_allreduce_f64(rrt_ctx *ctx, double *vals, int32_t count, int32_t op);
/* ncclAllGather of the batch's result slab on the context's stream: rank r's slab lands at gathered_dev + r * bytes_per_rank on
 * every rank.  Every rank must bring a batch of the same Q and capacity: checked by a 16-byte all-reduce in front of EVERY gather
 * (RRT_E_COMM on all ranks when the sizes differ).  That check is host-synchronous (it is rrt_comm_allreduce_f64: also a barrier
 * of the ranks), so the call returns after all ranks have entered it; only the all-gather itself is left asynchronous on the
 * stream (rrt_ctx_sync / the next synchronous call waits for it). */
int rrt_gather(rrt_batch *b, void **gathered_dev, int64_t *bytes_per_rank);
/* after rrt_gather ON THIS BATCH (the slabs of another batch, even one of equal size, are refused): query q of rank `rank` from
 * the gathered slabs into caller-allocated host arrays.  On entry out->rows is the CAPACITY of pts / vcost / parent in rows (the
 * remote query's row count is only known from its slab: RRT_E_ARG when it exceeds the capacity, nothing is written then); on
 * return rows = rows written; status, j, vgoal, found are filled; logs and statistics are not gathered */
int rrt_gather_fetch(rrt_batch *b, int32_t rank, int32_t q, rrt_result *out);

/* ---- one-shot wrappers (what plan() binds) --------------------------------------------- */
int rrt_plan(rrt_ctx *ctx, const rrt_query *query, uint32_t flags, rrt_result *out);
int rrt_plan_resume(rrt_ctx *ctx, const double *unitball, int32_t count, rrt_result *out);
int rrt_plan_batch(rrt_ctx *ctx, int32_t Q, const rrt_query *queries, rrt_result *out);
/* rrt_batch_connect_goals on the tree of the context's last rrt_plan / rrt_plan_resume (the batch behind them stays resident) */
int rrt_plan_connect_goals(rrt_ctx *ctx, const int32_t *goals_xy, int32_t m, int32_t *vertex, double *cost);
/* rrt_batch_connect_poses on the tree of the context's last rrt_plan of a Dubins query (the batch behind it stays resident) */
int rrt_plan_connect_poses(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, int32_t *vertex, double *cost);
/* rrt_batch_routes / rrt_batch_routes_rows on the tree of the context's last rrt_plan / rrt_plan_resume */
int rrt_plan_routes(rrt_ctx *ctx, const int32_t *goals_xy, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length, int64_t *offsets);
int rrt_plan_routes_rows(rrt_ctx *ctx, int32_t *xy, int32_t *id, int64_t rows);
/* rrt_batch_keep_tree / rrt_batch_keep_tree_ms on the tree of the context's last rrt_plan / rrt_plan_resume */
int rrt_plan_keep_tree(rrt_ctx *ctx, int32_t *n_alive, uint8_t *alive);
int rrt_plan_keep_tree_ms(rrt_ctx *ctx, float ms[3]);
/* rrt_batch_keep_pose_tree on the Dubins tree of the context's last rrt_plan (its stage times: rrt_plan_keep_tree_ms) */
int rrt_plan_keep_pose_tree(rrt_ctx *ctx, int32_t *n_alive, uint8_t *alive);
/* rrt_batch_pose_routes and its companions on the Dubins tree of the context's last rrt_plan */
int rrt_plan_pose_routes(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                         int64_t *offsets, int64_t *point_offsets);
int rrt_plan_pose_routes_rows(rrt_ctx *ctx, int32_t *xyh, int32_t *id, int64_t rows);
int rrt_plan_pose_routes_points(rrt_ctx *ctx, double *xy, int64_t points);
int rrt_plan_pose_routes_ms(rrt_ctx *ctx, float ms[4]);
/* rrt_batch_pose_shortcuts and its stage times on the Dubins tree of the context's last rrt_plan; the rows and points are read back
 * by rrt_plan_pose_routes_rows / rrt_plan_pose_routes_points */
int rrt_plan_pose_shortcuts(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                            int64_t *offsets, int64_t *point_offsets);
int rrt_plan_pose_shortcuts_ms(rrt_ctx *ctx, float ms[5]);
/* *j = vertices of the finished tree of the context's last rrt_plan / rrt_plan_resume: the bytes rrt_plan_keep_tree writes into
 * `alive`.  RRT_E_ARG: NULL; no finished rrt_plan on this context. */
int rrt_plan_tree_size(rrt_ctx *ctx, int32_t *j);
/* rrt_batch_grow on the tree of the context's last rrt_plan / rrt_plan_resume, launch, sync and result included: returns like
 * rrt_plan (out as rrt_plan fills it, for the query's n).  rrt_plan_grow_ms: rrt_batch_grow_ms of that batch -- the companion
 * rrt_plan_keep_tree_ms is to rrt_plan_keep_tree: a caller of rrt_plan holds no rrt_batch to ask (RRT.grow, tools/grow_wall.py). */
int rrt_plan_grow(rrt_ctx *ctx, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
int rrt_plan_grow_ms(rrt_ctx *ctx, float *ms, int32_t count);
/* rrt_batch_grow_poses on the Dubins tree of the context's last rrt_plan, launch, sync and result included (out->head too);
 * rrt_plan_grow_ms gives its stage times. */
int rrt_plan_grow_poses(rrt_ctx *ctx, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
/* rrt_batch_reroot on the tree of the context's last rrt_plan / rrt_plan_resume, launch, sync and result included: returns like
 * rrt_plan_grow.  rrt_plan_reroot_ms: rrt_batch_reroot_ms of that batch. */
int rrt_plan_reroot(rrt_ctx *ctx, int32_t root, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
int rrt_plan_reroot_ms(rrt_ctx *ctx, float *ms, int32_t count);
/* rrt_batch_relax on the tree of the context's last rrt_plan / rrt_plan_resume, launch, sync and result included: returns like
 * rrt_plan_grow.  rrt_plan_relax_ms, rrt_plan_relax_stats: rrt_batch_relax_ms and rrt_batch_relax_stats of that batch. */
int rrt_plan_relax(rrt_ctx *ctx, int64_t r2, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
int rrt_plan_relax_ms(rrt_ctx *ctx, float *ms, int32_t count);
int rrt_plan_relax_stats(rrt_ctx *ctx, int64_t out[4]);
/* rrt_batch_relax_poses on the Dubins tree of the context's last rrt_plan, launch, sync and result (headings included) as
 * rrt_plan_grow_poses; rrt_plan_relax_poses_ms, rrt_plan_relax_poses_stats: those of that batch. */
int rrt_plan_relax_poses(rrt_ctx *ctx, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out);
int rrt_plan_relax_poses_ms(rrt_ctx *ctx, float *ms, int32_t count);
int rrt_plan_relax_poses_stats(rrt_ctx *ctx, int64_t out[4]);

/* ---- host-driven planners: a caller-supplied cost function (rrt.py:55, :70-80 accepts any Python callable) cannot run on the
 * device, so for such a planner the loop of rrt.py:498-548 / :690-748 stays on the host and asks the device, once per
 * iteration, for what it needs of the tree and the grid: near()[0], within() and the lines of sight of rrt.py:506, :519, :537.
 * The vertex list lives on the device (one 4-byte append per accepted sample). -------------------------------------------- */
typedef struct rrt_tree rrt_tree;
int rrt_tree_create(rrt_ctx *ctx, int32_t capacity, rrt_tree **out);
int rrt_tree_destroy(rrt_tree *t);
int rrt_tree_reset(rrt_tree *t); /* no vertices */
/* points[j] = (x, y) for the next free row j (rrt.py:411, :525); *index receives j.  Asynchronous. */
int rrt_tree_append(rrt_tree *t, int32_t x, int32_t y, int32_t *index);
/* One iteration's questions about sample (x, y), against the context's current grid:
 *   *nearest       near(points, x)[0] over the live rows, lowest index among equal distance          (rrt.py:503)
 *   *within_count  number of live rows with d2 < r2; within_idx[0 .. min(count, cap)) their indices, ascending (rrt.py:513)
 *   los_free[0]    collisionfree(og, points[nearest], x);  los_free[1 + k] = collisionfree(og, points[within_idx[k]], x)
 * los_free holds cap + 1 bytes.  RRT_E_ARG when the tree is empty or (x, y) lies outside the grid. */
int rrt_tree_query(rrt_tree *t, int32_t x, int32_t y, int64_t r2, int32_t *nearest, int32_t *within_count, int32_t *within_idx, uint8_t *los_free,
                   int32_t cap);

/* ---- primitives of the path (parity tests, micro-benchmarks) --------------------------- */
/* RRT.collisionfree (rrt.py:183-229) for m segments ab[k] = {ax,ay,bx,by}; cells = grid cells the
 * reference's walk reads before it returns. */
int rrt_prim_collisionfree(rrt_ctx *ctx, const int32_t *ab, int32_t m, uint8_t *out_free, int32_t *out_cells);
/* the same with the walk named: RRT_WALK_AUTO (what rrt_prim_collisionfree picks by the grid's size), RRT_WALK_U24 (grids up to
 * 2048 x 2048), RRT_WALK_U26 (the large-grid pipeline's, grids up to 4096 x 4096), RRT_WALK_WIDE (64-bit division, any grid).
 * RRT_E_UNSUPPORTED when the grid is larger than the walk takes. */
#define RRT_WALK_AUTO 0
#define RRT_WALK_U24 1
#define RRT_WALK_U26 2
#define RRT_WALK_WIDE 3
int rrt_prim_collisionfree_walk(rrt_ctx *ctx, const int32_t *ab, int32_t m, int32_t walk, uint8_t *out_free, int32_t *out_cells);
/* near()[0] (rrt.py:150-155,:422) and |within()| (rrt.py:176-181) of m query points against j nodes */
int rrt_prim_nearest_within(rrt_ctx *ctx, const int32_t *pts, int32_t j, const int32_t *xq, int32_t m,
                            int64_t r2, int32_t *out_nearest, int32_t *out_within_count,
                            int64_t *out_within_idxsum);
/* sqrt of the integers lo .. lo+count-1 as the kernels compute it (r2norm, rrt.py:24) */
int rrt_prim_sqrt_u32(rrt_ctx *ctx, uint32_t lo, uint32_t count, double *out);
/* the block kernel's short sqrt, valid for radicands below 2^24 */
int rrt_prim_sqrt_u24(rrt_ctx *ctx, uint32_t lo, uint32_t count, double *out);
/* the large-grid pipeline's, valid for radicands below 2^25 */
int rrt_prim_sqrt_u25(rrt_ctx *ctx, uint32_t lo, uint32_t count, double *out);
/* sqrt of arbitrary doubles as the kernels compute it (ellipse minor axis, rrt.py:622) */
int rrt_prim_sqrt_f64(rrt_ctx *ctx, const double *in, uint32_t count, double *out);

/* The moving start of a Dubins vehicle: the pose re-root calls.  They are part of this ABI and declared in a file of their own, which
 * rrtplanner_amd/moving.py binds: the signature table of rrtplanner_amd/_ffi.py lists what THIS file declares, name by name. */
#include "rrt_hip_moving.h"

#ifdef __cplusplus
}
#endif
#endif /* RRT_HIP_H */
