// rrt_tree_calls.hip -- the calls of the C ABI that work on the tree a finished query left on the device, each as rrt_batch_X and
// rrt_plan_X.  Host code only: the kernels are launched through rrt_kernel_abi.h.  In this order:
//   what the calls share  the refusals (refuse_*), a query's tree and kept view (tree_ref), launches that several calls queue, the scratch
//                         of the goals calls (goal_scratch), the batch behind rrt_plan (plan_batch)
//   reading a tree        connect_goals (rrt_goals.h), connect_poses (rrt_pose_goals.h), keep_tree, keep_pose_tree (rrt_keep.h, rrt_pose_keep.h)
//   the seed calls        grow, grow_poses (rrt_seed.h, rrt_pose_seed.h), reroot (rrt_reroot.h), relax, relax_poses (rrt_relax.h, rrt_pose_relax.h),
//                         reroot_poses (rrt_pose_reroot.h).  Each replaces a query's tree and re-arms it: one record says which call it is
//                         (SeedCall), one place starts replacing the query (start_replacing), one arms it and makes the call the batch's last
//                         (seed_and_arm)
//   routes and the fields routes (rrt_routes.h), pose_routes, pose_shortcuts (rrt_pose_routes.h), cost_field (rrt_field.h), pose_field (rrt_pose_field.h; FieldCall)
//   the reports           every _ms and _stats call: one table row per family (Report), one reader for the times and one for the counters
#include "rrt_engine.h"
#include "rrt_hip_field.h"  // rrt_batch_cost_field and its forms: declared beside rrt_hip.h, not in it
#include "rrt_hip_pose_field.h"  // rrt_batch_pose_field and its forms: the same

// ---- the gate: a finished tree on the grid it belongs to ----
// Every call makes these in this order, after the refusals that are its own (NULL, the batch's flags).  0: not refused.
static int refuse_q(const char *who, rrt_batch *b, int32_t q) {
    return q < 0 || q >= b->Q ? fail(b->ctx, RRT_E_ARG, "%s: q=%d of %d", who, q, b->Q) : RRT_OK;
}

static int refuse_unfinished(const char *who, rrt_batch *b, int32_t q) {
    const int32_t status = b->h_desc[(size_t)q].status;
    if (status == ST_DONE || status == ST_UNREACHABLE) return RRT_OK;
    return fail(b->ctx, RRT_E_ARG, "%s: query %d has not finished (%s): its tree is not complete", who, q,
                status == ST_IDLE      ? "no query set"
                : status == ST_RUNNING ? "not launched, or launched and not synchronised"
                : status == ST_NEED_UB ? "it waits for its unit-ball stream"
                                       : "its launch failed");
}

// The grid's shape, then its generation.  how: what the call says happened to the shape; so: what a replaced grid means for the call,
// nullptr for the calls that adopt the new grid and so never ask (rrt_batch_keep_tree, rrt_batch_keep_pose_tree).
static int refuse_grid(const char *who, rrt_batch *b, int32_t q, const char *how = "changed shape since the batch was created",
                       const char *so = ": the tree belongs to the other grid") {
    rrt_ctx *ctx = b->ctx;
    if (!ctx->og || b->gridW != ctx->W || b->gridH != ctx->H)
        return fail(ctx, RRT_E_ARG, "%s: the context's grid %s (%dx%d)", who, how, b->gridW, b->gridH);
    if (so && (b->ran_gen[(size_t)q] != ctx->grid_gen || b->ran_og[(size_t)q] != ctx->og))
        return fail(ctx, RRT_E_ARG, "%s: the context's grid was replaced since query %d ran (grid generation %llu then, %llu now)%s", who, q,
                    (unsigned long long)b->ran_gen[(size_t)q], (unsigned long long)ctx->grid_gen, so);
    return RRT_OK;
}

// What the descriptor of a finished query reports, held against what the batch can hold before anything is sized by it: the vertices,
// and of a Dubins query (the caller says which) the turning radius and the headings.
static int refuse_vertex_count(const char *who, rrt_batch *b, int32_t q) {
    const int32_t j = b->h_desc[(size_t)q].j;
    return j < 0 || j > b->n_cap ? fail(b->ctx, RRT_E_HIP, "%s: query %d reports %d vertices, capacity %d", who, q, j, b->n_cap) : RRT_OK;
}

static int refuse_pose_desc(const char *who, rrt_batch *b, int32_t q) {
    const QDesc &d = b->h_desc[(size_t)q];
    return d.nh < 1 || d.nh > 256 || !(d.rho > 0.0) ? fail(b->ctx, RRT_E_HIP, "%s: query %d reports rho=%g, nh=%d", who, q, d.rho, d.nh) : RRT_OK;
}

// The window of a field call: its size, then its place inside the context's grid
struct FieldWindow {
    int32_t x0, y0, w, h;
};

static int refuse_window(const char *who, rrt_ctx *ctx, const FieldWindow &win) {
    if (win.w < 1 || win.h < 1) return fail(ctx, RRT_E_ARG, "%s: a window of %d x %d cells", who, win.w, win.h);
    if (win.x0 < 0 || win.y0 < 0 || win.x0 > ctx->W - win.w || win.y0 > ctx->H - win.h)
        return fail(ctx, RRT_E_ARG, "%s: the window (%d, %d) + %d x %d is not inside the %dx%d grid", who, win.x0, win.y0, win.w, win.h, ctx->W, ctx->H);
    return RRT_OK;
}

// rrt_batch_connect_goals and rrt_batch_connect_poses: q, the number of goals (`goals`: what the call names them), then the tree
static int refuse_goals_call(const char *who, rrt_batch *b, int32_t q, int32_t m, const char *goals) {
    if (const int rc = refuse_q(who, b, q)) return rc;
    if (m < 0 || m > GOALS_MAX) return fail(b->ctx, RRT_E_ARG, "%s: m=%d, at most %d %s per call", who, m, GOALS_MAX, goals);
    if (const int rc = refuse_unfinished(who, b, q)) return rc;
    return refuse_grid(who, b, q);
}

// ---- the tree of one query: its arrays in the batch's slab, and its kept view (rrt_keep.h) ----
struct TreeRef {
    uint32_t *nodes;  // [node_stride] each
    double *vcost;
    int32_t *parent;
    uint8_t *heading;     // (nullptr unless the batch is a Dubins batch)
    double *live_vcost;   // [n_cap] each: the alive vertices, dense and in the original order (nullptr before the query's first keep_tree)
    uint32_t *live_nodes;
    int32_t *live_id;     // ... and the original number of each
    uint8_t *live_heading;  // ... and its heading index (a Dubins batch; nullptr otherwise)
    int32_t kept;         // vertices of the view, at most the tree's j; -1: no view, the calls see the whole tree
};

static TreeRef tree_ref(rrt_batch *b, int32_t q) {
    const size_t at = (size_t)q * b->node_stride;
    TreeRef t{b->d_nodes + at, b->d_vcost + at, b->d_parent + at, b->d_heading ? b->d_heading + at : nullptr};
    if (b->keep[(size_t)q].p) {
        const KeepScratch k = b->keep[(size_t)q].carve<KeepScratch>(b->d_heading != nullptr);
        t.live_vcost = k.live_vcost;
        t.live_nodes = k.live_nodes;
        t.live_id = k.live_id;
        t.live_heading = k.live_heading;
    }
    t.kept = std::min(b->keep_alive[(size_t)q], b->h_desc[(size_t)q].j);
    return t;
}

// ---- launches that several calls queue ----
// the workgroups of `per` items each that cover `items`
static unsigned wgs(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

// The rounds of pointer jumping over j >= 1 vertices (jump_round, rrt_tree_dev.h): ceil(log2(max(j, 2))) of them, fixed from j -- nothing
// is read back to stop early --, ping-ponging two sets of buffers.  round(cur) queues one round from set cur to set cur ^ 1.  Returns
// the set that holds the result.
template <typename Round>
static int jump_rounds(int j, Round round) {
    int rounds = 1, cur = 0;
    while (((int64_t)1 << rounds) < (int64_t)j) ++rounds;
    for (int r = 0; r < rounds; ++r, cur ^= 1) round(cur);
    return cur;
}

// The parents of a kept view renumbered into sv.new_parent (rrt_seed_rank_kernel, rrt_seed_parent_kernel; sv: parent, j_old, j0, live_id,
// rank, new_parent, err).  sv.err is the caller's word: it clears it in front and reads it behind.
static int renumber_view_parents(rrt_ctx *ctx, const SeedView &sv) {
    HIPCHK(ctx, hipMemsetAsync(sv.rank, 0xff, (size_t)sv.j_old * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(rrt_seed_rank_kernel, dim3(wgs(sv.j0, SEED_TPB)), dim3(SEED_TPB), 0, ctx->stream, sv);
    hipLaunchKernelGGL(rrt_seed_parent_kernel, dim3(wgs(sv.j0, SEED_TPB)), dim3(SEED_TPB), 0, ctx->stream, sv);
    return RRT_OK;
}

// What a decision (goals_decide, poses_decide) runs over: the whole tree of query q, or, for a query that was kept on this grid
// (rrt_batch_keep_tree, rrt_batch_keep_pose_tree), the view of its alive vertices, dense and in the original order.  `launch` gets
// (nodes, vcost, heading, j) and launches the kernel, which answers in indices of what it was given; rrt_keep_remap_kernel then turns
// those of a view into the original ones.
template <typename Launch>
static void decide_over(rrt_batch *b, int32_t q, int32_t *vertex, int32_t m, Launch launch) {
    const TreeRef t = tree_ref(b, q);
    const bool view = t.kept >= 0;
    const int32_t j = view ? t.kept : b->h_desc[(size_t)q].j;
    launch(view ? t.live_nodes : t.nodes, view ? t.live_vcost : t.vcost, view ? t.live_heading : t.heading, j);
    if (view)
        hipLaunchKernelGGL(rrt_keep_remap_kernel, dim3(wgs(m, KEEP_TPB)), dim3(KEEP_TPB), 0, b->ctx->stream, vertex,
                           (const int32_t *)t.live_id, m, j);
}

// The m rows (x, y) or, with nh > 0, (x, y, heading index < nh) of a call, checked against the grid one after the other and then
// packed into the batch's staging buffers (stage: x | y << 16, stage8: the headings).  noun: what the call names a row.  A refusal
// leaves the staging buffers as they were.
static int stage_cells(const char *who, rrt_batch *b, int32_t q, const char *noun, const int32_t *rows, int32_t m, int nh) {
    rrt_ctx *ctx = b->ctx;
    const int W = ctx->W, H = ctx->H, row = nh > 0 ? 3 : 2;
    for (int k = 0; k < m; ++k) {
        const int x = rows[row * k], y = rows[row * k + 1];
        if (x < 0 || x >= W || y < 0 || y >= H) return fail(ctx, RRT_E_ARG, "%s: %s %d = (%d, %d) outside the %dx%d grid", who, noun, k, x, y, W, H);
        if (nh > 0 && (rows[row * k + 2] < 0 || rows[row * k + 2] >= nh))
            return fail(ctx, RRT_E_ARG, "%s: %s %d has heading %d, query %d has headings [0, %d)", who, noun, k, rows[row * k + 2], q, nh);
    }
    b->stage.resize((size_t)m);
    if (nh > 0) b->stage8.resize((size_t)m);
    for (int k = 0; k < m; ++k) {
        b->stage[(size_t)k] = ((uint32_t)rows[row * k] & 0xffffu) | ((uint32_t)rows[row * k + 1] << 16);
        if (nh > 0) b->stage8[(size_t)k] = (uint8_t)rows[row * k + 2];
    }
    return RRT_OK;
}

// ---- the scratch of the goals and poses calls ----
static_assert(POSES_MAX == GOALS_MAX && POSES_MAX_SLABS == GOALS_MAX_SLABS && POSES_SLAB_BUDGET == GOALS_SLAB_BUDGET,
              "rrt_batch_connect_goals and rrt_batch_connect_poses share the batch's scratch and its limits");

// Room for m goals (m >= 1): their packed cells, vertex and cost, and the order slabs.  One slab of n_cap words per workgroup, at most
// GOALS_MAX_SLABS of them and GOALS_SLAB_BUDGET bytes, never fewer than one nor more than goals: `slabs` is the grid of the launch.
static hipError_t goal_scratch(rrt_batch *b, int32_t m, int &slabs) {
    const size_t fit = GOALS_SLAB_BUDGET / ((size_t)b->n_cap * sizeof(uint32_t));
    slabs = (int)std::clamp<size_t>(fit, 1, std::min<size_t>(GOALS_MAX_SLABS, (size_t)m));
    hipError_t e = hipSetDevice(b->ctx->device);
    if (e == hipSuccess) e = b->goal_order.reserve(slabs, (size_t)slabs * (size_t)b->n_cap * sizeof(uint32_t));
    if (e == hipSuccess) e = b->goal_xy.reserve(m, (size_t)m * sizeof(uint32_t));
    if (e == hipSuccess) e = b->goal_vertex.reserve(m, (size_t)m * sizeof(int32_t));
    if (e == hipSuccess) e = b->goal_cost.reserve(m, (size_t)m * sizeof(double));
    return e;
}

// vertex and cost of the m goals the last kernel decided, to the caller; waits for the stream (also: the staging buffers are reused)
static int fetch_goal_answers(rrt_batch *b, int32_t m, int32_t *vertex, double *cost) {
    rrt_ctx *ctx = b->ctx;
    HIPCHK(ctx, hipMemcpyAsync(vertex, b->goal_vertex.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cost, b->goal_cost.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    return RRT_OK;
}

// ---- the batch behind rrt_plan ----
// nullptr: refused with RRT_E_ARG and the message recorded, for a NULL context, or for no batch, which `sentence` puts in the call's words
static rrt_batch *plan_batch(rrt_ctx *ctx, const char *who, const char *sentence) {
    if (!ctx) fail(nullptr, RRT_E_ARG, "%s: NULL", who);
    else if (!ctx->single) fail(ctx, RRT_E_ARG, "%s: %s", who, sentence);
    return ctx ? ctx->single : nullptr;
}
static const char NO_PLAN[] = "no rrt_plan on this context yet, or its batch is gone";
static const char NO_PLAN_NO_TREE[] = "query 0 has not finished (no rrt_plan on this context yet, or its batch is gone)";

// ---- many goals against a finished tree (rrt_goals.h) ----
// The part that rrt_batch_connect_goals and rrt_batch_routes share: every refusal, the goals packed and uploaded, the scratch of the
// first call, and the goals kernel launched on the context's stream.  Nothing is read back and nothing waited for: vertex and cost
// of the m goals are in b->goal_vertex / b->goal_cost once the stream gets there.  m == 0: RRT_OK, nothing launched.
static int goals_decide(const char *who, rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, bool null_out) {
    rrt_ctx *ctx = b->ctx;
    if (!goals_xy || null_out) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (b->flags & RRT_FLAG_DUBINS)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: a Dubins batch (an edge to a goal is a Dubins word to a goal pose; these kernels price straight lines)", who);
    if (const int rc = refuse_goals_call(who, b, q, m, "goals")) return rc;
    if (const int rc = stage_cells(who, b, q, "goal", goals_xy, m, 0)) return rc;
    if (m == 0) return RRT_OK;
    int slabs = 0;
    HIPCHK(ctx, goal_scratch(b, m, slabs));
    if (const int rc = refuse_vertex_count(who, b, q)) return rc;
    GoalsView gv{};
    gv.og = ctx->og;
    gv.H = ctx->H;
    gv.goals = b->goal_xy.as<uint32_t>();
    gv.m = m;
    gv.order = b->goal_order.as<uint32_t>();
    gv.slab_words = b->n_cap;
    gv.vertex = b->goal_vertex.as<int32_t>();
    gv.cost = b->goal_cost.as<double>();
    HIPCHK(ctx, hipMemcpyAsync(b->goal_xy.p, b->stage.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    decide_over(b, q, gv.vertex, m, [&](const uint32_t *nodes, const double *vcost, const uint8_t *, int32_t j) {
        gv.nodes = nodes;
        gv.vcost = vcost;
        gv.j = j;
        hipLaunchKernelGGL((b->flags & RRT_FLAG_LARGE_GRID) ? rrt_goals_large_kernel : rrt_goals_kernel, dim3((unsigned)slabs), dim3(TPB), 0, ctx->stream, gv);
    });
    HIPCHK(ctx, hipGetLastError());
    return RRT_OK;
}

static int connect_goals(const char *who, rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, int32_t *vertex, double *cost) {
    if (const int rc = goals_decide(who, b, q, goals_xy, m, !vertex || !cost); rc != RRT_OK || m == 0) return rc;
    return fetch_goal_answers(b, m, vertex, cost);
}

extern "C" int rrt_batch_connect_goals(rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, int32_t *vertex, double *cost) {
    return b ? connect_goals("rrt_batch_connect_goals", b, q, goals_xy, m, vertex, cost) : fail(nullptr, RRT_E_ARG, "rrt_batch_connect_goals: NULL");
}

extern "C" int rrt_plan_connect_goals(rrt_ctx *ctx, const int32_t *goals_xy, int32_t m, int32_t *vertex, double *cost) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_connect_goals", NO_PLAN_NO_TREE);
    return s ? connect_goals("rrt_plan_connect_goals", s, 0, goals_xy, m, vertex, cost) : RRT_E_ARG;
}

// ---- many goal poses against a finished Dubins tree (rrt_pose_goals.h) ----
// The conditions are goals_decide's, for a batch created with RRT_FLAG_DUBINS; a goal is a pose (x, y, h), h < the query's nh.
// The part that rrt_batch_connect_poses, rrt_batch_pose_routes and rrt_batch_pose_shortcuts share, as goals_decide serves the straight-line calls: every refusal
// (`use`: the call a straight-line batch is sent to), the poses packed and uploaded, the scratch, and the pose goals kernel launched
// on the context's stream.  Nothing is read back and nothing waited for.  m == 0: RRT_OK, nothing launched.  pose_last_m is left at -1
// (the counters are being rewritten) for the caller to set once its call has succeeded.
// time: nullptr, or the timer whose marks 0 and 1 to create if need be and to record around the upload and the kernel.
static int poses_decide(const char *who, rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, bool null_out, const char *use,
                        StageTimer *time = nullptr) {
    rrt_ctx *ctx = b->ctx;
    if (!poses_xyh || null_out) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (!(b->flags & RRT_FLAG_DUBINS))
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: not a Dubins batch (its goals are cells and its edges straight lines: use %s)", who, use);
    if (const int rc = refuse_goals_call(who, b, q, m, "goal poses")) return rc;
    const QDesc &d = b->h_desc[(size_t)q];
    if (const int rc = refuse_pose_desc(who, b, q)) return rc;
    if (const int rc = stage_cells(who, b, q, "goal", poses_xyh, m, d.nh)) return rc;
    if (const int rc = refuse_vertex_count(who, b, q)) return rc;
    b->pose_last_m = m == 0 ? 0 : -1;  // (-1 until this call has succeeded: the counters are being rewritten)
    if (m == 0) return RRT_OK;
    int slabs = 0;
    HIPCHK(ctx, goal_scratch(b, m, slabs));
    HIPCHK(ctx, b->pose_h.reserve(m, (size_t)m));
    HIPCHK(ctx, b->pose_counts.reserve(m, (size_t)m * 2 * sizeof(uint32_t)));
    PoseGoalsView pv{};
    pv.og = ctx->og;
    pv.W = ctx->W;
    pv.H = ctx->H;
    pv.nh = d.nh;
    pv.rho = d.rho;
    pv.goals = b->goal_xy.as<uint32_t>();
    pv.goal_h = b->pose_h.as<uint8_t>();
    pv.m = m;
    pv.slab_words = b->n_cap;
    pv.order = b->goal_order.as<uint32_t>();
    pv.vertex = b->goal_vertex.as<int32_t>();
    pv.cost = b->goal_cost.as<double>();
    pv.counts = b->pose_counts.as<uint32_t>();
    if (time) HIPCHK(ctx, time->create(2));
    if (time) HIPCHK(ctx, time->mark(0, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b->goal_xy.p, b->stage.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b->pose_h.p, b->stage8.data(), (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    decide_over(b, q, pv.vertex, m, [&](const uint32_t *nodes, const double *vcost, const uint8_t *heading, int32_t j) {
        pv.nodes = nodes;
        pv.vcost = vcost;
        pv.heading = heading;
        pv.j = j;
        hipLaunchKernelGGL(rrt_pose_goals_kernel, dim3((unsigned)slabs), dim3(TPB), 0, ctx->stream, pv);
    });
    if (time) HIPCHK(ctx, time->mark(1, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    return RRT_OK;
}

static int connect_poses(const char *who, rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, int32_t *vertex, double *cost) {
    if (const int rc = poses_decide(who, b, q, poses_xyh, m, !vertex || !cost, "rrt_batch_connect_goals"); rc != RRT_OK || m == 0) return rc;
    if (const int rc = fetch_goal_answers(b, m, vertex, cost)) return rc;
    b->pose_last_m = m;
    return RRT_OK;
}

extern "C" int rrt_batch_connect_poses(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, int32_t *vertex, double *cost) {
    return b ? connect_poses("rrt_batch_connect_poses", b, q, poses_xyh, m, vertex, cost) : fail(nullptr, RRT_E_ARG, "rrt_batch_connect_poses: NULL");
}

extern "C" int rrt_plan_connect_poses(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, int32_t *vertex, double *cost) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_connect_poses", NO_PLAN_NO_TREE);
    return s ? connect_poses("rrt_plan_connect_poses", s, 0, poses_xyh, m, vertex, cost) : RRT_E_ARG;
}

extern "C" int rrt_batch_connect_poses_counts(rrt_batch *b, int64_t out[2]) {
    if (!b || !out) return fail(nullptr, RRT_E_ARG, "rrt_batch_connect_poses_counts: NULL");
    rrt_ctx *ctx = b->ctx;
    if (b->pose_last_m < 0) return fail(ctx, RRT_E_ARG, "rrt_batch_connect_poses_counts: no rrt_batch_connect_poses on this batch yet, or its last one failed");
    out[0] = out[1] = 0;
    const size_t m = (size_t)b->pose_last_m;
    if (m == 0) return RRT_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    b->stage.resize(2 * m);
    HIPCHK(ctx, hipMemcpyAsync(b->stage.data(), b->pose_counts.p, 2 * m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    for (size_t k = 0; k < m; ++k) {
        out[0] += (int64_t)b->stage[2 * k];
        out[1] += (int64_t)b->stage[2 * k + 1];
    }
    return RRT_OK;
}

// ---- keep a finished tree when the map changes (rrt_keep.h; a Dubins tree: rrt_pose_keep.h) ----
// rrt_batch_keep_tree (poses == false: straight-line batches) and rrt_batch_keep_pose_tree (poses == true: Dubins batches) are one call
// with two edge tests; the Dubins view carries one more array, the heading bytes, gathered behind the compaction.
// Adopts the context's current grid for query q and installs the view of the vertices that still hang on the root through edges
// that are free on it.  Every call starts from the whole tree of the query.  A call refused for its arguments changes nothing.  Past
// that, a view the query had is dropped together with the grid it was built for (drop_keep_views), so a call that fails half way
// leaves a query that was kept before refused by goals_decide, never answered from the whole tree on a grid that cut it.
static int keep_tree(const char *who, rrt_batch *b, int32_t q, int32_t *n_alive, uint8_t *alive, bool poses) {
    rrt_ctx *ctx = b->ctx;
    if (!n_alive) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (!poses && (b->flags & RRT_FLAG_DUBINS))
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: a Dubins batch (its edges are Dubins words between poses; these kernels test straight lines)", who);
    if (poses && !(b->flags & RRT_FLAG_DUBINS))
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: not a Dubins batch (its edges are straight lines: use rrt_batch_keep_tree)", who);
    if (const int rc = refuse_q(who, b, q)) return rc;
    if (const int rc = refuse_unfinished(who, b, q)) return rc;
    if (const int rc = refuse_grid(who, b, q, "has another shape than the batch was created for", nullptr)) return rc;
    const QDesc &d = b->h_desc[(size_t)q];
    const int j = d.j;
    if (const int rc = refuse_vertex_count(who, b, q)) return rc;
    if (const int rc = poses ? refuse_pose_desc(who, b, q) : RRT_OK) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    drop_keep_views(b, q);
    StageTimer &time = b->keep_time;
    time.ran = 0;
    HIPCHK(ctx, b->keep_tmp.reserve<KeepTmpScratch>(b->n_cap));
    HIPCHK(ctx, b->keep[(size_t)q].reserve<KeepScratch>(b->n_cap, poses));  // (a batch is a Dubins batch or not for life)
    HIPCHK(ctx, time.create(4));
    const KeepTmpScratch tmp = b->keep_tmp.carve<KeepTmpScratch>();
    auto &anc = tmp.anc;
    auto &ok = tmp.ok;
    int32_t *d_count = tmp.count;
    int32_t count = 0;
    if (j > 0) {
        const TreeRef t = tree_ref(b, q);
        HIPCHK(ctx, time.mark(0, ctx->stream));
        if (poses) {  // one edge per lane, 64 a wavefront and round
            PoseKeepView kv{};
            kv.og = ctx->og;
            kv.W = ctx->W;
            kv.H = ctx->H;
            kv.nodes = t.nodes;
            kv.parent = t.parent;
            kv.heading = t.heading;
            kv.j = j;
            kv.nh = d.nh;
            kv.rho = d.rho;
            kv.ok = ok[0];
            kv.anc = anc[0];
            hipLaunchKernelGGL(rrt_pose_keep_edge_kernel, dim3(std::min<unsigned>(wgs(j, POSE_KEEP_TPB), POSE_KEEP_MAX_WG)), dim3(POSE_KEEP_TPB), 0, ctx->stream,
                               kv);
        } else {  // one edge per wavefront
            KeepView kv{};
            kv.og = ctx->og;
            kv.H = ctx->H;
            kv.nodes = t.nodes;
            kv.parent = t.parent;
            kv.vcost = t.vcost;
            kv.j = j;
            kv.ok = ok[0];
            kv.anc = anc[0];
            hipLaunchKernelGGL((b->flags & RRT_FLAG_LARGE_GRID) ? rrt_keep_edge_large_kernel : rrt_keep_edge_kernel,
                               dim3(std::min<unsigned>(wgs(j, KEEP_TPB / 64), KEEP_MAX_WG)), dim3(KEEP_TPB), 0, ctx->stream, kv);
        }
        HIPCHK(ctx, time.mark(1, ctx->stream));
        const int cur = jump_rounds(j, [&](int from) {
            hipLaunchKernelGGL(rrt_keep_jump_kernel, dim3(wgs(j, KEEP_TPB)), dim3(KEEP_TPB), 0, ctx->stream, (const uint8_t *)ok[from], (const int32_t *)anc[from],
                               ok[from ^ 1], anc[from ^ 1], j);
        });
        HIPCHK(ctx, time.mark(2, ctx->stream));
        KeepCompact kc{};
        kc.nodes = t.nodes;
        kc.vcost = t.vcost;
        kc.ok = ok[cur];
        kc.anc = anc[cur];
        kc.j = j;
        kc.alive = ok[cur ^ 1];
        kc.live_vcost = t.live_vcost;
        kc.live_nodes = t.live_nodes;
        kc.live_id = t.live_id;
        kc.count = d_count;
        hipLaunchKernelGGL(rrt_keep_compact_kernel, dim3(1), dim3(TPB), 0, ctx->stream, kc);
        if (poses)
            hipLaunchKernelGGL(rrt_pose_keep_gather_kernel, dim3(wgs(j, POSE_KEEP_TPB)), dim3(POSE_KEEP_TPB), 0, ctx->stream,
                               (const uint8_t *)t.heading, (const int32_t *)t.live_id, (const int32_t *)d_count, t.live_heading, j);
        HIPCHK(ctx, time.mark(3, ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
        if (alive) HIPCHK(ctx, hipMemcpyAsync(alive, kc.alive, (size_t)j, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, wait_stream_spin(ctx->stream));
        if (count < 0 || count > j) return fail(ctx, RRT_E_HIP, "%s: %d of %d vertices alive", who, count, j);
        time.ran = 3;
    }
    b->ran_gen[(size_t)q] = ctx->grid_gen;
    b->ran_og[(size_t)q] = ctx->og;
    b->keep_alive[(size_t)q] = count;
    b->drop_routes();  // the rows of an earlier routes call belong to another view
    *n_alive = count;
    return RRT_OK;
}

extern "C" int rrt_batch_keep_tree(rrt_batch *b, int32_t q, int32_t *n_alive, uint8_t *alive) {
    return b ? keep_tree("rrt_batch_keep_tree", b, q, n_alive, alive, false) : fail(nullptr, RRT_E_ARG, "rrt_batch_keep_tree: NULL");
}

extern "C" int rrt_plan_keep_tree(rrt_ctx *ctx, int32_t *n_alive, uint8_t *alive) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_keep_tree", NO_PLAN_NO_TREE);
    return s ? keep_tree("rrt_plan_keep_tree", s, 0, n_alive, alive, false) : RRT_E_ARG;
}

extern "C" int rrt_batch_keep_pose_tree(rrt_batch *b, int32_t q, int32_t *n_alive, uint8_t *alive) {
    return b ? keep_tree("rrt_batch_keep_pose_tree", b, q, n_alive, alive, true) : fail(nullptr, RRT_E_ARG, "rrt_batch_keep_pose_tree: NULL");
}

extern "C" int rrt_plan_keep_pose_tree(rrt_ctx *ctx, int32_t *n_alive, uint8_t *alive) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_keep_pose_tree", NO_PLAN_NO_TREE);
    return s ? keep_tree("rrt_plan_keep_pose_tree", s, 0, n_alive, alive, true) : RRT_E_ARG;
}

extern "C" int rrt_plan_tree_size(rrt_ctx *ctx, int32_t *j) {
    if (!ctx || !j) return fail(ctx, RRT_E_ARG, "rrt_plan_tree_size: NULL");
    rrt_batch *s = ctx->single;
    if (!s || (s->h_desc[0].status != ST_DONE && s->h_desc[0].status != ST_UNREACHABLE))
        return fail(ctx, RRT_E_ARG, "rrt_plan_tree_size: %s", NO_PLAN_NO_TREE);
    *j = s->h_desc[0].j;
    return RRT_OK;
}

// ---- grow a finished tree with new samples (rrt_seed.h) ----
// The seed kernels turn the finished tree of query q -- the view of its alive vertices, if it was kept on a new map -- into the loop
// state the expansion kernels resume from, and the descriptor is armed as a loop that stopped at iteration j0 of j0 + m:
//     D->n = j0 + m,  D->i = D->j = j0,  status RUNNING,  statistics zero,  the m samples at rows [j0, j0 + m) of the sample buffer.
// i != 0 keeps rrt_init_kernel away; every expansion kernel reads (i, j) from the descriptor and samples[i] by absolute row, and
// none of them depends on i == 0 or on i being a multiple of its block ("Growing a finished tree").  rrt_batch_sync puts
// the query's own n back (grow_n).  A refusal changes nothing; past the refusals a failure leaves the query idle.
// rrt_batch_grow (poses == false: straight-line batches, rows (x, y)) and rrt_batch_grow_poses (poses == true: Dubins batches, rows
// (x, y, h)) are one call: the Dubins seed carries one more array, the heading bytes (rrt_pose_seed.h), and the m sample headings go
// to rows [j0, j0 + m) of the sample heading buffer, which both Dubins kernels read by absolute row like the samples.
// What the seed calls share: the record of the call (SeedCall), the refusals (refuse_grow), where the query starts being replaced
// (start_replacing), what the seed is made from (SeedFrom), and the seed stages and the arming (seed_and_arm).

// One seed call, as its entry point fills it in once: every stage the seed calls share takes it.
struct SeedCall {
    const char *who;         // the entry point, as its messages name it
    SeedKind kind;           // what the batch's last_seed says once the call has succeeded
    rrt_batch *b;
    int32_t q;
    const int32_t *samples;  // m rows (x, y), of a pose call (x, y, heading index)
    int32_t m;
    int32_t *j0_out, *old_id, *log0;
    bool poses;              // a pose call: it takes a Dubins batch, and its seed carries the heading bytes
    rrt_ctx *ctx() const { return b->ctx; }
    QDesc &desc() const { return b->h_desc[(size_t)q]; }  // (once refuse_q has passed)
};

// Every refusal of a grow call up to the room, in its order; `dubins`: why this call takes no Dubins batch.  0: not refused, and
// j_in is what the call starts from: the vertices of the view, else of the tree.  use: the call a pose call sends a straight-line batch to.
static int refuse_grow(const SeedCall &c, const char *dubins, int &j_in, const char *use = "rrt_batch_grow") {
    const char *who = c.who;
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const int32_t q = c.q, m = c.m;
    const bool poses = c.poses;
    if (!c.j0_out || !c.log0 || (m > 0 && !c.samples)) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (!poses && (b->flags & RRT_FLAG_DUBINS)) return fail(ctx, RRT_E_UNSUPPORTED, "%s: a Dubins batch (%s)", who, dubins);
    if (poses && !(b->flags & RRT_FLAG_DUBINS))
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: not a Dubins batch (its samples are cells and its edges straight lines: use %s)", who, use);
    if (b->flags & RRT_FLAG_REWIRE)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: a batch created with RRT_FLAG_REWIRE (its kernel keeps child lists, which the seed does not rebuild)", who);
    if (b->flags & RRT_FLAG_LARGE_GRID)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: a batch created with RRT_FLAG_LARGE_GRID", who);
    if (const int rc = refuse_q(who, b, q)) return rc;
    if (const int rc = refuse_unfinished(who, b, q)) return rc;
    const QDesc &d = b->h_desc[(size_t)q];
    if (d.alg == RRT_ALG_INFORMED)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: query %d is an Informed RRT* query (its ellipse state is not rebuilt); RRTStandard and RRTStar only", who, q);
    if (const int rc = refuse_grid(who, b, q, "changed shape since the batch was created",
                                   poses ? " and the tree was not kept on it (rrt_batch_keep_pose_tree)" : " and the tree was not kept on it (rrt_batch_keep_tree)"))
        return rc;
    if (m < 0) return fail(ctx, RRT_E_ARG, "%s: m=%d", who, m);
    if (const int rc = poses ? refuse_pose_desc(who, b, q) : RRT_OK) return rc;
    const int j_old = d.j, own_n = d.n;
    if (j_old < 1 || j_old > b->n_cap || own_n < 1 || own_n > b->n_cap)
        return fail(ctx, RRT_E_HIP, "%s: query %d reports %d vertices of %d, capacity %d", who, q, j_old, own_n, b->n_cap);
    const int32_t kept = std::min(b->keep_alive[(size_t)q], j_old);
    if (kept == 0) return fail(ctx, RRT_E_ARG, "%s: no vertex of query %d is alive on this grid (the root is blocked): there is nothing to grow from", who, q);
    j_in = kept > 0 ? kept : j_old;
    if ((long long)j_in + m > own_n)
        return fail(ctx, RRT_E_ARG, "%s: %d vertices and m=%d samples exceed the query's n=%d: room for %d", who, j_in, m, own_n, own_n - j_in);
    return RRT_OK;
}

// The j0 vertices a seed is made from, dense.  All null: the query's own tree arrays [0, j0), which stay where they are.  Otherwise
// the arrays are copied in (rrt_seed_install_kernel); id: the number each had before; parent: its parent among the j0, or nullptr for
// a kept view, whose parents are those of the tree renumbered through id (rrt_seed_rank_kernel, rrt_seed_parent_kernel).
struct SeedFrom {
    const uint32_t *nodes = nullptr;
    const double *vcost = nullptr;
    const int32_t *id = nullptr;
    const int32_t *parent = nullptr;
    const uint8_t *heading = nullptr;  // (a Dubins batch)
    int32_t j0 = 0;
};

static SeedFrom seed_from_tree(const TreeRef &t, int32_t j_in) {
    SeedFrom from;
    if (t.kept > 0) {
        from.nodes = t.live_nodes;
        from.vcost = t.live_vcost;
        from.id = t.live_id;
        from.heading = t.live_heading;
    }
    from.j0 = j_in;
    return from;
}

// the refusal of reroot, relax and reroot_poses that the placement by depth forces (rrt_reroot.h)
static int refuse_capacity(const SeedCall &c) {
    if (c.b->n_cap <= REROOT_WAVES * REROOT_OWN) return RRT_OK;
    return fail(c.ctx(), RRT_E_UNSUPPORTED, "%s: a batch of capacity %d; the placement by depth takes trees of up to %d vertices", c.who, c.b->n_cap,
                REROOT_WAVES * REROOT_OWN);
}

// the samples of the call checked and staged (stage_cells): the last refusal that touches nothing of the batch
static int stage_samples(const SeedCall &c) { return stage_cells(c.who, c.b, c.q, "sample", c.samples, c.m, c.poses ? c.desc().nh : 0); }

// From here on the query is being replaced.  No seed call is the batch's last until this one has armed the query (seed_and_arm), so
// every report of a seed call is refused meanwhile and after a failure; the rows of an earlier routes call belong to the old tree;
// and the query is idle: a failure on the way leaves it without a tree.
static void start_replacing(const SeedCall &c) {
    c.b->last_seed = SeedKind::none;
    c.b->seed_time.ran = c.b->front_time.ran = 0;
    c.b->drop_routes();
    c.desc().status = ST_IDLE;
}

// The seed of query q from `from`, the m staged samples uploaded, and the descriptor armed at (j0, j0) of j0 + m.  The caller has
// made every refusal, staged the samples (stage_samples), reserved seed_tmp and the marks of seed_time, and started replacing the
// query (start_replacing): a failure leaves it idle without a tree.  A success makes the call the batch's last seed call.
static int seed_and_arm(const SeedCall &c, const SeedFrom &from) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const int32_t q = c.q, m = c.m;
    QDesc &d = c.desc();
    const int j_old = d.j, own_n = d.n, j0 = from.j0;
    const TreeRef t = tree_ref(b, q);
    const SeedTmpScratch tmp = b->seed_tmp.carve<SeedTmpScratch>();
    StageTimer &time = b->seed_time;
    SeedView sv{};
    sv.nodes = t.nodes;
    sv.vcost = t.vcost;
    sv.parent = t.parent;
    sv.j_old = j_old;
    sv.j0 = j0;
    sv.node_stride = b->node_stride;
    sv.rank = tmp.rank;
    sv.new_parent = from.parent ? const_cast<int32_t *>(from.parent) : tmp.new_parent;  // (only rrt_seed_parent_kernel writes it)
    sv.err = tmp.err;
    sv.bitmap = b->d_bitmap + (size_t)q * b->bitmap_words;
    sv.bitmap_words = b->bitmap_words;
    sv.H = ctx->H;
    sv.live_vcost = from.vcost;
    sv.live_nodes = from.nodes;
    sv.live_id = from.id;
    auto blocks = [](int items) { return dim3(wgs(items, SEED_TPB)); };
    HIPCHK(ctx, hipMemsetAsync(sv.err, 0, sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, time.mark(0, ctx->stream));
    if (sv.live_id && !from.parent)
        if (const int rc = renumber_view_parents(ctx, sv)) return rc;
    hipLaunchKernelGGL(rrt_seed_install_kernel, blocks(b->node_stride), dim3(SEED_TPB), 0, ctx->stream, sv);
    if (c.poses && sv.live_id)  // (without a view heading[0, j0) already stands; rrt_pose_seed.h says why the slots behind j0 are left)
        hipLaunchKernelGGL(rrt_pose_seed_heading_kernel, blocks(j0), dim3(SEED_TPB), 0, ctx->stream, t.heading, from.heading, j0, b->node_stride);
    HIPCHK(ctx, time.mark(1, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(sv.bitmap, 0, (size_t)b->bitmap_words * sizeof(uint32_t), ctx->stream));
    if (j0 > 1) hipLaunchKernelGGL(rrt_seed_bitmap_kernel, blocks(j0 - 1), dim3(SEED_TPB), 0, ctx->stream, sv);
    HIPCHK(ctx, time.mark(2, ctx->stream));
    if (b->d_cellcnt) {  // (a batch without cell records, RRT_FLAG_SERIAL: its kernel scans the node array)
        SeedRecords sr{};
        sr.nodes = sv.nodes;
        sr.vcost = sv.vcost;
        sr.j0 = j0;
        sr.cshift = d.cell_shift;
        sr.ncx = d.ncx;
        sr.ncy = d.ncy;
        sr.ccap = d.cell_cap;
        sr.rec_stride = b->rec_stride;
        sr.cellrec = reinterpret_cast<u32x4 *>(b->d_cellrec) + (size_t)q * (size_t)b->rec_stride;
        sr.cellcnt = b->d_cellcnt + (size_t)q * (size_t)MAX_CELLS;
        sr.err = sv.err;
        hipLaunchKernelGGL(rrt_seed_records_kernel, dim3(SEED_WG), dim3(SEED_TPB), 0, ctx->stream, sr);
    }
    HIPCHK(ctx, time.mark(3, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    int32_t err = 0;
    HIPCHK(ctx, hipMemcpyAsync(&err, sv.err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    if (c.old_id) {
        if (sv.live_id) HIPCHK(ctx, hipMemcpyAsync(c.old_id, sv.live_id, (size_t)j0 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        else
            for (int k = 0; k < j0; ++k) c.old_id[k] = k;
    }
    if (m > 0)
        HIPCHK(ctx, hipMemcpyAsync(b->d_samples + (size_t)q * b->n_cap + j0, b->stage.data(), (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (c.poses && m > 0)
        HIPCHK(ctx, hipMemcpyAsync(b->d_shead + (size_t)q * b->n_cap + j0, b->stage8.data(), (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    drop_keep_views(b, q);  // the view is used up: the tree arrays hold its vertices now
    if (err) {
        HIPCHK(ctx, hipMemcpyAsync(b->d_desc + q, &d, sizeof(QDesc), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, wait_stream_spin(ctx->stream));
        return fail(ctx, RRT_E_HIP, "%s: the tree of query %d on the device is not one the seed can place (a parent that is not alive, a vertex outside the "
                    "record grid or a cell past its capacity): the query is left without a tree", c.who, q);
    }
    arm_desc(d);
    d.n = j0 + m;
    d.i = d.j = j0;
    d.i_switch = own_n;
    b->grow_n[(size_t)q] = own_n;
    b->grow_gen[(size_t)q] = ctx->grid_gen;
    b->grow_og[(size_t)q] = ctx->og;
    HIPCHK(ctx, hipMemcpyAsync(b->d_desc + q, &d, sizeof(QDesc), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    time.ran = 3;
    b->last_seed = c.kind;
    *c.j0_out = j0;
    *c.log0 = j0;
    return RRT_OK;
}

static int batch_grow(const SeedCall &c) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    int j_in = 0;
    if (const int rc = refuse_grow(c, "the seed kernels carry no headings", j_in)) return rc;
    // (the last refusal: the staging buffers, written once every sample has passed, are the first thing of the batch this call touches)
    if (const int rc = stage_samples(c)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, b->seed_tmp.reserve<SeedTmpScratch>(b->n_cap));
    HIPCHK(ctx, b->seed_time.create(4));
    start_replacing(c);
    return seed_and_arm(c, seed_from_tree(tree_ref(b, c.q), j_in));
}

// ---- re-root a finished tree at one of its vertices (rrt_reroot.h) or relax it over its r-disc (rrt_relax.h), then the seed and the
// arming of grow ----
// What rrt_batch_reroot and rrt_batch_relax share comes in three parts: the dense input with a kept view (tree_input), the view of the
// scratch both work in and its reset (reroot_view, reroot_reset), and every stage from the pointer jumping to the armed descriptor
// (order_price_and_seed).

// The dense input of the call: the query's tree arrays, or, with a kept view, the view with its parents renumbered into the new_parent
// of seed_tmp (one wait: the view's err).  rv: og, H, nodes, parent, id, j.  vertex >= 0: a number of the tree as the caller holds it,
// whose number in the input goes to in_input (-1: not alive in the view).  heading: nullptr, or where the heading bytes of the input go
// (a Dubins batch).
static int tree_input(const SeedCall &c, const TreeRef &t, int32_t j_in, int32_t vertex, RerootView &rv, int32_t &in_input, const uint8_t **heading = nullptr) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const int32_t q = c.q;
    const char *who = c.who;
    const SeedTmpScratch stmp = b->seed_tmp.carve<SeedTmpScratch>();
    if (heading) *heading = t.kept > 0 ? t.live_heading : t.heading;
    rv.og = ctx->og;
    rv.H = ctx->H;
    rv.nodes = t.nodes;
    rv.parent = t.parent;
    rv.id = nullptr;
    rv.j = j_in;
    in_input = vertex;
    if (t.kept <= 0) return RRT_OK;
    SeedView sv{};
    sv.parent = t.parent;
    sv.j_old = b->h_desc[(size_t)q].j;
    sv.j0 = j_in;
    sv.live_id = t.live_id;
    sv.rank = stmp.rank;
    sv.new_parent = stmp.new_parent;
    sv.err = stmp.err;
    HIPCHK(ctx, hipMemsetAsync(sv.err, 0, sizeof(int32_t), ctx->stream));
    if (const int rc = renumber_view_parents(ctx, sv)) return rc;
    HIPCHK(ctx, hipGetLastError());
    int32_t err = 0;
    in_input = -1;
    HIPCHK(ctx, hipMemcpyAsync(&err, sv.err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    if (vertex >= 0) HIPCHK(ctx, hipMemcpyAsync(&in_input, sv.rank + vertex, sizeof in_input, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    if (err || in_input >= j_in)
        return fail(ctx, RRT_E_HIP, "%s: the kept view of query %d on the device is not a tree (a parent that is not alive)", who, q);
    rv.nodes = t.live_nodes;
    rv.parent = stmp.new_parent;
    rv.id = t.live_id;
    return RRT_OK;
}

static void reroot_view(RerootView &rv, const RerootScratch &tmp) {
    rv.path = tmp.path;
    rv.new_parent = tmp.new_parent;
    rv.ok = tmp.ok[0];
    rv.anc = tmp.anc[0];
    rv.dep = tmp.dep[0];
    rv.level_cnt = tmp.level_cnt;
    rv.level_start = tmp.level_start;
    rv.rank = tmp.rank;
    rv.src = tmp.src;
    rv.out_nodes = tmp.out_nodes;
    rv.out_vcost = tmp.out_vcost;
    rv.out_parent = tmp.out_parent;
    rv.out_id = tmp.out_id;
    rv.head = tmp.head;
}

// keep_err: the order is run a second time in one call (batch_reroot_poses), and what the first run raised stays raised
static int reroot_reset(rrt_ctx *ctx, const RerootView &rv, bool keep_err = false) {
    static const int32_t head0[REROOT_HEAD] = {0, 0, 0, 0, -1, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(rv.head, head0, keep_err ? REROOT_ERR * sizeof(int32_t) : sizeof head0, hipMemcpyHostToDevice, ctx->stream));
    if (keep_err)
        HIPCHK(ctx, hipMemcpyAsync(rv.head + REROOT_ERR + 1, head0 + REROOT_ERR + 1, (REROOT_HEAD - REROOT_ERR - 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                                   ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(rv.level_cnt, 0, ((size_t)rv.j + 1) * sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(rv.rank, 0xff, (size_t)rv.j * sizeof(int32_t), ctx->stream));
    return RRT_OK;
}

// a call that failed past its refusals leaves the query idle without a tree, on the device too
static int leave_without_tree(const SeedCall &c) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    drop_keep_views(b, c.q);
    HIPCHK(ctx, hipMemcpyAsync(b->d_desc + c.q, &c.desc(), sizeof(QDesc), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    return RRT_OK;
}

// the cost stage of a straight-line call: what batch_reroot and batch_relax hand to order_price_and_seed as `price`
static void price_lines(rrt_ctx *ctx, const RerootView &rv) { hipLaunchKernelGGL(rrt_reroot_cost_kernel, dim3(1), dim3(TPB), 0, ctx->stream, rv); }

// Behind rrt_reroot_link_kernel (ok, anc, dep of set 0 stand): alive and depth by pointer jumping, then the order by (depth, previous
// number) down to rrt_reroot_parent_kernel.  time: nullptr, or the timer whose mark `mark` goes between the two.
static int order_by_depth(rrt_ctx *ctx, RerootView &rv, const RerootScratch &tmp, StageTimer *time, int mark) {
    const int j = rv.j;
    auto blocks = [](int items) { return dim3(wgs(items, REROOT_TPB)); };
    const int cur = jump_rounds(j, [&](int from) {
        hipLaunchKernelGGL(rrt_reroot_jump_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, (const uint8_t *)tmp.ok[from], (const int32_t *)tmp.anc[from],
                           (const int32_t *)tmp.dep[from], tmp.ok[from ^ 1], tmp.anc[from ^ 1], tmp.dep[from ^ 1], j);
    });
    if (time) HIPCHK(ctx, time->mark(mark, ctx->stream));
    rv.key = tmp.dep[cur ^ 1];  // (the set the last round read: free from here on)
    hipLaunchKernelGGL(rrt_reroot_count_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, rv, (const uint8_t *)tmp.ok[cur], (const int32_t *)tmp.anc[cur],
                       (const int32_t *)tmp.dep[cur]);
    hipLaunchKernelGGL(rrt_reroot_level_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, rv);
    hipLaunchKernelGGL(rrt_reroot_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, rv);
    hipLaunchKernelGGL(rrt_reroot_place_kernel, dim3(REROOT_WG), dim3(REROOT_TPB), 0, ctx->stream, rv);
    hipLaunchKernelGGL(rrt_reroot_parent_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, rv);
    return RRT_OK;
}

// ... and of a pose call: the j words in parallel (and the headings into the new order, px.out_heading), then the sums level by level
static void price_words(rrt_ctx *ctx, const PoseRelaxView &pv, const RerootView &rv, const PoseRelaxScratch &px) {
    hipLaunchKernelGGL(rrt_pose_relax_word_kernel, dim3(wgs(rv.j, RELAX_TPB)), dim3(RELAX_TPB), 0, ctx->stream, pv, rv, px.out_heading, px.word);
    hipLaunchKernelGGL(rrt_pose_relax_cost_kernel, dim3(1), dim3(TPB), 0, ctx->stream, rv, (const double *)px.word);
}

// What order_price_and_seed is told beside the call.  The caller recorded mark `mark0` of front_time, and the call has mark0 + 3 stages
// in front of its seed.
struct OrderAndSeed {
    int mark0 = 0;
    bool whole = false;       // every input vertex has to be alive
    bool new_start = false;   // the descriptor's xs becomes the root's cell
    const char *what = "";    // the failure in the call's words
    const uint8_t *out_heading = nullptr;    // a pose call: the heading bytes in the new order, which `price` wrote
    const uint8_t *start_heading = nullptr;  // with new_start, a pose call: the host byte that `checks` has queued the new root's heading index into (the descriptor's hs becomes it)
};

// Behind rrt_reroot_link_kernel (rv.new_parent, ok, anc, dep of set 0 stand): alive and depth by pointer jumping, the order by (depth,
// previous number) (order_by_depth), the costs from the root down (`price` queues that stage) -- marks o.mark0 + 1 .. o.mark0 + 3 --,
// `checks` (what the call queues behind the costs), the one wait, then the seed and the arming.
template <typename Price, typename Checks>
static int order_price_and_seed(const SeedCall &c, RerootView &rv, const RerootScratch &tmp, const OrderAndSeed &o, Price price, Checks checks) {
    rrt_ctx *ctx = c.ctx();
    StageTimer &time = c.b->front_time;
    QDesc &d = c.desc();
    const int j = rv.j;
    if (const int rc = order_by_depth(ctx, rv, tmp, &time, o.mark0 + 1)) return rc;
    HIPCHK(ctx, time.mark(o.mark0 + 2, ctx->stream));
    price();
    HIPCHK(ctx, time.mark(o.mark0 + 3, ctx->stream));
    if (const int rc = checks()) return rc;
    HIPCHK(ctx, hipGetLastError());
    // the one wait that the sizes force: how many vertices are alive decides the launches of the seed
    int32_t head[REROOT_HEAD] = {0, 0, 1, 0, -1, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(head, rv.head, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    if (head[REROOT_ERR] || head[REROOT_COUNT] < 1 || head[REROOT_COUNT] > j || (o.whole && head[REROOT_COUNT] != j)) {
        if (const int rc = leave_without_tree(c)) return rc;
        return fail(ctx, RRT_E_HIP, "%s: %s: the query is left without a tree", c.who, o.what);
    }
    if (o.new_start) {
        d.xs[0] = (int32_t)((uint32_t)head[REROOT_XY] & 0xffffu);
        d.xs[1] = (int32_t)((uint32_t)head[REROOT_XY] >> 16);
        if (o.start_heading) d.hs = (int32_t)*o.start_heading;
    }
    SeedFrom from;
    from.nodes = tmp.out_nodes;
    from.vcost = tmp.out_vcost;
    from.id = tmp.out_id;
    from.parent = tmp.out_parent;
    from.heading = o.out_heading;
    from.j0 = head[REROOT_COUNT];
    if (const int rc = seed_and_arm(c, from)) return rc;
    time.ran = o.mark0 + 3;
    return RRT_OK;
}

// `root` is a vertex number of the tree as the caller holds it: with a kept view an original number, which must be alive.  The stages
// of rrt_reroot.h leave the re-rooted tree, renumbered by depth and repriced, in scratch; the seed installs it.  The descriptor's xs
// becomes the new root's cell.  A refusal changes nothing; past the refusals a failure leaves the query idle without a tree.
static int batch_reroot(const SeedCall &c, int32_t root) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const char *who = c.who;
    const int32_t q = c.q;
    int j_in = 0;
    if (const int rc = refuse_grow(c, "a Dubins word is not reversible", j_in)) return rc;
    QDesc &d = c.desc();
    if (root < 0 || root >= d.j) return fail(ctx, RRT_E_ARG, "%s: root=%d, query %d has the vertices [0, %d)", who, root, q, d.j);
    if (const int rc = refuse_capacity(c)) return rc;
    if (const int rc = stage_samples(c)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, b->seed_tmp.reserve<SeedTmpScratch>(b->n_cap));
    HIPCHK(ctx, b->reroot_tmp.reserve<RerootScratch>(b->n_cap));
    HIPCHK(ctx, b->seed_time.create(4));
    HIPCHK(ctx, b->front_time.create(6));
    const TreeRef t = tree_ref(b, q);
    const RerootScratch tmp = b->reroot_tmp.carve<RerootScratch>();
    auto blocks = [](int items) { return dim3(wgs(items, REROOT_TPB)); };
    RerootView rv{};
    // with a view the input is the view: its parents renumbered into scratch, and the root's number in it (-1: not alive)
    if (const int rc = tree_input(c, t, j_in, root, rv, rv.root)) return rc;
    if (rv.root < 0)
        return fail(ctx, RRT_E_ARG, "%s: root=%d is not alive in the kept view of query %d (%d of %d vertices alive)", who, root, q, j_in, d.j);
    reroot_view(rv, tmp);
    start_replacing(c);
    StageTimer &time = b->front_time;
    const int j = j_in;
    if (const int rc = reroot_reset(ctx, rv)) return rc;
    HIPCHK(ctx, time.mark(0, ctx->stream));
    hipLaunchKernelGGL(rrt_reroot_path_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, rv);
    HIPCHK(ctx, time.mark(1, ctx->stream));
    // one reversed edge per wavefront; how many there are only the device knows: at most j - 1
    hipLaunchKernelGGL(rrt_reroot_edge_kernel, dim3(std::clamp<unsigned>(wgs(j, REROOT_TPB / 64), 1, REROOT_MAX_WG)), dim3(REROOT_TPB), 0, ctx->stream, rv);
    hipLaunchKernelGGL(rrt_reroot_link_kernel, blocks(j), dim3(REROOT_TPB), 0, ctx->stream, rv);
    HIPCHK(ctx, time.mark(2, ctx->stream));
    char what[256];
    snprintf(what, sizeof what, "the parent array of query %d on the device is not a tree (a walk that did not reach vertex 0 within %d steps, or a "
             "vertex that cannot be placed)", q, j);
    OrderAndSeed o;
    o.mark0 = 2;
    o.new_start = true;
    o.what = what;
    return order_price_and_seed(c, rv, tmp, o, [&] { price_lines(ctx, rv); }, [] { return (int)RRT_OK; });
}

// ---- relax a finished tree to shortest paths over its r-disc (rrt_relax.h) ----
#ifndef RRT_RELAX_READ_EVERY
#define RRT_RELAX_READ_EVERY 1  // the host looks at the count of changes behind every round (DESIGN.md 4.2f3 measured 4 against it)
#endif
constexpr int RELAX_READ_EVERY = RRT_RELAX_READ_EVERY;
static_assert(RELAX_READ_EVERY >= 1, "rounds between two looks at the count of changes");

// The cells of the buckets for the threshold R on a W x H grid: the edge 2^shift with 2^(2 shift) >= R, so that d2 < R keeps u within
// one cell of v on either axis, doubled until the cells fit RELAX_MAX_CELLS.  (Coordinates are below 2^12 on every grid that is not
// refused, so shift 12 is one cell.)
static void relax_cells(int64_t R, int W, int H, RelaxView &xv) {
    int s = 0;
    while (s < 12 && ((int64_t)1 << (2 * s)) < R) ++s;
    auto across = [&](int cells_of) { return ((cells_of - 1) >> s) + 1; };
    while (s < 12 && (int64_t)across(W) * across(H) > RELAX_MAX_CELLS) ++s;
    xv.shift = s;
    xv.ncx = across(W);
    xv.ncy = across(H);
}

// The grid of a RelaxView with the buckets for the threshold R, and what the bucket kernels and the counters work in: the arrays that
// a RelaxScratch (the relax calls) and a FieldScratch (the field calls) both have.
template <typename Scratch>
static void bucket_view(rrt_ctx *ctx, RelaxView &xv, int64_t R, const Scratch &s) {
    xv.og = ctx->og;
    xv.H = ctx->H;
    relax_cells(R, ctx->W, ctx->H, xv);
    xv.cell_of = s.cell_of;
    xv.cell_start = s.cell_start;
    xv.cell_fill = s.cell_fill;
    xv.items = s.items;
    xv.item_xy = s.item_xy;
    xv.stats = s.stats;
}

// What batch_relax and batch_reroot_poses share of a RelaxView: the grid, the threshold R with its buckets (cells for max(R, 1): R = 0
// has no near pair, and one cell edge serves), and the arrays of the two scratch buffers.  nodes, parent, vcost and j are the call's.
static void relax_view(rrt_ctx *ctx, RelaxView &xv, int64_t R, const RelaxScratch &rx, const RerootScratch &tmp) {
    bucket_view(ctx, xv, std::max<int64_t>(R, 1), rx);
    xv.R = R;
    xv.pos_of = rx.pos_of;
    xv.cost = rx.cost;
    xv.new_parent = tmp.new_parent;
    xv.err = tmp.head + REROOT_ERR;
}

// ... and of a PoseRelaxView around it (heading is the call's)
static void pose_relax_view(rrt_ctx *ctx, PoseRelaxView &pv, const RelaxView &xv, const QDesc &d, const PoseRelaxScratch &px) {
    pv.xv = xv;
    pv.W = ctx->W;
    pv.nh = d.nh;
    pv.rho = d.rho;
    pv.item_h = px.item_h;
    pv.plen = px.plen;
}

// The rounds of both calls: round(in, first) queues one round that reads the flags of set `in` and writes those of the other.  The host
// reads the count of changes back behind every RELAX_READ_EVERY-th round and stops behind a look that saw none; a shortest path has
// fewer than j edges, so j rounds are the most.  rounds: how many ran.  Not settled by then: the query is left without a tree.
template <typename Round>
static int relax_rounds(const SeedCall &c, const RelaxView &xv, const RelaxScratch &rx, Round round, int64_t &rounds) {
    rrt_ctx *ctx = c.ctx();
    const int j = xv.j;
    const size_t cells = (size_t)xv.ncx * (size_t)xv.ncy;
    unsigned long long changes = 0, before = 0;
    bool settled = false;
    const int64_t most = (int64_t)j + 2 * (RELAX_READ_EVERY - 1);
    rounds = 0;
    while (!settled && rounds < most) {
        const int in = (int)(rounds & 1);
        HIPCHK(ctx, hipMemsetAsync(rx.dirty[in ^ 1], 0, cells, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(rx.changed[in ^ 1], 0, (size_t)j, ctx->stream));
        round(in, (int32_t)(rounds == 0));
        HIPCHK(ctx, hipGetLastError());
        if (++rounds % RELAX_READ_EVERY != 0 && rounds < most) continue;
        HIPCHK(ctx, hipMemcpyAsync(&changes, xv.stats + RELAX_CHANGES, sizeof changes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, wait_stream_spin(ctx->stream));
        settled = changes == before;  // (nothing changed since the last look: the last round changed nothing)
        before = changes;
    }
    if (settled) return RRT_OK;
    if (const int rc = leave_without_tree(c)) return rc;
    return fail(ctx, RRT_E_INTERNAL, "%s: the costs of query %d still fell in round %lld of a tree of %d vertices: the query is left without a tree", c.who, c.q,
                (long long)rounds, j);
}

// ---- what rrt_batch_relax and rrt_batch_reroot_poses both do around their own stages ----
// The scratch both calls work in beside seed_tmp: reserved, then carved (px: of a pose call).
static int reserve_relax_set(const SeedCall &c) {
    rrt_batch *b = c.b;
    HIPCHK(b->ctx, b->reroot_tmp.reserve<RerootScratch>(b->n_cap));
    HIPCHK(b->ctx, b->relax_tmp.reserve<RelaxScratch>(b->n_cap, (size_t)RELAX_MAX_CELLS));
    if (c.poses) HIPCHK(b->ctx, b->pose_relax_tmp.reserve<PoseRelaxScratch>(b->n_cap));
    return RRT_OK;
}

struct RelaxSet {
    const RerootScratch tmp;
    const RelaxScratch rx;
    const PoseRelaxScratch px;
    explicit RelaxSet(const SeedCall &c)
        : tmp(c.b->reroot_tmp.carve<RerootScratch>()), rx(c.b->relax_tmp.carve<RelaxScratch>((size_t)RELAX_MAX_CELLS)),
          px(c.poses ? c.b->pose_relax_tmp.carve<PoseRelaxScratch>() : PoseRelaxScratch(nullptr, 0)) {}
};

// In front of the buckets: the re-root scratch reset, the counters and the cells' fill counts zeroed, every vertex alive (no edge is cut)
static int reset_for_buckets(rrt_ctx *ctx, const RerootView &rv, const RelaxView &xv) {
    if (const int rc = reroot_reset(ctx, rv)) return rc;
    HIPCHK(ctx, hipMemsetAsync(xv.stats, 0, RELAX_STATS * sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(xv.cell_fill, 0, (size_t)xv.ncx * (size_t)xv.ncy * sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(rv.ok, 1, (size_t)rv.j, ctx->stream));
    return RRT_OK;
}

// The buckets of xv filled (rrt_batch_cost_field fills its own with these too): `first`, the kernel that says which cell each vertex
// lies in and counts the cells (rrt_relax_cell_kernel, or rrt_pose_reroot_front_kernel, which writes the root-first input on the way),
// then the scan of the counts and the fill.
template <typename... Args>
static void fill_buckets(rrt_ctx *ctx, const RelaxView &xv, void (*first)(Args...), Args... args) {
    const dim3 per_vertex(wgs(xv.j, RELAX_TPB));
    hipLaunchKernelGGL(first, per_vertex, dim3(RELAX_TPB), 0, ctx->stream, args...);
    hipLaunchKernelGGL(rrt_relax_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, xv);
    hipLaunchKernelGGL(rrt_relax_fill_kernel, per_vertex, dim3(RELAX_TPB), 0, ctx->stream, xv);
}

// the counters of the call that has just succeeded, for its _stats report: the rounds, then what the device counted
static void store_front_stats(rrt_batch *b, int64_t rounds, const unsigned long long (&stats)[RELAX_STATS]) {
    b->front_stats[0] = rounds;
    b->front_stats[1] = (int64_t)stats[RELAX_FELL];
    b->front_stats[2] = (int64_t)stats[RELAX_LOS];
    b->front_stats[3] = (int64_t)stats[RELAX_PRICED];
}

// The vertices stay and every parent is chosen again: the costs relaxed in rounds to their fixpoint, the parents in a pass over the
// final costs, then the later stages of the re-root (every vertex stays alive: its old parent edge is a candidate), whose repriced
// costs have to be the fixpoint's, and the seed.  The descriptor's xs stays.  The host reads the count of changes back after every
// round and stops behind a round that changed nothing; a shortest path has fewer than j edges, so j rounds are the most.
// rrt_batch_relax (poses == false: straight-line batches, rows (x, y)) and rrt_batch_relax_poses (poses == true: Dubins batches, rows
// (x, y, h)) are one call with two edges: a Dubins batch relaxes over the words between its poses (rrt_pose_relax.h) on the same
// buckets, flags and counters, prices the new order with words, and its seed carries the heading bytes.
static int batch_relax(const SeedCall &c, int64_t r2) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const bool poses = c.poses;
    int j_in = 0;
    if (const int rc = refuse_grow(c, "the cost of a Dubins word depends on the headings at its ends: a new parent changes the word", j_in, "rrt_batch_relax"))
        return rc;
    if (r2 <= 0) return fail(ctx, RRT_E_ARG, "%s: r2=%lld: the threshold of the squared distance has to be positive", c.who, (long long)r2);
    if (const int rc = refuse_capacity(c)) return rc;
    if (const int rc = stage_samples(c)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, b->seed_tmp.reserve<SeedTmpScratch>(b->n_cap));
    if (const int rc = reserve_relax_set(c)) return rc;
    HIPCHK(ctx, b->seed_time.create(4));
    HIPCHK(ctx, b->front_time.create(7));
    const TreeRef t = tree_ref(b, c.q);
    const RelaxSet set(c);
    const RerootScratch &tmp = set.tmp;
    const RelaxScratch &rx = set.rx;
    const PoseRelaxScratch &px = set.px;
    RerootView rv{};
    int32_t unused = -1;
    PoseRelaxView pv{};
    if (const int rc = tree_input(c, t, j_in, -1, rv, unused, poses ? &pv.heading : nullptr)) return rc;
    rv.root = 0;
    reroot_view(rv, tmp);
    const int j = j_in;
    RelaxView xv{};
    xv.nodes = rv.nodes;
    xv.parent = rv.parent;
    xv.vcost = t.kept > 0 ? t.live_vcost : t.vcost;
    xv.j = j;
    relax_view(ctx, xv, r2, rx, tmp);
    if (poses) pose_relax_view(ctx, pv, xv, c.desc(), px);
    start_replacing(c);
    StageTimer &time = b->front_time;
    auto blocks = [](int items) { return dim3(wgs(items, RELAX_TPB)); };
    const dim3 per_wave(std::clamp<unsigned>(wgs(j, RELAX_TPB / 64), 1, RELAX_MAX_WG));
    if (const int rc = reset_for_buckets(ctx, rv, xv)) return rc;
    HIPCHK(ctx, time.mark(0, ctx->stream));
    fill_buckets(ctx, xv, rrt_relax_cell_kernel, xv);
    if (poses) hipLaunchKernelGGL(rrt_pose_relax_item_kernel, blocks(j), dim3(RELAX_TPB), 0, ctx->stream, pv);
    HIPCHK(ctx, time.mark(1, ctx->stream));
    int64_t rounds = 0;
    double *costs[2] = {xv.cost, xv.cost};
#ifdef RRT_RELAX_TWO_ARRAYS  // (experiment build: a round reads the costs of the round before alone; out_vcost is free until the cost kernel)
    costs[1] = tmp.out_vcost;
    HIPCHK(ctx, hipMemcpyAsync(costs[1], costs[0], (size_t)j * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
#endif
    if (const int rc = relax_rounds(c, xv, rx, [&](int in, int32_t first) {
            if (poses)
                hipLaunchKernelGGL(rrt_pose_relax_round_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, pv, (const uint8_t *)rx.dirty[in], rx.dirty[in ^ 1],
                                   (const uint8_t *)rx.changed[in], rx.changed[in ^ 1], first);
            else
                hipLaunchKernelGGL(rrt_relax_round_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, xv, (const double *)costs[in], costs[in ^ 1],
                                   (const uint8_t *)rx.dirty[in], rx.dirty[in ^ 1], (const uint8_t *)rx.changed[in], rx.changed[in ^ 1], first);
        }, rounds))
        return rc;
    HIPCHK(ctx, time.mark(2, ctx->stream));
    if (poses) hipLaunchKernelGGL(rrt_pose_relax_parent_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, pv);
    else hipLaunchKernelGGL(rrt_relax_parent_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, xv);
    hipLaunchKernelGGL(rrt_reroot_link_kernel, dim3(wgs(j, REROOT_TPB)), dim3(REROOT_TPB), 0, ctx->stream, rv);
    HIPCHK(ctx, time.mark(3, ctx->stream));
    unsigned long long stats[RELAX_STATS] = {0, 0, 0, 0};
    char what[256];
    snprintf(what, sizeof what, "the relaxed parents of query %d on the device are not a tree over all %d vertices, or its costs summed from the root "
             "down are not the fixpoint's", c.q, j);
    OrderAndSeed o;
    o.mark0 = 3;
    o.whole = true;
    o.what = what;
    o.out_heading = poses ? px.out_heading : nullptr;
    const int rc = order_price_and_seed(c, rv, tmp, o, [&] { poses ? price_words(ctx, pv, rv, px) : price_lines(ctx, rv); }, [&] {
        hipLaunchKernelGGL(rrt_relax_check_kernel, blocks(j), dim3(RELAX_TPB), 0, ctx->stream, xv, (const int32_t *)tmp.src, (const double *)tmp.out_vcost,
                           (const int32_t *)(tmp.head + REROOT_COUNT));
        HIPCHK(ctx, hipMemcpyAsync(stats, xv.stats, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
        return (int)RRT_OK;
    });
    if (rc != RRT_OK) return rc;
    store_front_stats(b, rounds, stats);
    return RRT_OK;
}

// ---- re-root a finished Dubins tree at one of its poses (rrt_pose_reroot.h) ----
// batch_relax for a Dubins batch from another root.  The dense input (tree_input) goes root-first into scratch, and that is what the
// buckets, the item kernel, the rounds and the parent pass of the pose relax see.  The costs start at 0 for the root, at the sums of
// the old edges' words for what hangs below it in the old tree (the link kernel, the pointer jumping and the order by depth over the
// OLD parents, then rrt_pose_reroot_start_kernel), and at +inf elsewhere.  What is +inf at the fixpoint is cut; the later stages are
// order_price_and_seed's with whole = false and new_start = true, and the descriptor's hs becomes the root's heading too.
static int batch_reroot_poses(const SeedCall &c, int32_t root, int64_t r2) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    const char *who = c.who;
    const int32_t q = c.q;
    int j_in = 0;
    if (const int rc = refuse_grow(c, "", j_in, "rrt_batch_reroot")) return rc;
    if (const int rc = refuse_capacity(c)) return rc;
    QDesc &d = c.desc();
    if (root < 0 || root >= d.j) return fail(ctx, RRT_E_ARG, "%s: root=%d, query %d has the vertices [0, %d)", who, root, q, d.j);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, b->seed_tmp.reserve<SeedTmpScratch>(b->n_cap));
    const TreeRef t = tree_ref(b, q);
    RerootView rv{};
    PoseRerootView fv{};
    // with a view the input is the view: its parents renumbered into scratch, and the root's number in it (-1: not alive)
    if (const int rc = tree_input(c, t, j_in, root, rv, fv.root, &fv.heading)) return rc;
    if (fv.root < 0)
        return fail(ctx, RRT_E_ARG, "%s: root=%d is not alive in the kept view of query %d (%d of %d vertices alive)", who, root, q, j_in, d.j);
    if (r2 < 0) return fail(ctx, RRT_E_ARG, "%s: r2=%lld: the threshold of the squared distance cannot be negative", who, (long long)r2);
    if (const int rc = stage_samples(c)) return rc;
    if (const int rc = reserve_relax_set(c)) return rc;
    HIPCHK(ctx, b->pose_reroot_tmp.reserve<PoseRerootScratch>(b->n_cap));
    HIPCHK(ctx, b->seed_time.create(4));
    HIPCHK(ctx, b->front_time.create(8));
    const RelaxSet set(c);
    const RerootScratch &tmp = set.tmp;
    const RelaxScratch &rx = set.rx;
    const PoseRelaxScratch &px = set.px;
    const PoseRerootScratch fx = b->pose_reroot_tmp.carve<PoseRerootScratch>();
    const int j = j_in;
    fv.nodes = rv.nodes;
    fv.parent = rv.parent;
    fv.id = rv.id;
    fv.j = j;
    fv.f_nodes = fx.f_nodes;
    fv.f_parent = fx.f_parent;
    fv.f_heading = fx.f_heading;
    fv.f_id = fx.f_id;
    // from here on the input is the root-first one
    rv.nodes = fx.f_nodes;
    rv.parent = fx.f_parent;
    rv.id = fx.f_id;
    rv.root = 0;
    reroot_view(rv, tmp);
    RelaxView xv{};
    xv.nodes = fx.f_nodes;
    xv.parent = fx.f_parent;
    xv.vcost = nullptr;  // (the costs start from the sums below the new root: no kernel of this call reads the old ones)
    xv.j = j;
    relax_view(ctx, xv, r2, rx, tmp);
    PoseRelaxView pv{};
    pv.heading = fx.f_heading;
    pose_relax_view(ctx, pv, xv, d, px);
    start_replacing(c);
    StageTimer &time = b->front_time;
    auto blocks = [](int items) { return dim3(wgs(items, RELAX_TPB)); };
    const dim3 per_wave(std::clamp<unsigned>(wgs(j, RELAX_TPB / 64), 1, RELAX_MAX_WG));
    if (const int rc = reset_for_buckets(ctx, rv, xv)) return rc;
    HIPCHK(ctx, time.mark(0, ctx->stream));
    fill_buckets(ctx, xv, rrt_pose_reroot_front_kernel, fv, xv);
    hipLaunchKernelGGL(rrt_pose_relax_item_kernel, blocks(j), dim3(RELAX_TPB), 0, ctx->stream, pv);
    HIPCHK(ctx, time.mark(1, ctx->stream));
    {  // the start: what hangs below the new root in the OLD tree, placed by depth, and its costs along the old edges
        RerootView sv = rv;
        sv.new_parent = fx.f_parent;  // (the link kernel and rrt_reroot_parent_kernel only read it)
        hipLaunchKernelGGL(rrt_reroot_link_kernel, dim3(wgs(j, REROOT_TPB)), dim3(REROOT_TPB), 0, ctx->stream, sv);
        if (const int rc = order_by_depth(ctx, sv, tmp, nullptr, 0)) return rc;
        hipLaunchKernelGGL(rrt_pose_reroot_start_kernel, dim3(1), dim3(TPB), 0, ctx->stream, sv, (const double *)px.plen, xv.cost);
        HIPCHK(ctx, hipGetLastError());
        if (const int rc = reroot_reset(ctx, rv, true)) return rc;  // (the order runs again behind the parents; an err of this run stays)
        HIPCHK(ctx, hipMemsetAsync(rv.ok, 1, (size_t)j, ctx->stream));
    }
    HIPCHK(ctx, time.mark(2, ctx->stream));
    int64_t rounds = 0;
    if (const int rc = relax_rounds(c, xv, rx, [&](int in, int32_t first) {
            hipLaunchKernelGGL(rrt_pose_reroot_round_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, pv, (const uint8_t *)rx.dirty[in], rx.dirty[in ^ 1],
                               (const uint8_t *)rx.changed[in], rx.changed[in ^ 1], first);
        }, rounds))
        return rc;
    HIPCHK(ctx, time.mark(3, ctx->stream));
    hipLaunchKernelGGL(rrt_pose_reroot_parent_kernel, per_wave, dim3(RELAX_TPB), 0, ctx->stream, pv);
    hipLaunchKernelGGL(rrt_reroot_link_kernel, dim3(wgs(j, REROOT_TPB)), dim3(REROOT_TPB), 0, ctx->stream, rv);
    HIPCHK(ctx, time.mark(4, ctx->stream));
    unsigned long long stats[RELAX_STATS] = {0, 0, 0, 0};
    uint8_t root_heading = 0;
    char what[256];
    snprintf(what, sizeof what, "the parents of query %d on the device chosen from its new root are not a tree over the vertices that were reached, or "
             "its costs summed from the root down are not the fixpoint's", q);
    OrderAndSeed o;
    o.mark0 = 4;
    o.new_start = true;
    o.what = what;
    o.out_heading = px.out_heading;
    o.start_heading = &root_heading;
    const int rc = order_price_and_seed(c, rv, tmp, o, [&] { price_words(ctx, pv, rv, px); }, [&] {
        hipLaunchKernelGGL(rrt_pose_reroot_check_kernel, blocks(j), dim3(RELAX_TPB), 0, ctx->stream, xv, (const int32_t *)tmp.src, (const double *)tmp.out_vcost,
                           (const int32_t *)(tmp.head + REROOT_COUNT));
        // the new start: the root's cell to the head, where order_price_and_seed reads it, and its heading index
        HIPCHK(ctx, hipMemcpyAsync(tmp.head + REROOT_XY, tmp.out_nodes, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(&root_heading, px.out_heading, 1, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(stats, xv.stats, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
        return (int)RRT_OK;
    });
    if (rc != RRT_OK) return rc;
    store_front_stats(b, rounds, stats);
    return RRT_OK;
}

// ---- the entry points of the seed calls ----
// The rrt_batch_ form of a seed call hands its record to `call`, the batch-level call, with what that takes beside the record (`lead`).
// The rrt_plan_ form does the same with a record that lacks batch and log0, which become the batch behind rrt_plan and a local, and
// adds the launch and the result of rrt_plan.
template <typename Call, typename... Lead>
static int batch_seed(const SeedCall &c, Call call, Lead... lead) {
    return c.b ? call(c, lead...) : fail(nullptr, RRT_E_ARG, "%s: NULL", c.who);
}

template <typename Call, typename... Lead>
static int plan_seed(SeedCall c, rrt_ctx *ctx, rrt_result *out, Call call, Lead... lead) {
    if (ctx && !out) return fail(ctx, RRT_E_ARG, "%s: NULL", c.who);
    int32_t log0 = 0;
    c.b = plan_batch(ctx, c.who, NO_PLAN_NO_TREE);
    c.log0 = &log0;
    const int rc = c.b ? call(c, lead...) : RRT_E_ARG;
    return rc != RRT_OK ? rc : run_single(ctx, out);
}

extern "C" int rrt_batch_grow(rrt_batch *b, int32_t q, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0) {
    return batch_seed({"rrt_batch_grow", SeedKind::grow, b, q, samples_xy, m, j0, old_id, log0, false}, batch_grow);
}

extern "C" int rrt_batch_grow_poses(rrt_batch *b, int32_t q, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0) {
    return batch_seed({"rrt_batch_grow_poses", SeedKind::grow, b, q, samples_xyh, m, j0, old_id, log0, true}, batch_grow);
}

extern "C" int rrt_plan_grow(rrt_ctx *ctx, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out) {
    return plan_seed({"rrt_plan_grow", SeedKind::grow, nullptr, 0, samples_xy, m, j0, old_id, nullptr, false}, ctx, out, batch_grow);
}

extern "C" int rrt_plan_grow_poses(rrt_ctx *ctx, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out) {
    return plan_seed({"rrt_plan_grow_poses", SeedKind::grow, nullptr, 0, samples_xyh, m, j0, old_id, nullptr, true}, ctx, out, batch_grow);
}

extern "C" int rrt_batch_reroot(rrt_batch *b, int32_t q, int32_t root, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0) {
    return batch_seed({"rrt_batch_reroot", SeedKind::reroot, b, q, samples_xy, m, j0, old_id, log0, false}, batch_reroot, root);
}

extern "C" int rrt_plan_reroot(rrt_ctx *ctx, int32_t root, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out) {
    return plan_seed({"rrt_plan_reroot", SeedKind::reroot, nullptr, 0, samples_xy, m, j0, old_id, nullptr, false}, ctx, out, batch_reroot, root);
}

extern "C" int rrt_batch_relax(rrt_batch *b, int32_t q, int64_t r2, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0) {
    return batch_seed({"rrt_batch_relax", SeedKind::relax, b, q, samples_xy, m, j0, old_id, log0, false}, batch_relax, r2);
}

extern "C" int rrt_batch_relax_poses(rrt_batch *b, int32_t q, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, int32_t *log0) {
    return batch_seed({"rrt_batch_relax_poses", SeedKind::relax, b, q, samples_xyh, m, j0, old_id, log0, true}, batch_relax, r2);
}

extern "C" int rrt_plan_relax(rrt_ctx *ctx, int64_t r2, const int32_t *samples_xy, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out) {
    return plan_seed({"rrt_plan_relax", SeedKind::relax, nullptr, 0, samples_xy, m, j0, old_id, nullptr, false}, ctx, out, batch_relax, r2);
}

extern "C" int rrt_plan_relax_poses(rrt_ctx *ctx, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id, rrt_result *out) {
    return plan_seed({"rrt_plan_relax_poses", SeedKind::relax, nullptr, 0, samples_xyh, m, j0, old_id, nullptr, true}, ctx, out, batch_relax, r2);
}

extern "C" int rrt_batch_reroot_poses(rrt_batch *b, int32_t q, int32_t root, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id,
                                      int32_t *log0) {
    return batch_seed({"rrt_batch_reroot_poses", SeedKind::reroot_poses, b, q, samples_xyh, m, j0, old_id, log0, true}, batch_reroot_poses, root, r2);
}

extern "C" int rrt_plan_reroot_poses(rrt_ctx *ctx, int32_t root, int64_t r2, const int32_t *samples_xyh, int32_t m, int32_t *j0, int32_t *old_id,
                                     rrt_result *out) {
    return plan_seed({"rrt_plan_reroot_poses", SeedKind::reroot_poses, nullptr, 0, samples_xyh, m, j0, old_id, nullptr, true}, ctx, out, batch_reroot_poses, root, r2);
}

// ---- the rows of the routes to the goals a decision answered: what rrt_batch_routes and rrt_batch_pose_routes start with ----
// The depth pass and the scan of rrt_routes.h (rv: parent, j, vertex, m, cnt, raw_off, err), then the one wait that the sizes force: the
// rows of all routes together decide how much memory the rows need.  Its two refusals: a walk that is no tree's, and more rows than
// `budget` (noun: what the call names its goals).  time: nullptr, or the timer whose marks 2 and 3 go around the two kernels.
static int count_route_rows(const char *who, rrt_batch *b, int32_t q, const RoutesView &rv, size_t budget, const char *noun, StageTimer *time,
                            int64_t &rows) {
    rrt_ctx *ctx = b->ctx;
    HIPCHK(ctx, hipMemsetAsync(rv.err, 0, sizeof(int32_t), ctx->stream));
    if (time) HIPCHK(ctx, time->mark(2, ctx->stream));
    hipLaunchKernelGGL(rrt_route_depth_kernel, dim3(wgs(rv.m, ROUTE_TPB)), dim3(ROUTE_TPB), 0, ctx->stream, rv);
    hipLaunchKernelGGL(rrt_route_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, (const int32_t *)rv.cnt, rv.raw_off, rv.m);
    if (time) HIPCHK(ctx, time->mark(3, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    int32_t err = 0;
    HIPCHK(ctx, hipMemcpyAsync(&rows, rv.raw_off + rv.m, sizeof rows, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&err, rv.err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    if (err)
        return fail(ctx, RRT_E_HIP, "%s: a parent walk of query %d did not reach vertex 0 within %d steps: the parent array on the device is not a tree", who, q, rv.j);
    if (rows < 0 || (uint64_t)rows > budget)
        return fail(ctx, RRT_E_ARG, "%s: the routes of these %d %s have %lld rows together, at most %zu per call: pass fewer %s at a time", who, rv.m, noun,
                    (long long)rows, budget, noun);
    return RRT_OK;
}

// ---- finished routes to many goals (rrt_routes.h) ----
// where a routes call puts its answers: an entry per goal, one more in offsets and in point_offsets (the pose calls' alone)
struct RoutesOut {
    int32_t *vertex;
    double *cost, *length;
    int64_t *offsets, *point_offsets;
};

static int batch_routes(const char *who, rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, uint32_t flags, const RoutesOut &out) {
    rrt_ctx *ctx = b->ctx;
    const auto [vertex, cost, length, offsets, point_offsets] = out;
    b->route_rows = -1;  // whatever happens below, the rows of an earlier call are gone
    if (flags & ~(uint32_t)RRT_ROUTES_SHORTCUT) return fail(ctx, RRT_E_ARG, "%s: flags=0x%x, only RRT_ROUTES_SHORTCUT is defined", who, flags);
    if (const int rc = goals_decide(who, b, q, goals_xy, m, !vertex || !cost || !length || !offsets); rc != RRT_OK) return rc;
    if (m == 0) {
        offsets[0] = 0;
        b->route_rows = 0;
        return RRT_OK;
    }
    HIPCHK(ctx, b->route_goal.reserve<RouteGoalScratch>(m));
    const RouteGoalScratch goal = b->route_goal.carve<RouteGoalScratch>();
    const bool cut = (flags & RRT_ROUTES_SHORTCUT) != 0;
    const TreeRef t = tree_ref(b, q);
    RoutesView rv{};
    rv.og = ctx->og;
    rv.H = ctx->H;
    rv.nodes = t.nodes;
    rv.parent = t.parent;
    rv.j = b->h_desc[(size_t)q].j;
    rv.goals = b->goal_xy.as<uint32_t>();
    rv.vertex = b->goal_vertex.as<int32_t>();
    rv.m = m;
    rv.length = goal.length;
    rv.raw_off = goal.raw_off;
    rv.fin_off = cut ? goal.fin_off : goal.raw_off;
    rv.cnt = goal.cnt;
    rv.kept = goal.kept;
    rv.err = goal.err;
    int64_t raw_rows = 0;
    if (const int rc = count_route_rows(who, b, q, rv, ROUTE_ROW_BUDGET, "goals", nullptr, raw_rows)) return rc;
    HIPCHK(ctx, b->route_row.reserve<RouteRowScratch>(raw_rows));
    const RouteRowScratch row = b->route_row.carve<RouteRowScratch>();
    rv.row_xy = row.row_xy;
    rv.row_id = row.row_id;
    rv.out_xy = row.out_xy;
    rv.out_id = row.out_id;
    hipLaunchKernelGGL(rrt_route_fill_kernel, dim3(wgs(m, ROUTE_TPB)), dim3(ROUTE_TPB), 0, ctx->stream, rv, cut ? 0 : 1);
    if (cut) {
        const unsigned cut_wgs = (unsigned)(m < ROUTE_CUT_MAX_WG ? m : ROUTE_CUT_MAX_WG);
        hipLaunchKernelGGL((b->flags & RRT_FLAG_LARGE_GRID) ? rrt_route_cut_large_kernel : rrt_route_cut_kernel, dim3(cut_wgs), dim3(TPB), 0, ctx->stream, rv);
        hipLaunchKernelGGL(rrt_route_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, (const int32_t *)rv.kept, rv.fin_off, m);
    }
    hipLaunchKernelGGL(rrt_route_pack_kernel, dim3(wgs(m, ROUTE_TPB / 64)), dim3(ROUTE_TPB), 0, ctx->stream, rv);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(length, rv.length, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(offsets, rv.fin_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = fetch_goal_answers(b, m, vertex, cost)) return rc;
    if (offsets[m] < 0 || offsets[m] > raw_rows) return fail(ctx, RRT_E_HIP, "%s: %lld rows kept of %lld", who, (long long)offsets[m], (long long)raw_rows);
    b->route_rows = offsets[m];
    return RRT_OK;
}

static int batch_routes_rows(const char *who, rrt_batch *b, int32_t *xy, int32_t *id, int64_t rows) {
    rrt_ctx *ctx = b->ctx;
    if (b->route_rows < 0)
        return fail(ctx, RRT_E_ARG, "%s: no routes on this batch (no rrt_batch_routes call yet, one that failed, or a launch or rearm since)", who);
    if (rows != b->route_rows) return fail(ctx, RRT_E_ARG, "%s: rows=%lld, the last rrt_batch_routes call left %lld", who, (long long)rows, (long long)b->route_rows);
    if (rows == 0) return RRT_OK;
    if (!xy || !id) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const RouteRowScratch row = b->route_row.carve<RouteRowScratch>();
    HIPCHK(ctx, hipMemcpyAsync(xy, row.out_xy, (size_t)rows * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(id, row.out_id, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    return RRT_OK;
}

extern "C" int rrt_batch_routes(rrt_batch *b, int32_t q, const int32_t *goals_xy, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                                int64_t *offsets) {
    return b ? batch_routes("rrt_batch_routes", b, q, goals_xy, m, flags, {vertex, cost, length, offsets, nullptr}) : fail(nullptr, RRT_E_ARG, "rrt_batch_routes: NULL");
}

extern "C" int rrt_batch_routes_rows(rrt_batch *b, int32_t *xy, int32_t *id, int64_t rows) {
    return b ? batch_routes_rows("rrt_batch_routes_rows", b, xy, id, rows) : fail(nullptr, RRT_E_ARG, "rrt_batch_routes_rows: NULL");
}

extern "C" int rrt_plan_routes(rrt_ctx *ctx, const int32_t *goals_xy, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length, int64_t *offsets) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_routes", NO_PLAN_NO_TREE);
    return s ? batch_routes("rrt_plan_routes", s, 0, goals_xy, m, flags, {vertex, cost, length, offsets, nullptr}) : RRT_E_ARG;
}

extern "C" int rrt_plan_routes_rows(rrt_ctx *ctx, int32_t *xy, int32_t *id, int64_t rows) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_routes_rows", "no routes (no rrt_plan on this context yet, or its batch is gone)");
    return s ? batch_routes_rows("rrt_plan_routes_rows", s, xy, id, rows) : RRT_E_ARG;
}

// ---- finished routes to many goal poses, and the vehicle's path along them (rrt_pose_routes.h) ----
// rrt_batch_pose_routes (cut == false) and rrt_batch_pose_shortcuts (cut == true) are one call: with `cut` the rows of the walks go to
// scratch of their own, the shortcut kernel keeps some of them, and the dense rows that the leg, length and points kernels read are
// the kept ones under their own offsets.  The rows and points either call leaves are what the _rows / _points calls serve; the stage
// times are kept apart (pose_route_time / pose_cut_time), so that rrt_batch_pose_routes_ms goes on reporting the last plain call.
static int batch_pose_routes(const char *who, rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, uint32_t flags, const RoutesOut &out, bool cut) {
    rrt_ctx *ctx = b->ctx;
    const auto [vertex, cost, length, offsets, point_offsets] = out;
    b->pose_route_rows = b->pose_route_points = -1;  // whatever happens below, the rows and points of an earlier call are gone
    StageTimer &time = cut ? b->pose_cut_time : b->pose_route_time;
    time.ran = 0;
    const int leg_ev = cut ? 6 : 4;  // (the marks around legs + lengths, and behind them those around the points)
    if (flags & ~(uint32_t)RRT_POSE_ROUTES_POINTS) return fail(ctx, RRT_E_ARG, "%s: flags=0x%x, only RRT_POSE_ROUTES_POINTS is defined", who, flags);
    const bool pts = (flags & RRT_POSE_ROUTES_POINTS) != 0;
    if (const int rc = poses_decide(who, b, q, poses_xyh, m, !vertex || !cost || !length || !offsets || (pts && !point_offsets), "rrt_batch_routes", &time);
        rc != RRT_OK)
        return rc;
    if (m == 0) {
        offsets[0] = 0;
        if (point_offsets) point_offsets[0] = 0;
        b->pose_route_rows = 0;
        b->pose_route_points = pts ? 0 : -1;
        return RRT_OK;
    }
    HIPCHK(ctx, time.create(leg_ev + 4));
    HIPCHK(ctx, b->pose_route_goal.reserve<PoseRouteGoalScratch>(m));
    const PoseRouteGoalScratch goal = b->pose_route_goal.carve<PoseRouteGoalScratch>();
    const QDesc &d = b->h_desc[(size_t)q];
    const TreeRef t = tree_ref(b, q);  // (the whole tree: the vertex numbers the decision answers in are its own, after a keep too)
    PoseRoutesView pr{};
    pr.W = ctx->W;
    pr.H = ctx->H;
    pr.nodes = t.nodes;
    pr.parent = t.parent;
    pr.heading = t.heading;
    pr.nh = d.nh;
    pr.rho = d.rho;
    pr.goals = b->goal_xy.as<uint32_t>();
    pr.goal_h = b->pose_h.as<uint8_t>();
    pr.vertex = b->goal_vertex.as<int32_t>();
    pr.m = m;
    pr.length = goal.length;
    pr.raw_off = goal.raw_off;
    pr.goal_pt_off = pts ? goal.goal_pt_off : nullptr;
    pr.cnt = goal.cnt;
    pr.err = goal.err;
    // the depth pass and the scan are rrt_routes.h's, as they are: they read vertex / parent / j / m and write cnt / err / raw_off
    RoutesView rv{};
    rv.parent = t.parent;
    rv.j = d.j;
    rv.vertex = pr.vertex;
    rv.m = m;
    rv.cnt = goal.cnt;
    rv.raw_off = goal.raw_off;
    rv.err = goal.err;
    int64_t rows = 0;  // (the first wait of this call)
    if (const int rc = count_route_rows(who, b, q, rv, POSE_ROUTE_ROW_BUDGET, "poses", &time, rows)) return rc;
    int64_t npoints = 0;
    int32_t err = 0;
    HIPCHK(ctx, b->pose_route_row.reserve<PoseRouteRowScratch>(std::max<int64_t>(rows, 1)));  // (no row: pt_off alone, one zero)
    if (pts && rows > 0) HIPCHK(ctx, b->pose_route_sweep.reserve(rows, (size_t)rows * POSE_ROUTE_SWEEP_BYTES));
    const PoseRouteRowScratch row = b->pose_route_row.carve<PoseRouteRowScratch>();
    pr.rows = rows;
    pr.leg_len = row.leg_len;
    pr.pt_off = row.pt_off;
    pr.row_xy = row.row_xy;
    pr.row_id = row.row_id;
    pr.npts = pts ? row.npts : nullptr;
    pr.row_h = row.row_h;
    pr.sweep_bytes = pts ? b->pose_route_sweep.p : nullptr;
    HIPCHK(ctx, time.mark(4, ctx->stream));
    if (cut && rows > 0) {
        // the raw rows and what is kept of them per goal: the walks fill the raw rows, the shortcut kernel compacts each goal's kept
        // rows to the front of its own, the pack makes them the dense rows above
        HIPCHK(ctx, b->pose_cut_row.reserve<PoseCutRowScratch>(rows));
        HIPCHK(ctx, b->pose_cut_goal.reserve<PoseCutGoalScratch>(m));
        const PoseCutRowScratch cut_row = b->pose_cut_row.carve<PoseCutRowScratch>();
        const PoseCutGoalScratch cut_goal = b->pose_cut_goal.carve<PoseCutGoalScratch>();
        PoseCutView pc{};
        pc.og = ctx->og;
        pc.W = ctx->W;
        pc.H = ctx->H;
        pc.nh = d.nh;
        pc.rho = d.rho;
        pc.m = m;
        pc.cnt = goal.cnt;
        pc.raw_off = goal.raw_off;
        pc.fin_off = cut_goal.fin_off;
        pc.kept = cut_goal.kept;
        pc.row_xy = cut_row.row_xy;
        pc.row_id = cut_row.row_id;
        pc.row_h = cut_row.row_h;
        pc.out_xy = pr.row_xy;
        pc.out_h = pr.row_h;
        pc.out_id = pr.row_id;
        PoseRoutesView raw = pr;
        raw.row_xy = pc.row_xy;
        raw.row_h = pc.row_h;
        raw.row_id = pc.row_id;
        const unsigned waves_grid = wgs(m, POSE_CUT_TPB / 64);
        hipLaunchKernelGGL(rrt_pose_route_fill_kernel, dim3(wgs(m, POSE_ROUTE_TPB)), dim3(POSE_ROUTE_TPB), 0, ctx->stream, raw);
        hipLaunchKernelGGL(rrt_pose_route_cut_kernel, dim3(std::min<unsigned>(waves_grid, POSE_CUT_MAX_WG)), dim3(POSE_CUT_TPB), 0, ctx->stream, pc);
        hipLaunchKernelGGL(rrt_route_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, (const int32_t *)pc.kept, cut_goal.fin_off, m);
        hipLaunchKernelGGL(rrt_pose_route_pack_kernel, dim3(waves_grid), dim3(POSE_CUT_TPB), 0, ctx->stream, pc);
        HIPCHK(ctx, time.mark(5, ctx->stream));
        HIPCHK(ctx, hipGetLastError());
        // a wait of the shortcut call alone: the leg and the points kernel take the number of dense rows by value
        int64_t kept_rows = 0;
        HIPCHK(ctx, hipMemcpyAsync(&kept_rows, cut_goal.fin_off + m, sizeof kept_rows, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, wait_stream_spin(ctx->stream));
        if (kept_rows < 1 || kept_rows > rows) return fail(ctx, RRT_E_HIP, "%s: %lld rows kept of %lld", who, (long long)kept_rows, (long long)rows);
        pr.cnt = pc.kept;
        pr.raw_off = cut_goal.fin_off;
        pr.rows = rows = kept_rows;
        HIPCHK(ctx, time.mark(6, ctx->stream));
    } else if (cut) {
        HIPCHK(ctx, time.mark(5, ctx->stream));  // (nothing connects: no row to cut; cnt and raw_off, all zero, are the kept ones)
        HIPCHK(ctx, time.mark(6, ctx->stream));
    }
    if (rows > 0) {
        const unsigned rows_grid = std::min<unsigned>(wgs(rows, POSE_ROUTE_TPB), POSE_ROUTE_MAX_WG);
        if (!cut) hipLaunchKernelGGL(rrt_pose_route_fill_kernel, dim3(wgs(m, POSE_ROUTE_TPB)), dim3(POSE_ROUTE_TPB), 0, ctx->stream, pr);
        hipLaunchKernelGGL(rrt_pose_route_leg_kernel, dim3(rows_grid), dim3(POSE_ROUTE_TPB), 0, ctx->stream, pr);
        // a leg's count is at most POSE_ROUTE_LEG_POINTS = 2^19 (the leg kernel raises err beyond, and a word whose every sample lies inside
        // a grid of 2048 x 2048 cells has some 55 000 at most): the 1024 counts of a pass of the scan sum below 2^32, as its rows do
        if (pts) hipLaunchKernelGGL(rrt_route_scan_kernel, dim3(1), dim3(TPB), 0, ctx->stream, (const int32_t *)pr.npts, pr.pt_off, (int32_t)rows);
    } else if (pts) {
        HIPCHK(ctx, hipMemsetAsync(pr.pt_off, 0, sizeof(int64_t), ctx->stream));  // (nothing connects: no point)
    }
    hipLaunchKernelGGL(rrt_pose_route_length_kernel, dim3(wgs(m + 1, POSE_ROUTE_TPB)), dim3(POSE_ROUTE_TPB), 0, ctx->stream, pr);
    HIPCHK(ctx, time.mark(leg_ev + 1, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(length, pr.length, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(offsets, pr.raw_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&err, pr.err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    if (pts) HIPCHK(ctx, hipMemcpyAsync(point_offsets, pr.goal_pt_off, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    // the second wait (with points: the points of all legs together decide how much memory the points need)
    if (const int rc = fetch_goal_answers(b, m, vertex, cost)) return rc;
    if (err)
        return fail(ctx, RRT_E_HIP, "%s: a leg of a route of query %d has no Dubins word, or a length that is not finite or beyond %d samples: the tree on the "
                    "device is not one the planner built", who, q, POSE_ROUTE_LEG_POINTS);
    if (offsets[m] != rows) return fail(ctx, RRT_E_HIP, "%s: %lld rows of %lld", who, (long long)offsets[m], (long long)rows);
    if (pts) {
        npoints = point_offsets[m];
        if (npoints < 0 || (uint64_t)npoints > POSE_ROUTE_POINT_BUDGET)
            return fail(ctx, RRT_E_ARG, "%s: the routes of these %d poses have %lld points together, at most %zu per call: pass fewer poses at a time", who, m,
                        (long long)npoints, POSE_ROUTE_POINT_BUDGET);
        if (npoints > 0) {
            HIPCHK(ctx, b->pose_route_pts.reserve(npoints, (size_t)npoints * sizeof(double2)));
            pr.npoints = npoints;
            pr.points = b->pose_route_pts.as<double2>();
            const unsigned pts_grid = std::min<unsigned>(wgs(npoints, POSE_ROUTE_TPB), POSE_ROUTE_MAX_WG);
            HIPCHK(ctx, time.mark(leg_ev + 2, ctx->stream));
            hipLaunchKernelGGL(rrt_pose_route_points_kernel, dim3(pts_grid), dim3(POSE_ROUTE_TPB), 0, ctx->stream, pr);
            HIPCHK(ctx, time.mark(leg_ev + 3, ctx->stream));
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, wait_stream_spin(ctx->stream));  // (so that a fault of the kernel is this call's, and the stage times are there)
        }
    }
    b->pose_last_m = m;
    b->pose_route_rows = rows;
    b->pose_route_points = pts ? npoints : -1;
    time.ran = (pts && npoints > 0 ? 4 : 3) + (cut ? 1 : 0);
    return RRT_OK;
}

static int batch_pose_routes_rows(const char *who, rrt_batch *b, int32_t *xyh, int32_t *id, int64_t rows) {
    rrt_ctx *ctx = b->ctx;
    if (b->pose_route_rows < 0)
        return fail(ctx, RRT_E_ARG, "%s: no routes on this batch (no rrt_batch_pose_routes call yet, one that failed, or a launch, rearm, keep or grow since)", who);
    if (rows != b->pose_route_rows)
        return fail(ctx, RRT_E_ARG, "%s: rows=%lld, the last rrt_batch_pose_routes call left %lld", who, (long long)rows, (long long)b->pose_route_rows);
    if (rows == 0) return RRT_OK;
    if (!xyh || !id) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const PoseRouteRowScratch row = b->pose_route_row.carve<PoseRouteRowScratch>();
    b->stage.resize((size_t)rows);
    b->stage8.resize((size_t)rows);
    HIPCHK(ctx, hipMemcpyAsync(b->stage.data(), row.row_xy, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(b->stage8.data(), row.row_h, (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(id, row.row_id, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    for (int64_t r = 0; r < rows; ++r) {
        const uint32_t p = b->stage[(size_t)r];
        xyh[3 * r] = (int32_t)(p & 0xffffu);
        xyh[3 * r + 1] = (int32_t)(p >> 16);
        xyh[3 * r + 2] = (int32_t)b->stage8[(size_t)r];
    }
    return RRT_OK;
}

static int batch_pose_routes_points(const char *who, rrt_batch *b, double *xy, int64_t points) {
    rrt_ctx *ctx = b->ctx;
    if (b->pose_route_points < 0)
        return fail(ctx, RRT_E_ARG, "%s: no points on this batch (no rrt_batch_pose_routes call with RRT_POSE_ROUTES_POINTS yet, one that failed, or a launch, "
                    "rearm, keep or grow since)", who);
    if (points != b->pose_route_points)
        return fail(ctx, RRT_E_ARG, "%s: points=%lld, the last rrt_batch_pose_routes call left %lld", who, (long long)points, (long long)b->pose_route_points);
    if (points == 0) return RRT_OK;
    if (!xy) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(xy, b->pose_route_pts.p, (size_t)points * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    return RRT_OK;
}

extern "C" int rrt_batch_pose_routes(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                                     int64_t *offsets, int64_t *point_offsets) {
    return b ? batch_pose_routes("rrt_batch_pose_routes", b, q, poses_xyh, m, flags, {vertex, cost, length, offsets, point_offsets}, false)
             : fail(nullptr, RRT_E_ARG, "rrt_batch_pose_routes: NULL");
}

extern "C" int rrt_batch_pose_routes_rows(rrt_batch *b, int32_t *xyh, int32_t *id, int64_t rows) {
    return b ? batch_pose_routes_rows("rrt_batch_pose_routes_rows", b, xyh, id, rows) : fail(nullptr, RRT_E_ARG, "rrt_batch_pose_routes_rows: NULL");
}

extern "C" int rrt_batch_pose_routes_points(rrt_batch *b, double *xy, int64_t points) {
    return b ? batch_pose_routes_points("rrt_batch_pose_routes_points", b, xy, points) : fail(nullptr, RRT_E_ARG, "rrt_batch_pose_routes_points: NULL");
}

extern "C" int rrt_plan_pose_routes(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                                    int64_t *offsets, int64_t *point_offsets) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_pose_routes", NO_PLAN_NO_TREE);
    return s ? batch_pose_routes("rrt_plan_pose_routes", s, 0, poses_xyh, m, flags, {vertex, cost, length, offsets, point_offsets}, false) : RRT_E_ARG;
}

// the same call with the shortcut pass (rrt_pose_route_cut_kernel) between the walks and the legs
extern "C" int rrt_batch_pose_shortcuts(rrt_batch *b, int32_t q, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost,
                                        double *length, int64_t *offsets, int64_t *point_offsets) {
    return b ? batch_pose_routes("rrt_batch_pose_shortcuts", b, q, poses_xyh, m, flags, {vertex, cost, length, offsets, point_offsets}, true)
             : fail(nullptr, RRT_E_ARG, "rrt_batch_pose_shortcuts: NULL");
}

extern "C" int rrt_plan_pose_shortcuts(rrt_ctx *ctx, const int32_t *poses_xyh, int32_t m, uint32_t flags, int32_t *vertex, double *cost, double *length,
                                       int64_t *offsets, int64_t *point_offsets) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_pose_shortcuts", NO_PLAN_NO_TREE);
    return s ? batch_pose_routes("rrt_plan_pose_shortcuts", s, 0, poses_xyh, m, flags, {vertex, cost, length, offsets, point_offsets}, true) : RRT_E_ARG;
}

extern "C" int rrt_plan_pose_routes_rows(rrt_ctx *ctx, int32_t *xyh, int32_t *id, int64_t rows) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_pose_routes_rows", "no routes (no rrt_plan on this context yet, or its batch is gone)");
    return s ? batch_pose_routes_rows("rrt_plan_pose_routes_rows", s, xyh, id, rows) : RRT_E_ARG;
}

extern "C" int rrt_plan_pose_routes_points(rrt_ctx *ctx, double *xy, int64_t points) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_pose_routes_points", "no points (no rrt_plan on this context yet, or its batch is gone)");
    return s ? batch_pose_routes_points("rrt_plan_pose_routes_points", s, xy, points) : RRT_E_ARG;
}

// ---- the field calls: every cell of a window of the map against a finished tree (rrt_field.h, rrt_pose_field.h) ----
// connect_goals / connect_poses for every cell of the window, without the cells as goals: the vertices of the dense input (decide_over:
// the tree, or its kept view) are bucketed once by the relax calls' bucket kernels (relax_cells gives the edge: FIELD_MIN_SHIFT, doubled
// until the cells fit), and the call's kernel decides every cell from the buckets whose lower bound can still beat what the cell has.
// The answers go through goal_vertex / goal_cost, which the goals calls share, and are copied out in the window's own (w, h) order.
static_assert(FIELD_STATS == 4 && POSE_FIELD_STATS == 4, "the field calls clear, read back and report four counters, whichever kernel counted them");

// One field call, as its entry point fills it in once its refusals have passed: field_buckets and run_field take it.
struct FieldCall {
    rrt_batch *b;
    int32_t q;
    FieldWindow win;
    StageTimer *time;  // the call's own timer ...
    int64_t *stats;    // ... and where its four counters go
    struct {
        void *host;  // (nullptr: no such output)
        DevBuf *dev;
        size_t each;
    } out[3];  // what is read back, an entry per cell of the window each: vertex, cost, and of a pose call the arrival heading
    int64_t cells() const { return (int64_t)win.w * win.h; }  // (inside a grid of at most 4096 x 4096: 2^24 cells)
};

// From here on the last reports of the call's family are gone.  Room for the outputs and for the buckets (a FieldScratch in field_tmp), and
// what both kernel views have filled in: the RelaxView from the scratch, the window and the answers.
template <typename View>
static int field_buckets(const FieldCall &c, View &v) {
    rrt_batch *b = c.b;
    rrt_ctx *ctx = b->ctx;
    c.time->ran = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (const auto &o : c.out)
        if (o.host) HIPCHK(ctx, o.dev->reserve(c.cells(), (size_t)c.cells() * o.each));
    HIPCHK(ctx, b->field_tmp.reserve<FieldScratch>(b->n_cap, (size_t)RELAX_MAX_CELLS));
    const FieldScratch fx = b->field_tmp.carve<FieldScratch>((size_t)RELAX_MAX_CELLS);
    bucket_view(ctx, v.xv, (int64_t)1 << (2 * FIELD_MIN_SHIFT), fx);
    v.xv.item_cost = fx.item_cost;
    v.xv.cell_min = fx.cell_min;
    v.xv.err = fx.err;
    v.W = ctx->W;
    v.x0 = c.win.x0;
    v.y0 = c.win.y0;
    v.w = c.win.w;
    v.h = c.win.h;
    v.vertex = b->goal_vertex.as<int32_t>();
    v.cost = b->goal_cost.as<double>();
    return RRT_OK;
}

static int clear_field_buckets(rrt_ctx *ctx, const RelaxView &xv) {
    const size_t cells = (size_t)xv.ncx * (size_t)xv.ncy;
    HIPCHK(ctx, hipMemsetAsync(xv.stats, 0, FIELD_STATS * sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(xv.err, 0, sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(xv.cell_fill, 0, cells * sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(xv.cell_start, 0, (cells + 1) * sizeof(int32_t), ctx->stream));  // (a tree without a vertex launches no bucket kernel)
    HIPCHK(ctx, hipMemsetAsync(xv.cell_min, 0xff, cells * sizeof(unsigned long long), ctx->stream));
    return RRT_OK;
}

// The four stages of a field call, every reserve behind it: buckets, decide, remap, read-back.  v: the view the call's kernels take; the
// tree goes into it here.  items(heading, j): behind the buckets, what else the call keeps per item; decide(): its kernel over the window.
// FIELD_VERTEX_LOST: the device raised err; the caller says what that means for its kernels, and no reports are left, as after any failure.
constexpr int FIELD_VERTEX_LOST = 1 << 30;  // (no RRT_ code, and never returned to a caller of the library)
template <typename View, typename Items, typename Decide>
static int run_field(const FieldCall &c, View &v, Items items, Decide decide) {
    rrt_ctx *ctx = c.b->ctx;
    StageTimer &time = *c.time;
    RelaxView &xv = v.xv;
    HIPCHK(ctx, time.create(5));
    if (const int rc = clear_field_buckets(ctx, xv)) return rc;
    HIPCHK(ctx, time.mark(0, ctx->stream));
    hipError_t marked = hipSuccess;
    decide_over(c.b, c.q, v.vertex, (int32_t)c.cells(), [&](const uint32_t *nodes, const double *vcost, const uint8_t *heading, int32_t j) {
        xv.nodes = nodes;
        xv.vcost = vcost;
        xv.j = j;
        if (j > 0) fill_buckets(ctx, xv, rrt_relax_cell_kernel, xv);
        items(heading, j);
        marked = time.mark(1, ctx->stream);
        decide();
        if (marked == hipSuccess) marked = time.mark(2, ctx->stream);
    });
    HIPCHK(ctx, marked);
    HIPCHK(ctx, time.mark(3, ctx->stream));
    HIPCHK(ctx, hipGetLastError());
    unsigned long long stats[FIELD_STATS] = {0, 0, 0, 0};
    int32_t err = 0;
    for (const auto &o : c.out)
        if (o.host) HIPCHK(ctx, hipMemcpyAsync(o.host, o.dev->p, (size_t)c.cells() * o.each, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(stats, xv.stats, sizeof stats, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&err, xv.err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, time.mark(4, ctx->stream));
    HIPCHK(ctx, wait_stream_spin(ctx->stream));
    if (err) return FIELD_VERTEX_LOST;
    for (int k = 0; k < FIELD_STATS; ++k) c.stats[k] = (int64_t)stats[k];
    time.ran = 4;
    return RRT_OK;
}

// the cost-to-come field (rrt_field.h): rrt_field_kernel, on a large grid rrt_field_large_kernel, prices straight lines to cells
static int cost_field(const char *who, rrt_batch *b, int32_t q, const FieldWindow &win, int32_t *vertex, double *cost) {
    rrt_ctx *ctx = b->ctx;
    if (b->flags & RRT_FLAG_DUBINS)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: a Dubins batch (its goal is a pose, and there is no field of poses here; these kernels price straight lines to cells)", who);
    if (const int rc = refuse_goals_call(who, b, q, 0, "goals")) return rc;
    if (const int rc = refuse_window(who, ctx, win)) return rc;
    if (!vertex || !cost) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (const int rc = refuse_vertex_count(who, b, q)) return rc;
    const FieldCall c{b, q, win, &b->field_time, b->field_stats, {{vertex, &b->goal_vertex, sizeof(int32_t)}, {cost, &b->goal_cost, sizeof(double)}, {}}};
    FieldView fv{};
    if (const int rc = field_buckets(c, fv)) return rc;
    const int rc = run_field(c, fv, [](const uint8_t *, int32_t) {}, [&] {
        const int64_t runs = (int64_t)win.w * ((win.h + FIELD_RUN - 1) / FIELD_RUN);
        hipLaunchKernelGGL((b->flags & RRT_FLAG_LARGE_GRID) ? rrt_field_large_kernel : rrt_field_kernel,
                           dim3(std::clamp<unsigned>(wgs(runs, FIELD_TPB / 64), 1, FIELD_MAX_WG)), dim3(FIELD_TPB), 0, ctx->stream, fv);
    });
    if (rc != FIELD_VERTEX_LOST) return rc;
    return fail(ctx, RRT_E_HIP, "%s: a vertex of query %d on the device lies outside the buckets of the %dx%d grid", who, q, ctx->W, ctx->H);
}

extern "C" int rrt_batch_cost_field(rrt_batch *b, int32_t q, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t *vertex, double *cost) {
    return b ? cost_field("rrt_batch_cost_field", b, q, {x0, y0, w, h}, vertex, cost) : fail(nullptr, RRT_E_ARG, "rrt_batch_cost_field: NULL");
}

extern "C" int rrt_plan_cost_field(rrt_ctx *ctx, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t *vertex, double *cost) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_cost_field", NO_PLAN_NO_TREE);
    return s ? cost_field("rrt_plan_cost_field", s, 0, {x0, y0, w, h}, vertex, cost) : RRT_E_ARG;
}

// The pose cost field (rrt_pose_field.h), at one arrival heading or at the best of all (heading -1): cost_field's buckets (field_tmp serves no
// other call of a Dubins batch), the heading byte of every item beside them (PoseRelaxScratch's item_h: the relax calls fill it anew each time).
static int pose_field(const char *who, rrt_batch *b, int32_t q, const FieldWindow &win, int32_t heading, int32_t *vertex, double *cost, int32_t *heading_out) {
    rrt_ctx *ctx = b->ctx;
    if (!(b->flags & RRT_FLAG_DUBINS))
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: not a Dubins batch (its goals are cells and its edges straight lines: use rrt_batch_cost_field)", who);
    if (const int rc = refuse_goals_call(who, b, q, 0, "poses")) return rc;
    if (const int rc = refuse_window(who, ctx, win)) return rc;
    if (!vertex || !cost || !heading_out) return fail(ctx, RRT_E_ARG, "%s: NULL", who);
    if (const int rc = refuse_pose_desc(who, b, q)) return rc;
    const QDesc &d = b->h_desc[(size_t)q];
    if (heading < -1 || heading >= d.nh)
        return fail(ctx, RRT_E_ARG, "%s: heading %d, query %d has headings [0, %d) (-1: any heading)", who, heading, q, d.nh);
    if (const int rc = refuse_vertex_count(who, b, q)) return rc;
    if (d.j > POSE_FIELD_MAX_J)
        return fail(ctx, RRT_E_UNSUPPORTED, "%s: query %d has %d vertices, at most %d (a pair of heading and vertex is one 32-bit key)", who, q, d.j, POSE_FIELD_MAX_J);
    const FieldCall c{b, q, win, &b->pose_field_time, b->pose_field_stats,
                      {{vertex, &b->goal_vertex, sizeof(int32_t)}, {cost, &b->goal_cost, sizeof(double)}, {heading_out, &b->pose_field_heading, sizeof(int32_t)}}};
    PoseFieldView pv{};
    if (const int rc = field_buckets(c, pv)) return rc;
    HIPCHK(ctx, b->pose_relax_tmp.reserve<PoseRelaxScratch>(b->n_cap));
    pv.nh = d.nh;
    pv.rho = d.rho;
    pv.item_h = b->pose_relax_tmp.carve<PoseRelaxScratch>().item_h;  // (of that scratch, item_h alone)
    pv.heading_lo = heading < 0 ? 0 : heading;
    pv.heading_hi = heading < 0 ? d.nh : heading + 1;
    const int64_t m = c.cells();
    pv.run = (int32_t)std::clamp<int64_t>(m / POSE_FIELD_WAVES, 1, POSE_FIELD_RUN);  // (a small window: short runs, so that every CU has cells)
    pv.heading_out = b->pose_field_heading.as<int32_t>();
    auto items = [&](const uint8_t *headings, int32_t j) {
        pv.heading = headings;
        if (j > 0) hipLaunchKernelGGL(rrt_pose_field_item_kernel, dim3(wgs(j, RELAX_TPB)), dim3(RELAX_TPB), 0, ctx->stream, pv);
    };
    const int rc = run_field(c, pv, items, [&] {
        const int64_t runs = (int64_t)win.w * ((win.h + pv.run - 1) / pv.run);
        hipLaunchKernelGGL(rrt_pose_field_kernel, dim3(std::clamp<unsigned>(wgs(runs, POSE_FIELD_TPB / 64), 1, POSE_FIELD_MAX_WG)), dim3(POSE_FIELD_TPB), 0,
                           ctx->stream, pv);
    });
    if (rc != FIELD_VERTEX_LOST) return rc;
    return fail(ctx, RRT_E_HIP, "%s: a vertex of query %d on the device lies outside the buckets of the %dx%d grid, or its heading outside [0, %d)", who, q, ctx->W,
                ctx->H, d.nh);
}

extern "C" int rrt_batch_pose_field(rrt_batch *b, int32_t q, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t heading, int32_t *vertex, double *cost,
                                    int32_t *heading_out) {
    return b ? pose_field("rrt_batch_pose_field", b, q, {x0, y0, w, h}, heading, vertex, cost, heading_out) : fail(nullptr, RRT_E_ARG, "rrt_batch_pose_field: NULL");
}

extern "C" int rrt_plan_pose_field(rrt_ctx *ctx, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t heading, int32_t *vertex, double *cost, int32_t *heading_out) {
    rrt_batch *s = plan_batch(ctx, "rrt_plan_pose_field", NO_PLAN_NO_TREE);
    return s ? pose_field("rrt_plan_pose_field", s, 0, {x0, y0, w, h}, heading, vertex, cost, heading_out) : RRT_E_ARG;
}

// ---- the reports: the kernel times in ms of the stages (_ms) and the counters (_stats) of the last successful call of a family ----
// One row per family.  A family that is a seed call answers while it is the batch's last seed call (last_seed); the others answer
// while their timer says that stages ran.  A stage that did not run reads 0.
struct Report {
    StageTimer rrt_batch::*time;     // the timer of the family's own stages
    int own;                         // how many those are
    bool seed;                       // the three stages of the seed follow them (seed_time)
    int64_t (rrt_batch::*stats)[4];  // the family's counters, or nullptr
    SeedKind kind;                   // the seed call it reports on; none: no seed call, the timer's `ran` says whether there is a call to report on
    const char *stages;              // what a count out of range is told; nullptr: the form has a fixed size
    const char *refusal;             // what the call is told when there is nothing to report
    const char *after_other;         // rrt_batch_grow_ms alone: ... when another seed call came last
};
// ms[0, 3): edge test, pointer jumping, compaction
static const Report KEEP_TREE{&rrt_batch::keep_time, 3, false, nullptr, SeedKind::none, nullptr,
                              "no rrt_batch_keep_tree on this batch yet, or its last one failed", nullptr};
// ms[0, 3): renumbering and node slots, bitmap, cell records
static const Report GROW{&rrt_batch::seed_time, 0, true, nullptr, SeedKind::grow, "the seed has 3 stages",
                         "no rrt_batch_grow on this batch yet, or its last one failed", "a reroot or a relax came after the last rrt_batch_grow on this batch"};
// ms[0, 5): path, edge test, alive and depth, order, costs; ms[5, 8): the seed's stages, as rrt_batch_grow_ms reports them
static const Report REROOT{&rrt_batch::front_time, 5, true, nullptr, SeedKind::reroot, "a re-root has 5 stages and its seed 3",
                           "no rrt_batch_reroot on this batch yet, its last one failed, or a grow came after it", nullptr};
// ms[0, 6): buckets, rounds, parents, alive and depth, order, costs; ms[6, 9): the seed's stages.  A batch is a Dubins batch or not for
// life, so the kind, the timer and the counters of a batch belong to one of the two calls: each row names its own.
static const Report RELAX{&rrt_batch::front_time, 6, true, &rrt_batch::front_stats, SeedKind::relax, "a relax has 6 stages and its seed 3",
                          "no rrt_batch_relax on this batch yet, its last one failed, or a grow or a reroot came after it", nullptr};
static const Report RELAX_POSES{&rrt_batch::front_time, 6, true, &rrt_batch::front_stats, SeedKind::relax, "a relax has 6 stages and its seed 3",
                                "no rrt_batch_relax_poses on this batch yet, its last one failed, or a grow or a reroot came after it", nullptr};
// ms[0, 7): buckets, start, rounds, parents, alive and depth, order, costs; ms[7, 10): the seed's stages
static const Report REROOT_POSES{&rrt_batch::front_time, 7, true, &rrt_batch::front_stats, SeedKind::reroot_poses, "a pose re-root has 7 stages and its seed 3",
                                 "no rrt_batch_reroot_poses on this batch yet, its last one failed, or another seed call came after it", nullptr};
// ms[0, 4): the decision (the pose goals kernel), depth and scan, rows + legs + lengths (+ the scan of the point counts), the points (0 for
// a call without points, or without a point)
static const Report POSE_ROUTES{&rrt_batch::pose_route_time, 4, false, nullptr, SeedKind::none, nullptr,
                                "no rrt_batch_pose_routes with a pose on this batch yet, or its last one failed", nullptr};
// ms[0, 5): the decision, depth and scan, rows + shortcuts + scan + pack, legs + lengths (+ the scan of the point counts), the points
static const Report POSE_SHORTCUTS{&rrt_batch::pose_cut_time, 5, false, nullptr, SeedKind::none, nullptr,
                                   "no rrt_batch_pose_shortcuts with a pose on this batch yet, or its last one failed", nullptr};
// ms[0, 4): buckets, decide, remap, read-back (both fields)
static const Report COST_FIELD{&rrt_batch::field_time, 4, false, &rrt_batch::field_stats, SeedKind::none, nullptr,
                               "no rrt_batch_cost_field on this batch yet, or its last one failed", nullptr};
static const Report POSE_FIELD{&rrt_batch::pose_field_time, 4, false, &rrt_batch::pose_field_stats, SeedKind::none, nullptr,
                               "no rrt_batch_pose_field on this batch yet, or its last one failed", nullptr};

static int refuse_report(const char *who, const Report &r, rrt_batch *b) {
    if (r.kind == SeedKind::none ? (b->*r.time).ran != 0 : b->last_seed == r.kind) return RRT_OK;
    return fail(b->ctx, RRT_E_ARG, "%s: %s", who, r.after_other && b->last_seed != SeedKind::none ? r.after_other : r.refusal);
}

// ms[0, count): the family's own stages, then the seed's; a form of fixed size passes its size
static int report_ms(const char *who, const Report &r, rrt_batch *b, float *ms, int32_t count) {
    if (!b || !ms) return fail(nullptr, RRT_E_ARG, "%s: NULL", who);
    if (r.stages && (count < 1 || count > r.own + (r.seed ? 3 : 0))) return fail(b->ctx, RRT_E_ARG, "%s: count=%d, %s", who, count, r.stages);
    if (const int rc = refuse_report(who, r, b)) return rc;
    if (r.own) HIPCHK(b->ctx, (b->*r.time).read(ms, std::min(count, r.own)));
    if (count > r.own) HIPCHK(b->ctx, b->seed_time.read(ms + r.own, count - r.own));
    return RRT_OK;
}

static int report_stats(const char *who, const Report &r, rrt_batch *b, int64_t out[4]) {
    if (!b || !out) return fail(nullptr, RRT_E_ARG, "%s: NULL", who);
    if (const int rc = refuse_report(who, r, b)) return rc;
    for (int k = 0; k < 4; ++k) out[k] = (b->*r.stats)[k];
    return RRT_OK;
}

// the rrt_plan_ form of a report: the rrt_batch_ form on the batch behind rrt_plan, in that form's words
template <typename... Args>
static int plan_report(const char *who, rrt_ctx *ctx, int (*batch_form)(rrt_batch *, Args...), Args... args) {
    rrt_batch *s = plan_batch(ctx, who, NO_PLAN);
    return s ? batch_form(s, args...) : RRT_E_ARG;
}

extern "C" int rrt_batch_keep_tree_ms(rrt_batch *b, float ms[3]) { return report_ms("rrt_batch_keep_tree_ms", KEEP_TREE, b, ms, 3); }
extern "C" int rrt_plan_keep_tree_ms(rrt_ctx *ctx, float ms[3]) { return plan_report("rrt_plan_keep_tree_ms", ctx, rrt_batch_keep_tree_ms, ms); }
extern "C" int rrt_batch_grow_ms(rrt_batch *b, float *ms, int32_t count) { return report_ms("rrt_batch_grow_ms", GROW, b, ms, count); }
extern "C" int rrt_plan_grow_ms(rrt_ctx *ctx, float *ms, int32_t count) { return plan_report("rrt_plan_grow_ms", ctx, rrt_batch_grow_ms, ms, count); }
extern "C" int rrt_batch_reroot_ms(rrt_batch *b, float *ms, int32_t count) { return report_ms("rrt_batch_reroot_ms", REROOT, b, ms, count); }
extern "C" int rrt_plan_reroot_ms(rrt_ctx *ctx, float *ms, int32_t count) { return plan_report("rrt_plan_reroot_ms", ctx, rrt_batch_reroot_ms, ms, count); }
extern "C" int rrt_batch_relax_ms(rrt_batch *b, float *ms, int32_t count) { return report_ms("rrt_batch_relax_ms", RELAX, b, ms, count); }
extern "C" int rrt_plan_relax_ms(rrt_ctx *ctx, float *ms, int32_t count) { return plan_report("rrt_plan_relax_ms", ctx, rrt_batch_relax_ms, ms, count); }
extern "C" int rrt_batch_relax_stats(rrt_batch *b, int64_t out[4]) { return report_stats("rrt_batch_relax_stats", RELAX, b, out); }
extern "C" int rrt_plan_relax_stats(rrt_ctx *ctx, int64_t out[4]) { return plan_report("rrt_plan_relax_stats", ctx, rrt_batch_relax_stats, out); }
extern "C" int rrt_batch_relax_poses_ms(rrt_batch *b, float *ms, int32_t count) { return report_ms("rrt_batch_relax_poses_ms", RELAX_POSES, b, ms, count); }
extern "C" int rrt_plan_relax_poses_ms(rrt_ctx *ctx, float *ms, int32_t count) {
    return plan_report("rrt_plan_relax_poses_ms", ctx, rrt_batch_relax_poses_ms, ms, count);
}
extern "C" int rrt_batch_relax_poses_stats(rrt_batch *b, int64_t out[4]) { return report_stats("rrt_batch_relax_poses_stats", RELAX_POSES, b, out); }
extern "C" int rrt_plan_relax_poses_stats(rrt_ctx *ctx, int64_t out[4]) {
    return plan_report("rrt_plan_relax_poses_stats", ctx, rrt_batch_relax_poses_stats, out);
}
extern "C" int rrt_batch_reroot_poses_ms(rrt_batch *b, float *ms, int32_t count) { return report_ms("rrt_batch_reroot_poses_ms", REROOT_POSES, b, ms, count); }
extern "C" int rrt_plan_reroot_poses_ms(rrt_ctx *ctx, float *ms, int32_t count) {
    return plan_report("rrt_plan_reroot_poses_ms", ctx, rrt_batch_reroot_poses_ms, ms, count);
}
extern "C" int rrt_batch_reroot_poses_stats(rrt_batch *b, int64_t out[4]) { return report_stats("rrt_batch_reroot_poses_stats", REROOT_POSES, b, out); }
extern "C" int rrt_plan_reroot_poses_stats(rrt_ctx *ctx, int64_t out[4]) {
    return plan_report("rrt_plan_reroot_poses_stats", ctx, rrt_batch_reroot_poses_stats, out);
}
extern "C" int rrt_batch_pose_routes_ms(rrt_batch *b, float ms[4]) { return report_ms("rrt_batch_pose_routes_ms", POSE_ROUTES, b, ms, 4); }
extern "C" int rrt_plan_pose_routes_ms(rrt_ctx *ctx, float ms[4]) { return plan_report("rrt_plan_pose_routes_ms", ctx, rrt_batch_pose_routes_ms, ms); }
extern "C" int rrt_batch_pose_shortcuts_ms(rrt_batch *b, float ms[5]) { return report_ms("rrt_batch_pose_shortcuts_ms", POSE_SHORTCUTS, b, ms, 5); }
extern "C" int rrt_plan_pose_shortcuts_ms(rrt_ctx *ctx, float ms[5]) { return plan_report("rrt_plan_pose_shortcuts_ms", ctx, rrt_batch_pose_shortcuts_ms, ms); }
extern "C" int rrt_batch_cost_field_ms(rrt_batch *b, float ms[4]) { return report_ms("rrt_batch_cost_field_ms", COST_FIELD, b, ms, 4); }
extern "C" int rrt_plan_cost_field_ms(rrt_ctx *ctx, float ms[4]) { return plan_report("rrt_plan_cost_field_ms", ctx, rrt_batch_cost_field_ms, ms); }
extern "C" int rrt_batch_cost_field_stats(rrt_batch *b, int64_t out[4]) { return report_stats("rrt_batch_cost_field_stats", COST_FIELD, b, out); }
extern "C" int rrt_plan_cost_field_stats(rrt_ctx *ctx, int64_t out[4]) { return plan_report("rrt_plan_cost_field_stats", ctx, rrt_batch_cost_field_stats, out); }
extern "C" int rrt_batch_pose_field_ms(rrt_batch *b, float ms[4]) { return report_ms("rrt_batch_pose_field_ms", POSE_FIELD, b, ms, 4); }
extern "C" int rrt_plan_pose_field_ms(rrt_ctx *ctx, float ms[4]) { return plan_report("rrt_plan_pose_field_ms", ctx, rrt_batch_pose_field_ms, ms); }
extern "C" int rrt_batch_pose_field_stats(rrt_batch *b, int64_t out[4]) { return report_stats("rrt_batch_pose_field_stats", POSE_FIELD, b, out); }
extern "C" int rrt_plan_pose_field_stats(rrt_ctx *ctx, int64_t out[4]) { return plan_report("rrt_plan_pose_field_stats", ctx, rrt_batch_pose_field_stats, out); }
