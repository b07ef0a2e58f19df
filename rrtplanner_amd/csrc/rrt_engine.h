// rrt_engine.h -- private to the two host units of librrt_hip.so (rrt_engine.hip, rrt_tree_calls.hip): the context and the batch behind
// the handles of include/rrt_hip.h, and the functions of the engine that the tree calls use.
#pragma once
#define RRT_PRIVATE __attribute__((visibility("hidden")))  // shared by the two units, not exported by the library
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is opened on demand (rrt_comm_init), the single-GPU path never loads it
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

// The kernels are only LAUNCHED from the host units, through the declarations of rrt_kernel_abi.h; kernels_tu.hip holds their
// definitions, dealt to several translation units that compile side by side (the single unit of round 3 took two and a half minutes).
// (The engine's own small kernels -- init, primitives, tree query, noise, slab meta -- are rrt_engine.hip's: rrt_prims.h and the file itself.)
#include "rrt_hip.h"
#include "rrt_kernel_abi.h"
#include "rrt_block_variants.def"
#include "rrt_scratch.h"

using namespace rrtdev;

// Host copy of a batch's query descriptors in page-locked memory: the per-step copies to and from the device (rrt_batch_rearm,
// rrt_batch_sync) are then plain DMA transfers in stream order, with no staging copy and no hidden synchronisation.
struct PinnedDescs {
    QDesc *p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        release();
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(QDesc), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = count;
        for (size_t k = 0; k < n; ++k) p[k] = QDesc{};
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    QDesc *data() { return p; }
    QDesc *begin() { return p; }
    QDesc *end() { return p + n; }
    QDesc &operator[](size_t k) { return p[k]; }
};

struct rrt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // pipelined teams of 8 and more: the committers' kernel runs here, next to the workers' on `stream`
    uint8_t *og = nullptr;      // active grid, device (W,H): og_buf + frame * W * H
    uint8_t *og_buf = nullptr;  // allocation holding 1 uploaded grid or `nframes` generated grids
    size_t og_buf_bytes = 0;
    int32_t nframes = 1;
    int32_t W = 0, H = 0;
    std::string err;
    rrt_batch *single = nullptr;  // batch behind rrt_plan / rrt_plan_resume
    uint32_t single_flags = 0;
    int max_lds = 0;
    int num_cu = 0;
    uint64_t grid_gen = 0;  // bumped by every call that rewrites or reallocates og_buf (rrt_set_grid, rrt_noise_grids)
    // multi-GPU result gather (RCCL over xGMI); all null / 1 until rrt_comm_init
    ncclComm_t comm = nullptr;
    int32_t comm_rank = 0, comm_world = 1;
    unsigned char *gather_buf = nullptr;  // [world][slab bytes of the batch gathered last]
    size_t gather_bytes = 0;
    const rrt_batch *gather_owner = nullptr;  // the batch whose slabs gather_buf holds (rrt_gather_fetch serves no other)
    double *d_red = nullptr;  // small device scratch of rrt_comm_allreduce_f64
};

typedef void (*block_kernel_fn)(BatchView);
struct BlockVariant;  // a row of the engine's table of team kernels (rrt_engine.hip)

// What one launch decided (plan_launch).  The batch keeps the plan of its last launch for the questions asked afterwards
// (rrt_batch_kernel_name, rrt_batch_team_info, rrt_batch_pipelined, the continuation in rrt_batch_sync).
struct LaunchPlan {
    int team = 0;               // workers per query (1 after a hand-off timed out; 0: nothing launched yet)
    int qpad = 0;               // block = member * qpad + query
    int shifts = 1;             // worker shifts of the split team of 64: 2 = 128 workers, each shift takes every other block
    bool pipe = false;          // the pipelined team kernel: one more workgroup per query, which only commits
    bool inf = false;           // the Informed instantiation
    bool wide = false;          // a team variant with more than 16 samples per member
    bool split = false;         // committers and workers as two kernels (rrt_block_commit_kernel + rrt_block_work_kernel)
    bool pipe1 = false;         // the barrier-free one-CU kernel (rrt_pipe.h)
    bool large = false;         // ... in its form for grids up to 4096 x 4096 (RRT_FLAG_LARGE_GRID: the only kernel such a batch runs)
    bool continuation = false;  // of a launch that stopped at a block boundary: one CU per query, and the block kernel takes it from there
    const BlockVariant *row = nullptr;  // the team variant, or nullptr for a kernel that is none (pipe1, Dubins, one sample per iteration)
    block_kernel_fn kern = nullptr;     // the kernel of a launch that is one kernel (row->one, or the plain kernel)
    unsigned grid = 0;          // its workgroups (split: qpad committers, qpad * team workers)
    int lds_chunks = 1;         // node chunks cached in LDS
    size_t lds_bytes = 0;       // dynamic LDS per workgroup
};

// Grow-only device scratch: a pointer and its capacity in the caller's units (goals, slabs, rows, vertices).
struct RRT_PRIVATE DevBuf {
    void *p = nullptr;
    int64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    // Room for `want` units, which take `bytes`; while cap >= want nothing happens, otherwise what the buffer held is gone.  The pointer
    // is cleared before it is freed and the capacity recorded last: after a failure at any step the pointer is null or valid, never
    // freed twice, and cap is never more than what is allocated.
    hipError_t reserve(int64_t want, size_t bytes) {
        if (want <= cap) return hipSuccess;
        void *old = p;
        p = nullptr;
        cap = 0;
        hipError_t e = old ? hipFree(old) : hipSuccess;
        if (e == hipSuccess) e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
    template <typename T>
    T *as() const {
        return static_cast<T *>(p);
    }
    // A buffer of several arrays (rrt_scratch.h): room for `want` units of Layout, whose constructor says how many bytes that is,
    // and the arrays of what is allocated.  A buffer is carved by its capacity, never by the count of the call at hand.
    template <typename Layout, typename... Extra>
    hipError_t reserve(int64_t want, Extra... extra) {
        return reserve(want, Layout(nullptr, (size_t)want, extra...).bytes);
    }
    template <typename Layout, typename... Extra>
    Layout carve(Extra... extra) const {
        return Layout(p, (size_t)cap, extra...);
    }
};

// The kernel times of the stages of a call.  The call records marks (events, created by the first call) on its stream; the timer's
// table says between which two marks each stage lies, so that stages may share a mark or have a pair each.
constexpr int STAGE_MARKS = 10;
constexpr int STAGES_IN_A_ROW[][2] = {{0, 1}, {1, 2}, {2, 3}};               // four marks around three stages
constexpr int STAGES_IN_A_LONG_ROW[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}};  // up to eight marks around seven stages
constexpr int STAGES_IN_PAIRS[][2] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {8, 9}};  // a pair around each stage
struct RRT_PRIVATE StageTimer {
    const int (*stages)[2];
    hipEvent_t ev[STAGE_MARKS] = {};
    int ran = 0;  // stages of the last successful call that ran, the table's first ones; 0: no call yet, or the last one failed
    explicit StageTimer(const int (*stages_)[2]) : stages(stages_) {}
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // the first n marks exist: a call makes sure of it before it records any, so that no stage has the creation of an event in it
    hipError_t create(int n) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < n && e == hipSuccess; ++k)
            if (!ev[k]) e = hipEventCreate(&ev[k]);
        return e;
    }
    hipError_t mark(int k, hipStream_t stream) { return hipEventRecord(ev[k], stream); }
    // ms[0, count): the time of every stage that ran, 0 for one that did not
    hipError_t read(float *ms, int count) const {
        hipError_t e = hipSuccess;
        for (int k = 0; k < count && e == hipSuccess; ++k) {
            ms[k] = 0.f;
            if (k < ran) e = hipEventElapsedTime(&ms[k], ev[stages[k][0]], ev[stages[k][1]]);
        }
        return e;
    }
};

// the seed calls of a batch, as its last_seed names the one that succeeded last (relax: rrt_batch_relax and rrt_batch_relax_poses, of
// which a batch only ever takes one: it is a Dubins batch or not for life)
enum class SeedKind { none, grow, reroot, relax, reroot_poses };

struct rrt_batch {
    rrt_ctx *ctx = nullptr;
    int32_t Q = 0, n_cap = 0, node_stride = 0, bitmap_words = 0, lds_chunks = 1, spill_stride = 0;
    int32_t spill_stride2 = 0;  // the stride a launch on two shifts carves the spill area by (129 members; 0: the batch has no room for two shifts)
    int32_t gridW = 0, gridH = 0;
    uint32_t flags = 0;
    bool use_block = false;     // block-parallel kernel (rrt_block.h) instead of the one-sample-per-iteration kernel
    bool dub_block = false;     // Dubins planners on the 16-samples-per-round kernel (rrt_dubins_block.h); RRT_FLAG_SERIAL keeps the one-sample kernel
    int32_t blk_lds_chunks = 1; // node chunks cached in LDS by the block kernel: teams of 8 and more workers ...
    int32_t blk_lds_chunks16 = 1; // ... and the kernels that also keep their parked-entry lists there
    int32_t team = 1;           // workgroups (CUs) per query of the block kernel that scan and resolve (rrt_block.h, teams)
    bool pipe_team = false;     // the team is pipelined: one more workgroup per query, which only commits
    int32_t shifts_room = 1;    // fixed at rrt_batch_create: 2 = two shifts of `team` workers fit (no cap from the caller, a team of 64 + 1, 129 CUs per query)
    int32_t shifts = 1;         // what a launch asks for and rrt_batch_team reports: shifts_room, or 1 while an Informed query is set (rrt_batch_set_query recomputes it)
    LaunchPlan last;            // the plan of the last launch
    int32_t team_fallbacks = 0; // launches repeated with one CU per query after a team hand-off timed out
    int32_t team_qpad = 0;      // Q rounded up to a multiple of 8: block = member * team_qpad + query
    int32_t team_want = TEAM_MAX;  // the caller's cap on the team size
    int32_t claimed_cus = 0;    // compute units this batch's launch in flight holds in the device's registry (0: nothing in flight)
    int32_t shrunk = 0;         // launches that ran fewer workers than the batch was created with (a smaller team, or one shift of two) because other launches held CUs
    unsigned char *d_team = nullptr;  // [Q][TEAM_BYTES] sync words, state, exchanged records; zeroed before every launch
    QDesc *d_desc = nullptr;
    PinnedDescs h_desc;  // page-locked
    size_t serial_lds_static = 0;  // static LDS of the one-sample-per-iteration kernel + 1 (0 = not asked yet)
    uint32_t *d_samples = nullptr, *d_nodes = nullptr, *d_bitmap = nullptr;
    double *d_vcost = nullptr, *d_unitball = nullptr, *d_cbest_log = nullptr;
    int32_t *d_parent = nullptr, *d_nearest_log = nullptr, *d_j_log = nullptr;
    uint8_t *d_accept_log = nullptr;
    uint2 *d_spill = nullptr;
    int32_t *d_kids = nullptr;      // RRT_FLAG_REWIRE: [3][Q][node_stride] first child / next sibling / previous sibling
    uint32_t *d_frontier = nullptr; //                  [Q][2 * node_stride]
    int32_t *d_vsoln = nullptr;     //                  [Q][node_stride]
    uint8_t *d_heading = nullptr;   // RRT_FLAG_DUBINS: [Q][node_stride] node headings
    uint8_t *d_shead = nullptr;     //                  [Q][n_cap] sample headings
    double *d_dubpath = nullptr;    //                  [Q][NWAVE * WCAP][5] the words of the current iteration's near-set entries
    std::vector<uint8_t> stage8;
    uint4 *d_cellrec = nullptr;    // block kernel: near-set records, [Q][rec_stride]
    uint32_t *d_cellcnt = nullptr; // [Q][MAX_CELLS]
    int64_t rec_stride = 0;
    unsigned char *d_slab = nullptr;  // result slab: [vcost f64 | nodes u32 | parent i32], each [Q][node_stride]
    size_t slab_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;  // the split team kernels: stream -> stream2 behind the init kernel, back in front of ev1
    bool timed = false;
    float ms_before = 0.f;      // kernel time of the launch a fallback relaunch replaced (rrt_batch_elapsed_ms adds it)
    bool one_cu_once = false;   // the next launch runs one CU per query whatever b->team says (continuation after a timeout)
    std::vector<uint32_t> stage;  // host staging for packed samples
    // the goals and poses calls: the grid every query last ran on (recorded at launch), and scratch allocated at the first call and
    // grown by later ones (rrt_goals.h, rrt_pose_goals.h: a batch is a Dubins batch or not for life, so the two calls share it)
    std::vector<uint64_t> ran_gen;       // [Q] the context's grid generation
    std::vector<const uint8_t *> ran_og; // [Q] ... and its active grid
    DevBuf goal_order;                   // u32 [slabs][n_cap] the sorted vertex order, one slab per workgroup (never `spill`: a later launch needs it)
    DevBuf goal_xy;                      // u32 [goals] packed goal cells
    DevBuf goal_vertex;                  // i32 [goals]
    DevBuf goal_cost;                    // f64 [goals]
    DevBuf pose_h;                       // u8  [goals] rrt_batch_connect_poses: goal heading indices
    DevBuf pose_counts;                  // u32 [goals][2] ... words evaluated, sweeps run
    int32_t pose_last_m = -1;            // goals of the last successful rrt_batch_connect_poses; -1: none
    // rrt_batch_routes: per-goal arrays and the rows of the routes (rrt_routes.h)
    DevBuf route_goal;                   // RouteGoalScratch
    DevBuf route_row;                    // RouteRowScratch
    int64_t route_rows = -1;             // dense rows the last rrt_batch_routes left for rrt_batch_routes_rows; -1: none (launch, rearm)
    // rrt_batch_pose_routes: per-goal arrays, per-row arrays, the legs' sweeps and the points (rrt_pose_routes.h).  The last two are
    // allocated by the first call that asks for points.
    DevBuf pose_route_goal;              // PoseRouteGoalScratch
    DevBuf pose_route_row;               // PoseRouteRowScratch
    DevBuf pose_route_sweep;             // dub_sweep_t [rows]
    DevBuf pose_route_pts;               // f64 [points][2]
    int64_t pose_route_rows = -1;        // rows the last rrt_batch_pose_routes / rrt_batch_pose_shortcuts left for rrt_batch_pose_routes_rows; -1: none (launch, rearm, keep, grow)
    int64_t pose_route_points = -1;      // ... and points for rrt_batch_pose_routes_points; -1: none, or that call did not ask for points
    StageTimer pose_route_time{STAGES_IN_PAIRS};  // its four stages; 3 ran: no points
    // rrt_batch_pose_shortcuts: rrt_batch_pose_routes with the shortcut pass.  It shares everything above but the stage times (its rows
    // and points are what pose_route_rows / pose_route_points count), and adds the raw rows that the pass rewrites in place.
    DevBuf pose_cut_goal;                // PoseCutGoalScratch
    DevBuf pose_cut_row;                 // PoseCutRowScratch
    StageTimer pose_cut_time{STAGES_IN_PAIRS};  // its five stages; 4 ran: no points
    // rrt_batch_keep_tree / rrt_batch_keep_pose_tree: the views of the queries that were kept on a new map (rrt_keep.h, rrt_pose_keep.h),
    // allocated at the first call per query
    std::vector<DevBuf> keep;            // [Q] empty, or KeepScratch of n_cap vertices
    std::vector<int32_t> keep_alive;     // [Q] vertices of the view; -1: no view, the goals and routes calls see the whole tree
    DevBuf keep_tmp;                     // KeepTmpScratch of n_cap vertices
    StageTimer keep_time{STAGES_IN_A_ROW};  // the three stages of the last rrt_batch_keep_tree
    // rrt_batch_grow: a query armed as a loop stopped mid-way runs with D->n = j0 + m (rrt_seed.h)
    std::vector<int32_t> grow_n;            // [Q] the query's own n while it is armed so; -1 otherwise (rrt_batch_sync puts it back)
    std::vector<uint64_t> grow_gen;         // [Q] while it is armed so: the grid generation the seed was built on (rrt_batch_launch asks for it)
    std::vector<const uint8_t *> grow_og;   // [Q] ... and that grid
    DevBuf seed_tmp;                        // SeedTmpScratch of n_cap vertices
    // The seed calls all end in that seed, so the batch keeps once what the last successful one left: which it was (none from where a
    // seed call starts replacing the query until it has armed it; the report calls answer for that kind alone), and the times of ...
    SeedKind last_seed = SeedKind::none;
    StageTimer seed_time{STAGES_IN_A_ROW};        // ... the three stages of its seed
    StageTimer front_time{STAGES_IN_A_LONG_ROW};  // ... its stages in front of the seed: the five of reroot, the six of relax / relax_poses, the seven of reroot_poses
    // ... and its counters: of a relax rounds run, vertices whose cost fell, lines of sight walked, pairs priced (a Dubins batch: sweeps
    // run, words evaluated); of a pose re-root rounds run, vertices reached, sweeps run, words evaluated
    int64_t front_stats[4] = {0, 0, 0, 0};
    DevBuf reroot_tmp;       // rrt_batch_reroot (rrt_reroot.h): RerootScratch of n_cap vertices
    DevBuf relax_tmp;        // rrt_batch_relax (rrt_relax.h; it works in reroot_tmp too): RelaxScratch of n_cap vertices and RELAX_MAX_CELLS cells
    DevBuf pose_relax_tmp;   // rrt_batch_relax_poses (a Dubins batch, rrt_pose_relax.h): PoseRelaxScratch of n_cap vertices beside the two
    DevBuf pose_reroot_tmp;  // rrt_batch_reroot_poses (a Dubins batch, rrt_pose_reroot.h): the root-first input beside the three, PoseRerootScratch of n_cap vertices
    // rrt_batch_cost_field: the buckets of the call (rrt_field.h); the answers of the window go through goal_vertex / goal_cost
    DevBuf field_tmp;                             // FieldScratch of n_cap vertices and RELAX_MAX_CELLS cells
    StageTimer field_time{STAGES_IN_A_LONG_ROW};  // the four stages of the last rrt_batch_cost_field: buckets, decide, remap, read-back
    int64_t field_stats[4] = {0, 0, 0, 0};        // of that call: free cells decided, buckets visited, vertices priced, lines walked
    // rrt_batch_pose_field (a Dubins batch, rrt_pose_field.h): its buckets are a FieldScratch in field_tmp, which no other call of a Dubins
    // batch uses, and the heading byte of every item is PoseRelaxScratch's item_h in pose_relax_tmp, which relax_poses and reroot_poses
    // fill anew in every call of theirs; the vertex and the cost of the window go through goal_vertex / goal_cost
    DevBuf pose_field_heading;                         // i32 [cells of the window] the arrival heading of every answer
    StageTimer pose_field_time{STAGES_IN_A_LONG_ROW};  // the four stages of the last rrt_batch_pose_field: buckets, decide, remap, read-back
    int64_t pose_field_stats[4] = {0, 0, 0, 0};        // of that call: free cells decided, buckets visited, words evaluated, sweeps run
    // the rows and points an earlier routes call left are gone (a launch, a rearm, a keep, a grow: they belong to another tree or view)
    void drop_routes() { route_rows = pose_route_rows = pose_route_points = -1; }
};

// ---- defined in rrt_engine.hip ----
RRT_PRIVATE int fail(rrt_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));  // the message recorded, `code` returned
RRT_PRIVATE void arm_desc(QDesc &d);
RRT_PRIVATE void drop_keep_views(rrt_batch *b, int32_t q = -1);  // no query of the batch has a kept view any more, or only query q
RRT_PRIVATE int run_single(rrt_ctx *ctx, rrt_result *out);       // launch, sync and result of the batch behind rrt_plan

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) return fail(ctx, RRT_E_HIP, "%s: %s", #call, hipGetErrorString(e_));     \
    } while (0)

// Wait for the context's stream by polling (no interrupt wake-up of a sleeping host thread: on a host that parks the waiting
// thread the default wait costs up to a millisecond per step, against a 9 ms launch).  A wait that lasts longer than
// `spin_ms` falls through to the blocking wait, where the wake-up no longer matters and a spinning core would.
static hipError_t wait_stream_spin(hipStream_t stream, double spin_ms = 100.0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        const hipError_t e = hipStreamQuery(stream);
        if (e != hipErrorNotReady) return e;
        if ((it & 1023u) == 1023u && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > spin_ms)
            return hipStreamSynchronize(stream);
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
}
