// rrt_kernel_abi.h -- what the host units (rrt_engine.hip, rrt_tree_calls.hip) and the kernel units (kernels_tu.hip) share, and nothing
// else: the structs a kernel takes by value, the constants the engine sizes buffers and launches by, and a declaration of every kernel
// a host unit launches.  The definitions live in the kernel files (one per unit of kernels_tu.hip); no host unit includes those.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rrtdev {

constexpr int TPB = 1024;          // threads of one query workgroup (16 waves, one CU)
constexpr int NWAVE = TPB / 64;
constexpr int CHUNK = TPB * 4;     // nodes per scan chunk: one 16-byte load per thread
constexpr int MAX_LDS_CHUNKS = 8;  // node chunks cached in LDS (8 * 16 KiB = 128 KiB)
constexpr int WSLOTS = 3;          // near-set entries a lane prices in registers
constexpr int WCAP = 64 * WSLOTS;  // near-set entries per wave in LDS (16 waves * 1.5 KiB)
constexpr uint32_t NONE = 0xffffffffu;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#ifndef RRT_TS_BASE
#define RRT_TS_BASE 300  // diagnostic build: QDesc::ts holds the stamps of the 32 blocks of a run from this one on (TSMARK, rrt_block.h)
#endif

enum : int32_t { ST_DONE = 0, ST_NEED_UB = 1, ST_UNREACHABLE = -2, ST_TEAM_FAIL = -3, ST_RUNNING = 100, ST_IDLE = 101 };

// Per-query descriptor in HBM: inputs, resumable loop state, statistics.
struct QDesc {
    int32_t alg, n;
    int32_t xs[2], xg[2];
    uint32_t r2_rewire, goal_d2;
    double C[4];
    int32_t ub_offset, ub_count;
    int32_t cell_shift, ncx, ncy, cell_cap;  // block kernel: near-set record grid of this query (cell = 2^shift pixels)
    int32_t status, i, j, nsoln, vbest_soln, vgoal, found, i_switch;
    double cmin_soln;
    unsigned long long sum_j, sum_cells_nn, sum_near, sum_cells_cand, n_los_cand;
    unsigned long long wcyc[32]; // diagnostic build: per-wave cycles in the block kernel's owner phase [0..15] and its LoS part [16..31]
    unsigned long long cyc[6];  // diagnostic build (-DRRT_STAMPS): wave-0 cycles in scan / pre-barrier / barrier / B+C / D / go2goal
    unsigned long long n_rewired, n_propagated;  // opt-in true rewire (RRT_FLAG_REWIRE): nodes re-parented, descendant costs recomputed
    double rho;          // Dubins planners (alg 3 / 4): turning radius in cells, number of headings, start / goal heading index
    int32_t nh, hs, hg, pad_;
    unsigned long long n_words;  // Dubins planners: dub_shortest() evaluations made (the byte / flop model counts one per near-set entry)
#ifdef RRT_STAMPS
    // diagnostic build, pipelined teams: per worker m = member - 1: [m] polls of the committer's record fetch during which m's records were
    // still missing, [64 + m] blocks in which m was the LAST to arrive, [128 + m] the worker's own cycles in its resolve phase
    unsigned long long dbg2[448];  // (+ [192 + m], [256 + m], [320 + m]: blocks whose resolve phase took m more than 26 k / 32 k / 40 k cycles, [384 + m]: its longest)
    unsigned long long ts[32 * 16];  // wall-clock (10 ns) time stamps of 32 consecutive blocks, 16 events each (rrt_block.h: TSMARK)
#endif
};

struct BatchView {
    QDesc *desc;
    const uint32_t *samples;  // [Q][n_cap]         packed free-space samples
    uint32_t *nodes;          // [Q][node_stride]   packed tree nodes
    double *vcost;            // [Q][node_stride]
    int32_t *parent;          // [Q][node_stride]
    uint32_t *bitmap;         // [Q][bitmap_words]  `sampled` set (rrt.py:407)
    uint2 *spill;             // [Q][spill_stride]  per-wave near-set overflow / go2goal costs
    const double *unitball;   // [Q][2*n_cap] or null
    int32_t *nearest_log;     // optional logs [Q][n_cap]
    uint8_t *accept_log;
    double *cbest_log;
    int32_t *j_log;
    const uint8_t *og;        // (W,H) x-major occupancy, != 0 is obstacle
    int32_t W, H;
    int32_t n_cap, node_stride, bitmap_words, lds_chunks, spill_stride;
    uint4 *cellrec;           // [Q][rec_stride]    block kernel: per-cell arrays of {xy, index, vcost} records
    uint32_t *cellcnt;        // [Q][MAX_CELLS]     fill counts of the cells
    int64_t rec_stride;
    unsigned char *team;      // [Q][TEAM_BYTES]    block kernel with teams: sync words, state, exchanged records
    int32_t Q, team_qpad;     // queries of the batch; block stride between the members of a team (block = member * team_qpad + query)
    int32_t team_fault;       // testing: member 1 of every team leaves at once (the others' hand-offs time out)
    int32_t member0;          // added to the member number a team kernel derives from its block index (1: a launch of the workers only)
    int32_t shifts;           // worker shifts of a split team of 64 (rrt_block.h, "shifts"): 2 = members 1..64 take the odd blocks, 65..128 the even ones
    // opt-in true rewire (RRT_FLAG_REWIRE; serial kernel only), null otherwise
    int32_t *kid_first, *kid_next, *kid_prev;  // [Q][node_stride] child lists: first child, next / previous sibling (-1 = none)
    uint32_t *frontier;                        // [Q][2 * node_stride] two propagation frontiers
    int32_t *vsoln;                            // [Q][node_stride] Informed: solution vertices in insertion order
    // Dubins planners (RRT_FLAG_DUBINS; serial kernel only), null otherwise
    uint8_t *heading;               // [Q][node_stride] heading index of every node
    const uint8_t *sample_heading;  // [Q][n_cap]       heading index of sample i
    double *dub_path;               // [Q][NWAVE * WCAP][5] {t, p, q, len, word} of every priced near-set entry of the current iteration
};

constexpr int BLOCK_LIST_CAP = 256;                                  // block kernel, one wave per sample: parked entries per wave kept in LDS
constexpr size_t BLOCK_LIST_LDS_BYTES = (size_t)NWAVE * BLOCK_LIST_CAP * 16;  // 64 KiB
constexpr int MAX_CELLS = 4096;  // cells per query (their fill counts live in LDS: 16 KiB)

// ---- the team area of a query (rrt_block.h, "teams"): what a record carries decides its size ----
constexpr int TEAM_MAX = 64;
#ifndef RRT_NPMAX
#define RRT_NPMAX 2  // most blocks in flight a record can carry interaction masks for (>= both RRT_PIPE_LAG values)
#endif
constexpr int NPMAX = RRT_NPMAX;
// Owners on big teams (a group of waves per sample) also test the lines of sight from every sample IN FLIGHT within r_rewire to
// their sample -- positions come from the sample stream, not from the tree -- and hand the answers over as a list of up to PL_MAX
// 16-bit entries, so that the committer settles "an inserted sample in flight is a cheaper parent" (nine in ten of the samples a
// commit has to look at again) lane-parallel, without a line-of-sight test of its own.  Entry: bits 0-5 sample, 6-7 set (0 = oldest
// previous block ... NP = this block), 8-14 cells the test read, 15 free; order: oldest block first, sample order = node order.
#ifndef RRT_PL_MAX
#define RRT_PL_MAX 12
#endif
constexpr int PL_MAX = RRT_PL_MAX, PL_WORDS = (RRT_PL_MAX + 3) / 4;
constexpr int BREC_WORDS = 10 + 3 * NPMAX + PL_WORDS;  // 8-byte words of an owner's record (BRec, rrt_block.h): 152 bytes for two blocks in flight
// per query: [go | fail | state (NPMAX + 1 slots of 64 bytes) | records (NPMAX + 1 slots of 64) | arrival flags (65 x 128) | go2goal answers (65 x 16)
//             | the second shift's arrival flags (65 x 128: member 64 + m at index m) | its go2goal answers (65 x 16)]
constexpr int TEAM_OFF_GO = 128, TEAM_OFF_FAIL = 256, TEAM_OFF_STATE = 384, TEAM_OFF_REC = 1024;
constexpr int TEAM_OFF_ARRIVE = (TEAM_OFF_REC + (NPMAX + 1) * 64 * BREC_WORDS * 8 + 127) / 128 * 128;
constexpr int TEAM_OFF_RES = TEAM_OFF_ARRIVE + 65 * 128;
constexpr int TEAM_OFF_ARRIVE2 = (TEAM_OFF_RES + 65 * 16 + 1023) / 1024 * 1024;  // (behind everything a one-shift team uses: those offsets stay)
constexpr int TEAM_OFF_RES2 = TEAM_OFF_ARRIVE2 + 65 * 128;
constexpr int TEAM_BYTES = (TEAM_OFF_RES2 + 65 * 16 + 1023) / 1024 * 1024;
static_assert(TEAM_OFF_STATE + (NPMAX + 1) * 64 <= TEAM_OFF_REC, "state slots");

// ---- rrt_goals.h ----
constexpr int GOALS_MAX_SLABS = 512;                    // workgroups of a launch == `order` slabs of n_cap words each
constexpr size_t GOALS_SLAB_BUDGET = (size_t)128 << 20; // bytes of slabs a batch may hold (never fewer than one slab)
constexpr int GOALS_MAX = 1 << 20;                      // goals of one call

struct GoalsView {
    const uint8_t *og;      // (W,H) x-major occupancy, != 0 is obstacle
    int32_t H;
    const uint32_t *nodes;  // the query's packed vertices
    const double *vcost;
    int32_t j;              // vertices considered: [0, j)
    const uint32_t *goals;  // [m] packed like vertices
    int32_t m;
    uint32_t *order;        // [gridDim.x][slab_words] go2goal_phase's scratch, one slab per workgroup
    int32_t slab_words;     // >= j
    int32_t *vertex;        // [m] out: the vertex the goal connects to, or -1
    double *cost;           // [m] out: the cost of the goal through it, or +inf
};

// ---- rrt_pose_goals.h ----
constexpr int POSES_MAX_SLABS = 512;                    // workgroups of a launch == `order` slabs of n_cap words each
constexpr size_t POSES_SLAB_BUDGET = (size_t)128 << 20; // bytes of slabs a batch may hold (never fewer than one slab)
constexpr int POSES_MAX = 1 << 20;                      // goal poses of one call

struct PoseGoalsView {
    const uint8_t *og;       // (W,H) x-major occupancy, != 0 is obstacle
    int32_t W, H;
    const uint32_t *nodes;   // the query's packed vertices
    const double *vcost;
    const uint8_t *heading;  // ... and their heading indices
    int32_t j;               // vertices considered: [0, j)
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    const uint32_t *goals;   // [m] cells packed like vertices
    const uint8_t *goal_h;   // [m] heading indices, < nh
    int32_t m;
    int32_t slab_words;      // >= j
    uint32_t *order;         // [gridDim.x][slab_words] the sorted vertex order, one slab per workgroup
    int32_t *vertex;         // [m] out: the vertex the goal connects to, or -1
    double *cost;            // [m] out: the cost of the goal through it, or +inf
    uint32_t *counts;        // [m][2] out: words evaluated, sweeps run
};

// ---- rrt_routes.h ----
constexpr int ROUTE_TPB = 256;                            // depth, fill and pack: goals per workgroup (lanes), or 4 goals (waves)
constexpr int ROUTE_CUT_MAX_WG = 1024;                    // workgroups of the shortcut kernel, each loops over goals
constexpr size_t ROUTE_ROW_BUDGET = (size_t)1 << 28;      // raw rows of one call (20 bytes of device memory each)

struct RoutesView {
    const uint8_t *og;       // (W,H) x-major occupancy, != 0 is obstacle
    int32_t H;
    const uint32_t *nodes;   // the query's packed vertices
    const int32_t *parent;
    int32_t j;               // tree vertices: [0, j)
    const uint32_t *goals;   // [m] packed
    const int32_t *vertex;   // [m] what the goals kernel decided
    int32_t m;
    int32_t *cnt;            // [m] raw rows of a goal
    int32_t *kept;           // [m] rows after shortcutting
    int64_t *raw_off;        // [m + 1] exclusive scan of cnt
    int64_t *fin_off;        // [m + 1] exclusive scan of kept (== raw_off without shortcuts)
    double *length;          // [m]
    int32_t *err;            // != 0: a parent walk did not end at vertex 0
    uint32_t *row_xy;        // [raw rows] packed points; the shortcut kernel rewrites the front of a goal's rows in place
    int32_t *row_id;         // [raw rows]
    int32_t *out_xy;         // [final rows][2]
    int32_t *out_id;         // [final rows]
};

// ---- rrt_keep.h ----
constexpr int KEEP_TPB = 256;       // edge test: 4 vertices a workgroup (one per wave); pointer jumping and remap: one per lane
constexpr int KEEP_MAX_WG = 2048;   // workgroups of the edge test, grid-stride beyond

struct KeepView {
    const uint8_t *og;       // (W,H) x-major occupancy of the new map, != 0 is obstacle
    int32_t H;
    const uint32_t *nodes;   // the query's packed vertices
    const int32_t *parent;
    const double *vcost;
    int32_t j;               // tree vertices: [0, j)
    uint8_t *ok;             // [j] out of the edge test: edge_ok
    int32_t *anc;            // [j] out of the edge test: the parent, 0 for the root, k itself for a parent outside [0, j)
};

struct KeepCompact {
    const uint32_t *nodes;
    const double *vcost;
    const uint8_t *ok;       // [j] after the last round
    const int32_t *anc;      // [j] after the last round
    int32_t j;
    uint8_t *alive;          // [j] out
    uint32_t *live_nodes;    // [count] out, original order
    double *live_vcost;      // [count]
    int32_t *live_id;        // [count] the original index
    int32_t *count;          // out
};

// ---- rrt_pose_keep.h ----
constexpr int POSE_KEEP_TPB = 64;       // edge test: one wavefront a workgroup, 64 edges a round (one per lane); gather: one vertex per lane
constexpr int POSE_KEEP_MAX_WG = 2048;  // workgroups of the edge test, grid-stride beyond

struct PoseKeepView {
    const uint8_t *og;       // (W,H) x-major occupancy of the new map, != 0 is obstacle
    int32_t W, H;
    const uint32_t *nodes;   // the query's packed vertices
    const int32_t *parent;
    const uint8_t *heading;  // ... and their heading indices
    int32_t j;               // tree vertices: [0, j)
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    uint8_t *ok;             // [j] out of the edge test: edge_ok
    int32_t *anc;            // [j] out of the edge test: the parent, 0 for the root, k itself for a parent outside [0, j)
};

// ---- rrt_pose_routes.h ----
constexpr int POSE_ROUTE_TPB = 256;                         // goals, rows or points per workgroup (one per lane)
constexpr int POSE_ROUTE_MAX_WG = 2048;                     // workgroups of the leg and the points kernel, grid-stride beyond
constexpr size_t POSE_ROUTE_SWEEP_BYTES = 176;              // sizeof(dub_sweep_t) (include/rrt_dubins.h), which no host unit includes
constexpr size_t POSE_ROUTE_ROW_BUDGET = (size_t)1 << 24;   // rows of one call (33 bytes of device memory each, 209 with points: 3.3 GiB)
constexpr size_t POSE_ROUTE_POINT_BUDGET = (size_t)1 << 27; // points of one call (16 bytes of device memory each: 2 GiB)
constexpr int POSE_ROUTE_LEG_POINTS = 1 << 19;              // samples of one leg the kernels accept (rrt_route_scan_kernel sums 1024 counts in 32 bits)

struct PoseRoutesView {
    int32_t W, H;
    const uint32_t *nodes;   // the query's packed vertices
    const int32_t *parent;
    const uint8_t *heading;  // ... and their heading indices
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    const uint32_t *goals;   // [m] cells packed like vertices
    const uint8_t *goal_h;   // [m] heading indices
    const int32_t *vertex;   // [m] what the pose goals kernel decided
    int32_t m;
    const int32_t *cnt;      // [m] rows of a goal (rrt_route_depth_kernel)
    const int64_t *raw_off;  // [m + 1] exclusive scan of cnt
    double *length;          // [m]
    int64_t *goal_pt_off;    // [m + 1] the point offset of a goal's first row; null without points
    int32_t *err;            // bit 0: a parent walk did not end at vertex 0; bit 1: a leg without a word, or one too long
    int64_t rows;            // raw_off[m]
    uint32_t *row_xy;        // [rows] packed cells
    uint8_t *row_h;          // [rows] heading indices
    int32_t *row_id;         // [rows] the vertex, -1 for a goal row
    double *leg_len;         // [rows] length of the word from row r to row r + 1; 0 for a goal row
    int32_t *npts;           // [rows] points of the leg; null without points
    int64_t *pt_off;         // [rows + 1] exclusive scan of npts
    void *sweep_bytes;       // [rows] dub_sweep_t of the legs (POSE_ROUTE_SWEEP_BYTES each); null without points
    int64_t npoints;         // pt_off[rows]
    double2 *points;         // [npoints]
};

// the shortcut pass of rrt_batch_pose_shortcuts: the raw rows of the routes, rewritten in place, and the dense rows they are packed to
constexpr int POSE_CUT_TPB = 256;      // 4 goals a workgroup (one per wavefront); the pack: the same
constexpr int POSE_CUT_MAX_WG = 2048;  // workgroups of the shortcut kernel, grid-stride beyond

struct PoseCutView {
    const uint8_t *og;       // (W,H) x-major occupancy of the active grid, != 0 is obstacle
    int32_t W, H;
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    int32_t m;
    const int32_t *cnt;      // [m] raw rows of a goal (rrt_route_depth_kernel)
    const int64_t *raw_off;  // [m + 1] exclusive scan of cnt
    int32_t *kept;           // [m] rows after shortcutting
    const int64_t *fin_off;  // [m + 1] exclusive scan of kept (the pack reads it)
    uint32_t *row_xy;        // [raw rows] packed cells; the shortcut kernel rewrites the front of a goal's rows in place
    uint8_t *row_h;          // [raw rows] heading indices
    int32_t *row_id;         // [raw rows] the vertex, -1 for a goal row
    uint32_t *out_xy;        // [kept rows] the dense rows: PoseRoutesView's row_xy / row_h / row_id of the kernels that follow
    uint8_t *out_h;
    int32_t *out_id;
};

// ---- rrt_seed.h ----
constexpr int SEED_TPB = 256;                            // one slot / vertex per lane; records: 4 wavefronts a workgroup
constexpr int SEED_WG = 64;                               // workgroups of the records kernel
constexpr int SEED_WAVES = SEED_WG * (SEED_TPB / 64);     // wavefronts that share the cells: 256
constexpr int SEED_OWN = MAX_CELLS / SEED_WAVES;          // cells a wavefront owns: 16 (cell = slot * SEED_WAVES + wavefront)
static_assert(SEED_OWN * SEED_WAVES == MAX_CELLS && SEED_OWN <= 64, "every cell has one owner, one count per lane at the end");

struct SeedView {
    uint32_t *nodes;             // the query's tree arrays
    double *vcost;
    int32_t *parent;
    int32_t j_old, j0, node_stride;  // vertices of the finished tree, of the seed, slots of the node array
    const uint32_t *live_nodes;  // the view (rrt_keep.h), dense; all three null without a view (then j0 == j_old)
    const double *live_vcost;
    const int32_t *live_id;
    int32_t *rank;               // [j_old] scratch, filled with -1
    int32_t *new_parent;         // [j0] scratch
    uint32_t *bitmap;
    int32_t bitmap_words, H;
    int32_t *err;                // set to 1 by any kernel that met something it could not place
};

struct SeedRecords {
    const uint32_t *nodes;
    const double *vcost;
    int32_t j0;
    int32_t cshift, ncx, ncy, ccap;
    int64_t rec_stride;
    u32x4 *cellrec;
    uint32_t *cellcnt;           // [MAX_CELLS]
    int32_t *err;
};

// ---- rrt_reroot.h ----
constexpr int REROOT_TPB = 256;                              // one vertex per lane; edge test: 4 reversed edges a workgroup (one per wave)
constexpr int REROOT_MAX_WG = 2048;                          // workgroups of the edge test, grid-stride beyond
constexpr int REROOT_WG = 64;                                // workgroups of the placement
constexpr int REROOT_WAVES = REROOT_WG * (REROOT_TPB / 64);  // wavefronts that share the keys of the order: 256 (a key belongs to wavefront key % 256)
constexpr int REROOT_SEGS = 64;                              // most segments of the index range a level is spread over (divides REROOT_WAVES)
constexpr int REROOT_OWN = 1024;                             // keys a wavefront owns, their cursors in its LDS: trees of up to 262 144 vertices
static_assert((REROOT_WAVES & (REROOT_WAVES - 1)) == 0 && REROOT_WAVES % REROOT_SEGS == 0 && (REROOT_SEGS & (REROOT_SEGS - 1)) == 0,
              "the owner of a key is taken with a mask, and all keys of an owner lie in one segment");

struct RerootView {
    const uint8_t *og;       // (W,H) x-major occupancy of the context's grid, != 0 is obstacle
    int32_t H;
    const uint32_t *nodes;   // [j] the input tree, dense: the query's tree arrays, or its kept view
    const int32_t *parent;   // [j] ... its parents in the same numbering; vertex 0 is its root, whatever parent[0] holds
    const int32_t *id;       // [j] the number each input vertex has for the caller (the view's live_id); null: its own
    int32_t j, root;         // input vertices [0, j); the new root, one of them
    int32_t *path;           // [j] p_0 = root, p_1 = parent[root], ..., p_d = 0
    int32_t *new_parent;     // [j] the parents after the reversal, input numbering; -1 for the new root
    uint8_t *ok;             // [j] first buffer of the pointer jumping: the edge to new_parent holds (1 for every edge that was not reversed)
    int32_t *anc, *dep;      // [j] ... the ancestor reached and the edges walked to it
    int32_t *level_cnt;      // [j + 1] alive vertices per key (depth, segment); at most j keys (zeroed by the host)
    int32_t *level_start;    // [j + 1] exclusive scan of level_cnt over the keys: level d is [level_start[d * segments], level_start[(d + 1) * segments])
    int32_t *key;            // [j] depth * segments + segment of an alive vertex, -1 for one that is not
    int32_t *rank;           // [j] the new number of an input vertex (filled with -1 by the host: a vertex that is not alive has none)
    int32_t *src;            // [j] the input vertex behind a new number
    uint32_t *out_nodes;     // [j] the re-rooted tree in its new numbering: what rrt_seed_install_kernel takes for a view
    double *out_vcost;
    int32_t *out_parent;
    int32_t *out_id;
    int32_t *head;           // [8] out: d, the alive count, err (!= 0: not a tree, or a vertex that cannot be placed), the new root's packed cell,
                             //          the deepest level (-1 from the host)
};
enum : int { REROOT_D = 0, REROOT_COUNT = 1, REROOT_ERR = 2, REROOT_XY = 3, REROOT_MAXD = 4, REROOT_HEAD = 8 };

// ---- rrt_relax.h ----
constexpr int RELAX_TPB = 256;           // buckets and check: one vertex per lane; rounds and parents: 4 vertices a workgroup (one per wave)
constexpr int RELAX_MAX_WG = 2048;       // workgroups of a round and of the parent pass, grid-stride beyond
constexpr int RELAX_MAX_CELLS = 4096;    // cells of the buckets: the cell edge doubles until they fit
constexpr int RELAX_LIST = 1024;         // qualifying candidates a wavefront lists in LDS at a time (12 bytes each: 48 KiB a workgroup)

struct RelaxView {
    const uint8_t *og;       // (W,H) x-major occupancy of the context's grid, != 0 is obstacle
    int32_t H;
    const uint32_t *nodes;   // [j] the input tree, dense: the query's tree arrays, or its kept view
    const int32_t *parent;   // [j] ... its parents in the same numbering; vertex 0 is its root
    const double *vcost;     // [j] ... and its costs: cost[v] == cost[parent[v]] + d bit for bit
    int32_t j;
    int64_t R;               // an edge u -> v is a candidate when d2(u, v) < R (hostprep.radius_threshold)
    int32_t shift, ncx, ncy; // buckets: cells of edge 2^shift with 2^(2 shift) >= R, ncx * ncy <= RELAX_MAX_CELLS of them
    int32_t *cell_of;        // [j] the cell of a vertex, -1 for one outside the cells
    int32_t *cell_start;     // [ncx * ncy + 1] the CSR
    int32_t *cell_fill;      // [ncx * ncy] counts, then cursors (zeroed by the host)
    int32_t *items;          // [j] the vertices by cell
    uint32_t *item_xy;       // [j] ... and the point of each
    int32_t *pos_of;         // [j] where a vertex stands in items: the rounds flag the vertices whose cost fell in that order
    double *cost;            // [j] relaxed in place
    int32_t *new_parent;     // [j] out of the parent pass, input numbering; -1 for the root
    unsigned long long *stats;  // [4] (zeroed by the host)
    int32_t *err;            // != 0: an index that cannot be placed, or costs that are no fixpoint
    // The buckets alone serve rrt_field.h too, which has no parents and relaxes nothing: parent, pos_of and cost may be null (then the cell
    // kernel checks no parent and the two kernels leave those arrays out), and these two, null for the relax calls, are filled if given.
    double *item_cost;       // [j] vcost of every item of the CSR, beside item_xy
    unsigned long long *cell_min;  // [ncx * ncy] the smallest vcost of a cell's vertices, as the bits of a non-negative f64 (filled with ~0 by the host: an empty cell keeps it)
};
enum : int { RELAX_CHANGES = 0, RELAX_FELL = 1, RELAX_LOS = 2, RELAX_PRICED = 3, RELAX_STATS = 4 };

// ---- rrt_pose_relax.h ----
constexpr int POSE_RELAX_LIST = 256;     // surviving candidates a wavefront lists in LDS at a time (17 bytes each: 17 KiB a workgroup)

// The buckets, the costs, the flags and the counters are rrt_relax.h's (xv; its RELAX_LOS counts sweeps and its RELAX_PRICED words here);
// a pose adds a heading byte to every vertex and every item, and an edge is a Dubins word.
struct PoseRelaxView {
    RelaxView xv;
    int32_t W;               // the grid's other side (xv.H is the stride)
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    const uint8_t *heading;  // [j] the heading index of every input vertex
    uint8_t *item_h;         // [j] ... and of every item of the CSR, beside item_xy
    double *plen;            // [j] the length of the word parent[v] -> v, the old parent edge, evaluated once
};

// ---- rrt_field.h ----
constexpr int FIELD_TPB = 256;           // 4 cells a workgroup at a time (one per wave)
constexpr int FIELD_MAX_WG = 8192;       // workgroups of the decision, grid-stride beyond
constexpr int FIELD_RUN = 16;            // consecutive cells of one column that a wavefront decides one after the other, each starting from the winner before it
constexpr int FIELD_MIN_SHIFT = 3;       // buckets of edge 2^shift, shift at least this, doubled until they fit RELAX_MAX_CELLS
constexpr int FIELD_BUCKETS = 128;       // qualifying buckets a wavefront lists in LDS at a time (12 bytes each)
constexpr int FIELD_LIST = 256;          // candidates a wavefront lists in LDS (16 bytes each) before it walks them, one line per lane; both lists: 22 KiB a workgroup

// The cost-to-come field of a window of the grid: for every cell the smallest (vcost[k] + sqrt(d2(k, cell)), k) over the vertices that see it.
// xv holds the buckets (rrt_relax.h's CSR with item_cost and cell_min) over the dense input: the tree arrays, or the kept view.
struct FieldView {
    RelaxView xv;
    int32_t W;               // the grid's other side (xv.H is the stride)
    int32_t x0, y0, w, h;    // the window, inside the grid
    int32_t *vertex;         // [w * h] out, cell (x, y) at (x - x0) * h + (y - y0): the vertex in the numbers of the input, or -1
    double *cost;            // [w * h] out: the cost through it, or +inf
};
enum : int { FIELD_CELLS = 0, FIELD_BUCKETS_SEEN = 1, FIELD_PRICED = 2, FIELD_LOS = 3, FIELD_STATS = 4 };

// ---- rrt_pose_field.h ----
constexpr int POSE_FIELD_TPB = 256;      // 4 cells a workgroup at a time (one per wave)
constexpr int POSE_FIELD_MAX_WG = 8192;  // workgroups of the decision, grid-stride beyond
constexpr int POSE_FIELD_RUN = 16;       // most consecutive cells of one column that a wavefront decides one after the other, each starting from the winner before it
constexpr int POSE_FIELD_WAVES = 4096;   // wavefronts a window should give work to before its runs grow: 16 on each of 256 CUs
constexpr int POSE_FIELD_BUCKETS = 128;  // qualifying buckets a wavefront lists in LDS at a time (8 bytes each)
constexpr int POSE_FIELD_LIST = 256;     // surviving vertices a wavefront lists in LDS (17 bytes each) before it expands them to pairs; with the
                                         // heading table 27 KiB a workgroup: five of them fit the 160 KiB of a CU
constexpr int POSE_FIELD_MAX_J = 1 << 18;  // vertices of the dense input: a pair's key is heading << 18 | vertex in 32 bits

// The pose cost field of a window of the grid: for every cell the smallest (vcost[k] + word(pose_k -> (cell, a)).len, a, k) over the pairs
// (heading a in [heading_lo, heading_hi), vertex k) whose sweep is free.  xv holds the buckets (rrt_relax.h's CSR with item_cost and
// cell_min) over the dense input: the tree arrays, or the kept view.
struct PoseFieldView {
    RelaxView xv;
    int32_t W;               // the grid's other side (xv.H is the stride)
    int32_t nh;              // the query's discrete headings
    double rho;              // ... and turning radius
    const uint8_t *heading;  // [j] the heading index of every input vertex
    uint8_t *item_h;         // [j] ... and of every item of the CSR, beside item_xy
    int32_t x0, y0, w, h;    // the window, inside the grid
    int32_t heading_lo, heading_hi;  // the arrival headings asked: one, [H, H + 1), or all, [0, nh)
    int32_t run;             // consecutive cells of a column that one wavefront decides: 1 to POSE_FIELD_RUN
    int32_t *vertex;         // [w * h] out, cell (x, y) at (x - x0) * h + (y - y0): the vertex in the numbers of the input, or -1
    double *cost;            // [w * h] out: the cost through it, or +inf
    int32_t *heading_out;    // [w * h] out: the arrival heading of the answer, or -1
};
enum : int { POSE_FIELD_CELLS = 0, POSE_FIELD_BUCKETS_SEEN = 1, POSE_FIELD_WORDS = 2, POSE_FIELD_SWEEPS = 3, POSE_FIELD_STATS = 4 };

// ---- rrt_pose_reroot.h ----
// The dense input of a pose re-root (the tree arrays or the kept view, as RerootView takes them, with the heading bytes) and where it
// goes with `root` moved to the front as number 0 and the others in their order: what the relax kernels then take as their input.
struct PoseRerootView {
    const uint32_t *nodes;   // [j] the input, dense
    const int32_t *parent;   // [j] ... its parents in the same numbering; vertex 0 is its root, whatever parent[0] holds
    const uint8_t *heading;  // [j] ... its heading indices
    const int32_t *id;       // [j] the number each input vertex has for the caller; null: its own
    int32_t j, root;         // input vertices [0, j); the new root, one of them
    uint32_t *f_nodes;       // [j] root first
    int32_t *f_parent;       // [j] ... the old parents in the new numbers; -1 for the new root and for the old one
    uint8_t *f_heading;      // [j]
    int32_t *f_id;           // [j] ... the caller's number of each
};

// ---- the kernels a host unit launches, by the file that defines them ----
// rrt_serial.h (units 2 and 3 instantiate it)
template <bool RW, bool DUB = false>
__global__ __launch_bounds__(TPB) void rrt_expand_kernel(BatchView bv);
// rrt_pipe.h (unit 1; unit 4: grids up to 4096 x 4096), rrt_dubins_block.h (unit 2)
__global__ __launch_bounds__(TPB) void rrt_pipe_kernel(BatchView bv);
__global__ __launch_bounds__(TPB) void rrt_pipe_large_kernel(BatchView bv);
__global__ __launch_bounds__(TPB) void rrt_dubins_block_kernel(BatchView bv);
// rrt_block.h (units 10 and up instantiate the rows of rrt_block_variants.def)
template <int G, int BSM, bool PIPE, bool INF>
__global__ __launch_bounds__(TPB) void rrt_expand_block_kernel(BatchView bv);
template <int G, int BSM, bool INF>
__global__ __launch_bounds__(512) void rrt_block_commit_kernel(BatchView bv);
template <int G, int BSM, bool INF>
__global__ __launch_bounds__(TPB) void rrt_block_work_kernel(BatchView bv);
// rrt_goals.h (unit 5), rrt_pose_goals.h (unit 9)
__global__ __launch_bounds__(TPB) void rrt_goals_kernel(GoalsView gv);
__global__ __launch_bounds__(TPB) void rrt_goals_large_kernel(GoalsView gv);
__global__ __launch_bounds__(TPB) void rrt_pose_goals_kernel(PoseGoalsView pv);
// rrt_field.h (unit 5, beside the goals kernels; its buckets are rrt_relax.h's kernels of unit 0)
__global__ __launch_bounds__(FIELD_TPB) void rrt_field_kernel(FieldView fv);
__global__ __launch_bounds__(FIELD_TPB) void rrt_field_large_kernel(FieldView fv);
// rrt_routes.h (unit 6)
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_depth_kernel(RoutesView rv);
__global__ __launch_bounds__(TPB) void rrt_route_scan_kernel(const int32_t *in, int64_t *out, int32_t m);
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_fill_kernel(RoutesView rv, int32_t with_len);
__global__ __launch_bounds__(TPB) void rrt_route_cut_kernel(RoutesView rv);
__global__ __launch_bounds__(TPB) void rrt_route_cut_large_kernel(RoutesView rv);
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_pack_kernel(RoutesView rv);
// rrt_keep.h (unit 7)
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_edge_kernel(KeepView kv);
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_edge_large_kernel(KeepView kv);
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_jump_kernel(const uint8_t *ok, const int32_t *anc, uint8_t *ok2, int32_t *anc2, int32_t j);
__global__ __launch_bounds__(TPB) void rrt_keep_compact_kernel(KeepCompact kc);
__global__ __launch_bounds__(KEEP_TPB) void rrt_keep_remap_kernel(int32_t *vertex, const int32_t *live_id, int32_t m, int32_t count);
// rrt_pose_keep.h (unit 9, beside the pose goals)
__global__ __launch_bounds__(POSE_KEEP_TPB) void rrt_pose_keep_edge_kernel(PoseKeepView kv);
__global__ __launch_bounds__(POSE_KEEP_TPB) void rrt_pose_keep_gather_kernel(const uint8_t *heading, const int32_t *live_id, const int32_t *count,
                                                                            uint8_t *live_heading, int32_t j);
// rrt_pose_routes.h (unit 9, beside the other pose kernels)
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_fill_kernel(PoseRoutesView pr);
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_leg_kernel(PoseRoutesView pr);
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_length_kernel(PoseRoutesView pr);
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_points_kernel(PoseRoutesView pr);
__global__ __launch_bounds__(POSE_CUT_TPB) void rrt_pose_route_cut_kernel(PoseCutView pc);
__global__ __launch_bounds__(POSE_CUT_TPB) void rrt_pose_route_pack_kernel(PoseCutView pc);
// rrt_seed.h (unit 8)
__global__ __launch_bounds__(SEED_TPB) void rrt_seed_rank_kernel(SeedView sv);
__global__ __launch_bounds__(SEED_TPB) void rrt_seed_parent_kernel(SeedView sv);
__global__ __launch_bounds__(SEED_TPB) void rrt_seed_install_kernel(SeedView sv);
__global__ __launch_bounds__(SEED_TPB) void rrt_seed_bitmap_kernel(SeedView sv);
__global__ __launch_bounds__(SEED_TPB) void rrt_seed_records_kernel(SeedRecords sr);
// rrt_pose_seed.h (unit 8, beside the seed kernels)
__global__ __launch_bounds__(SEED_TPB) void rrt_pose_seed_heading_kernel(uint8_t *heading, const uint8_t *live_heading, int32_t j0, int32_t node_stride);

// rrt_reroot.h (unit 0; the numbers from 10 on belong to the team kernels)
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_path_kernel(RerootView rv);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_edge_kernel(RerootView rv);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_link_kernel(RerootView rv);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_jump_kernel(const uint8_t *ok, const int32_t *anc, const int32_t *dep, uint8_t *ok2, int32_t *anc2,
                                                                     int32_t *dep2, int32_t j);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_count_kernel(RerootView rv, const uint8_t *ok, const int32_t *anc, const int32_t *dep);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_level_kernel(RerootView rv);
__global__ __launch_bounds__(TPB) void rrt_reroot_scan_kernel(RerootView rv);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_place_kernel(RerootView rv);
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_parent_kernel(RerootView rv);
__global__ __launch_bounds__(TPB) void rrt_reroot_cost_kernel(RerootView rv);
// rrt_relax.h (unit 0, beside the re-root kernels whose later stages it runs)
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_cell_kernel(RelaxView xv);
__global__ __launch_bounds__(TPB) void rrt_relax_scan_kernel(RelaxView xv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_fill_kernel(RelaxView xv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_round_kernel(RelaxView xv, const double *cin, double *cout, const uint8_t *dirty_in, uint8_t *dirty_out,
                                                                    const uint8_t *changed_in, uint8_t *changed_out, int32_t first);
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_parent_kernel(RelaxView xv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_check_kernel(RelaxView xv, const int32_t *src, const double *out_vcost, const int32_t *count);
// rrt_pose_relax.h (unit 0, beside the relax kernels whose buckets and check it runs)
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_item_kernel(PoseRelaxView pv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_round_kernel(PoseRelaxView pv, const uint8_t *dirty_in, uint8_t *dirty_out, const uint8_t *changed_in,
                                                                         uint8_t *changed_out, int32_t first);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_parent_kernel(PoseRelaxView pv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_word_kernel(PoseRelaxView pv, RerootView rv, uint8_t *out_heading, double *word);
__global__ __launch_bounds__(TPB) void rrt_pose_relax_cost_kernel(RerootView rv, const double *word);
// rrt_pose_reroot.h (unit 0, beside the pose relax kernels whose round and parent pass it runs from another root)
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_front_kernel(PoseRerootView fv, RelaxView xv);
__global__ __launch_bounds__(TPB) void rrt_pose_reroot_start_kernel(RerootView rv, const double *plen, double *cost);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_round_kernel(PoseRelaxView pv, const uint8_t *dirty_in, uint8_t *dirty_out, const uint8_t *changed_in,
                                                                          uint8_t *changed_out, int32_t first);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_parent_kernel(PoseRelaxView pv);
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_reroot_check_kernel(RelaxView xv, const int32_t *src, const double *out_vcost, const int32_t *count);
// rrt_pose_field.h (unit -1: the numbers 0 to 9 are taken and those from 10 on are the team kernels'; its buckets are rrt_relax.h's kernels of unit 0)
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_field_item_kernel(PoseFieldView pv);
__global__ __launch_bounds__(POSE_FIELD_TPB) void rrt_pose_field_kernel(PoseFieldView pv);

}  // namespace rrtdev
