// rrt_scratch.h -- what every multi-array scratch buffer of the tree calls (rrt_tree_calls.hip) holds, said once.  A layout struct
// declares the arrays of a buffer in their order, each with its type and its length; constructing it over a base pointer and a capacity
// carves them, and the same pass counts the bytes to allocate (DevBuf::reserve<Layout> / DevBuf::carve<Layout>, rrt_engine.h).
// Host code in plain C++17, nothing of HIP: tests/scratch_layouts/ compiles it alone, under the sanitizers.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>

// Hands out the arrays of a buffer of capacity `cap` (goals, rows or vertices) one behind the other.  Over a null base the pointers
// are null and only the bytes are counted.  A layout derives from it: its members are initialised in the order they are declared.
struct Carver {
    unsigned char *base;
    size_t cap;
    size_t bytes = 0;  // the running offset; behind the last array, the size of the buffer
    Carver(void *base_, size_t cap_) : base(static_cast<unsigned char *>(base_)), cap(cap_) {}
    template <typename T>
    T *take(size_t count) {
        assert(bytes % alignof(T) == 0 && "an array of a scratch layout starts off its alignment: reorder the layout");
        T *p = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += count * sizeof(T);
        return p;
    }
};

// rrt_batch_routes, per goal (rrt_routes.h)
struct RouteGoalScratch : Carver {
    using Carver::Carver;
    double *length = take<double>(cap);
    int64_t *raw_off = take<int64_t>(cap + 1);
    int64_t *fin_off = take<int64_t>(cap + 1);
    int32_t *cnt = take<int32_t>(cap);
    int32_t *kept = take<int32_t>(cap);
    int32_t *err = take<int32_t>(1);
};

// ... and per raw row (shortcuts only ever drop rows, so the final rows fit the same capacity)
struct RouteRowScratch : Carver {
    using Carver::Carver;
    uint32_t *row_xy = take<uint32_t>(cap);
    int32_t *row_id = take<int32_t>(cap);
    int32_t *out_xy = take<int32_t>(2 * cap);  // [cap][2]
    int32_t *out_id = take<int32_t>(cap);
};

// rrt_batch_pose_routes / rrt_batch_pose_shortcuts, per goal pose (rrt_pose_routes.h)
struct PoseRouteGoalScratch : Carver {
    using Carver::Carver;
    double *length = take<double>(cap);
    int64_t *raw_off = take<int64_t>(cap + 1);
    int64_t *goal_pt_off = take<int64_t>(cap + 1);
    int32_t *cnt = take<int32_t>(cap);
    int32_t *err = take<int32_t>(1);
};

// ... and per dense row; cap >= 1, so that a call without a row still has pt_off[0]
struct PoseRouteRowScratch : Carver {
    using Carver::Carver;
    double *leg_len = take<double>(cap);
    int64_t *pt_off = take<int64_t>(cap + 1);
    uint32_t *row_xy = take<uint32_t>(cap);
    int32_t *row_id = take<int32_t>(cap);
    int32_t *npts = take<int32_t>(cap);
    uint8_t *row_h = take<uint8_t>(cap);
};

// rrt_batch_pose_shortcuts alone, per goal pose: what the shortcut pass keeps
struct PoseCutGoalScratch : Carver {
    using Carver::Carver;
    int64_t *fin_off = take<int64_t>(cap + 1);
    int32_t *kept = take<int32_t>(cap);
};

// ... and per raw row: the rows of the walks, which the pass rewrites in place
struct PoseCutRowScratch : Carver {
    using Carver::Carver;
    uint32_t *row_xy = take<uint32_t>(cap);
    int32_t *row_id = take<int32_t>(cap);
    uint8_t *row_h = take<uint8_t>(cap);
};

// The kept view of one query (rrt_keep.h, rrt_pose_keep.h): its alive vertices, dense and in the original order; cap = n_cap.
struct KeepScratch : Carver {
    KeepScratch(void *base_, size_t cap_, bool headings_) : Carver(base_, cap_), headings(headings_) {}
    bool headings;  // a Dubins batch
    double *live_vcost = take<double>(cap);
    uint32_t *live_nodes = take<uint32_t>(cap);
    int32_t *live_id = take<int32_t>(cap);  // the original number of each
    uint8_t *live_heading = headings ? take<uint8_t>(cap) : nullptr;
};

// What a keep call works in: ancestor and flag of every vertex, twice (the pointer jumping goes from one to the other and back), and
// the count of the compaction, for which 8 bytes are reserved.  cap = n_cap; the arrays have it rounded up to 8 elements.
struct KeepTmpScratch : Carver {
    using Carver::Carver;
    size_t cap8 = (cap + 7) & ~(size_t)7;
    int32_t *anc[2] = {take<int32_t>(cap8), take<int32_t>(cap8)};
    uint8_t *ok[2] = {take<uint8_t>(cap8), take<uint8_t>(cap8)};
    int32_t *count = take<int32_t>(2);
};

// What a grow call works in (rrt_seed.h); cap = n_cap.  Two words are reserved for err.
struct SeedTmpScratch : Carver {
    using Carver::Carver;
    int32_t *rank = take<int32_t>(cap);
    int32_t *new_parent = take<int32_t>(cap);
    int32_t *err = take<int32_t>(2);
};

// What a reroot call works in (rrt_reroot.h); cap = n_cap.  The pointer jumping goes between two sets of (anc, dep, ok) and back; the
// flag arrays have cap rounded up to 8 elements and come last.  key takes the set of the jumping that the last round did not write.
// head: d, the alive count, err, the new root's cell, the deepest level; eight words are reserved.
struct RerootScratch : Carver {
    using Carver::Carver;
    size_t cap8 = (cap + 7) & ~(size_t)7;
    double *out_vcost = take<double>(cap);
    uint32_t *out_nodes = take<uint32_t>(cap);
    int32_t *out_parent = take<int32_t>(cap);
    int32_t *out_id = take<int32_t>(cap);
    int32_t *path = take<int32_t>(cap);
    int32_t *new_parent = take<int32_t>(cap);
    int32_t *anc[2] = {take<int32_t>(cap), take<int32_t>(cap)};
    int32_t *dep[2] = {take<int32_t>(cap), take<int32_t>(cap)};
    int32_t *level_cnt = take<int32_t>(cap + 1);
    int32_t *level_start = take<int32_t>(cap + 1);
    int32_t *rank = take<int32_t>(cap);
    int32_t *src = take<int32_t>(cap);
    int32_t *head = take<int32_t>(8);
    uint8_t *ok[2] = {take<uint8_t>(cap8), take<uint8_t>(cap8)};
};

// What a relax call works in beside a RerootScratch (rrt_relax.h); cap = n_cap, cells = the most cells of the buckets.  The costs are
// relaxed in `cost`; the rounds mark the cells that changed in one of the two `dirty` arrays and the vertices whose cost fell, in the
// order of `items`, in one of the two `changed` arrays, and read the other of each.
struct RelaxScratch : Carver {
    RelaxScratch(void *base_, size_t cap_, size_t cells_) : Carver(base_, cap_), cells(cells_) {}
    size_t cells;
    size_t cells8 = (cells + 7) & ~(size_t)7;
    size_t cap8 = (cap + 7) & ~(size_t)7;
    double *cost = take<double>(cap);
    unsigned long long *stats = take<unsigned long long>(4);
    int32_t *cell_of = take<int32_t>(cap);
    int32_t *items = take<int32_t>(cap);
    uint32_t *item_xy = take<uint32_t>(cap);
    int32_t *pos_of = take<int32_t>(cap);
    int32_t *cell_start = take<int32_t>(cells + 1);
    int32_t *cell_fill = take<int32_t>(cells);
    uint8_t *dirty[2] = {take<uint8_t>(cells8), take<uint8_t>(cells8)};
    uint8_t *changed[2] = {take<uint8_t>(cap8), take<uint8_t>(cap8)};
};

// What a relax_poses call works in beside a RerootScratch and a RelaxScratch (rrt_pose_relax.h); cap = n_cap.  plen: the length of every
// old parent edge; word: of the edge to every new number's parent, for the cost stage; item_h: the heading byte of every item of the
// CSR; out_heading: the headings in the new order, which the seed installs.  The byte arrays have cap rounded up to 8 and come last.
struct PoseRelaxScratch : Carver {
    using Carver::Carver;
    size_t cap8 = (cap + 7) & ~(size_t)7;
    double *plen = take<double>(cap);
    double *word = take<double>(cap);
    uint8_t *item_h = take<uint8_t>(cap8);
    uint8_t *out_heading = take<uint8_t>(cap8);
};

// What a reroot_poses call works in beside the three of relax_poses (rrt_pose_reroot.h); cap = n_cap.  The dense input with the new root
// moved to the front: points, old parents in the new numbers, the caller's number of each, heading bytes (cap rounded up to 8, last).
struct PoseRerootScratch : Carver {
    using Carver::Carver;
    size_t cap8 = (cap + 7) & ~(size_t)7;
    uint32_t *f_nodes = take<uint32_t>(cap);
    int32_t *f_parent = take<int32_t>(cap);
    int32_t *f_id = take<int32_t>(cap);
    uint8_t *f_heading = take<uint8_t>(cap8);
};

// What a cost_field call works in (rrt_field.h); cap = n_cap, cells = the most cells of the buckets.  The CSR of rrt_relax.h without what
// only a relaxation needs, with the cost of every item and the smallest cost of every bucket.  stats: the four counters of the call;
// two words are reserved for err.
struct FieldScratch : Carver {
    FieldScratch(void *base_, size_t cap_, size_t cells_) : Carver(base_, cap_), cells(cells_) {}
    size_t cells;
    double *item_cost = take<double>(cap);
    unsigned long long *cell_min = take<unsigned long long>(cells);
    unsigned long long *stats = take<unsigned long long>(4);
    int32_t *cell_of = take<int32_t>(cap);
    int32_t *items = take<int32_t>(cap);
    uint32_t *item_xy = take<uint32_t>(cap);
    int32_t *cell_start = take<int32_t>(cells + 1);
    int32_t *cell_fill = take<int32_t>(cells);
    int32_t *err = take<int32_t>(2);
};
