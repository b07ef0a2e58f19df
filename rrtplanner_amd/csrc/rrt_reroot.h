// rrt_reroot.h -- re-root a finished straight-line tree at one of its vertices: the arrays that rrt_seed.h then installs as a seed.
//
// The tree is an undirected set of tested edges.  With r the new root and p_0 = r, p_1 = parent[r], ..., p_d = 0 its way to the old
// root, the new parents are  new_parent[p_{i+1}] = p_i,  new_parent[r] = -1,  every other vertex keeps its own.  The line walk is not
// symmetric (rrt_keep.h, "The direction of the walk"), and a valid edge is collisionfree(og, points[parent], points[child]): each of
// the d reversed edges is walked again from its new parent to its new child on the context's grid.  The other edges stand tested on
// this grid.  A vertex is alive iff every edge on its new way to r holds; a blocked reversed edge cuts what hangs behind it.
// The alive vertices are numbered by (depth below r, previous number): r is vertex 0 and every parent is below its child, which
// the seed, the route walks and go2goal rely on.  cost[0] = 0 and cost[k] = cost[new_parent[k]] + sqrt((double)d2), accumulated from
// the root down -- the arithmetic of the expansion loop, never old - cost[r].
//
// The input is dense: the tree arrays [0, j), or the kept view with its parents renumbered (rrt_seed_rank_kernel,
// rrt_seed_parent_kernel).  Nothing is permuted in place: every kernel writes scratch, and rrt_seed_install_kernel moves the result.
//
//   1. rrt_reroot_path_kernel     every lane: new_parent[k] = parent[k], ok[k] = 1.  One lane walks r -> 0, at most j - 1 steps, and
//                                 lists p_0 .. p_d.  A walk that is not at vertex 0 by then raises err (and d = 0).
//   2. rrt_reroot_edge_kernel     one wavefront per reversed edge i < d, grid-stride: ok[p_{i+1}] = los_wave(p_i -> p_{i+1}),
//                                 new_parent[p_{i+1}] = p_i; new_parent[r] = -1.
//      rrt_reroot_link_kernel     anc[k] = new_parent[k] (r: itself), dep[k] = 1 (r: 0): the start of the pointer jumping.
//   3. rrt_reroot_jump_kernel     one round of pointer jumping with the depth (jump_round, rrt_tree_dev.h): dep[k] is the number of
//                                 edges between k and anc[k] all along.  ceil(log2(max(j, 2))) rounds, queued by the host.  Afterwards
//                                 alive[k] = ok[k] and anc[k] == r, and dep[k] is the depth of an alive vertex.
//   4. The order is a stable counting sort on the key (depth, segment of the index range): the segments, up to 64 of them, only spread
//      the vertices of one level over several wavefronts; the key ascends with the index inside a level, so the order is still
//      (depth, previous number).
//      rrt_reroot_count_kernel    key[k] = dep[k] for an alive vertex, -1 otherwise, and the deepest level by atomicMax.
//      rrt_reroot_level_kernel    key[k] = depth * segments + k / segment length; level_cnt[key] += 1, one atomic per wavefront and
//                                 key (integer atomics: a sum, no order).
//      rrt_reroot_scan_kernel     one workgroup: level_start = exclusive scan of level_cnt over the keys, the alive count.
//      rrt_reroot_place_kernel    every wavefront OWNS the keys with key % REROOT_WAVES == its number, which all lie in one segment, and
//                                 walks that segment in index order, 256 keys a step; the owned ones go behind the key's cursor, which
//                                 starts at level_start (wave_place_by_key, rrt_tree_dev.h).  It writes rank[k] and src[pos] and loads
//                                 nothing but the keys.
//      rrt_reroot_parent_kernel   one new number per lane, behind the placement of every vertex: the point and the previous number of
//                                 src[pos], and out_parent[pos] = rank[new_parent[src[pos]]].
//   5. rrt_reroot_cost_kernel     one workgroup: a level is a contiguous range whose parents are in the level before; level after
//                                 level with one barrier each.  A chain of j vertices costs j barriers.
// Every index is checked before it is used; what cannot be placed raises err and is not stored.
// (The view, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_tree_dev.h"

namespace rrtdev {

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_path_kernel(RerootView rv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int j = rv.j;
    if (k < j) {
        const int p = k == 0 ? -1 : rv.parent[k];
        if (k > 0 && (p < 0 || p >= j)) atomicOr(&rv.head[REROOT_ERR], 1);
        rv.new_parent[k] = (p >= 0 && p < j) ? p : -1;
        rv.ok[k] = (uint8_t)1;
    }
    if (k != 0) return;
    int u = rv.root, steps = 0;
    if (u < 0 || u >= j) {
        atomicOr(&rv.head[REROOT_ERR], 1);
        rv.head[REROOT_D] = 0;
        rv.head[REROOT_XY] = 0;
        return;
    }
    rv.head[REROOT_XY] = (int32_t)rv.nodes[u];
    rv.path[0] = u;
    while (u > 0 && u < j && steps < j - 1) {
        u = rv.parent[u];
        ++steps;
        if (u >= 0 && u < j) rv.path[steps] = u;  // (steps <= j - 1)
    }
    if (u != 0) atomicOr(&rv.head[REROOT_ERR], 1);
    rv.head[REROOT_D] = u == 0 ? steps : 0;
}

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_edge_kernel(RerootView rv) {
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = rv.j, d = rv.head[REROOT_D];
    if (blockIdx.x == 0 && threadIdx.x == 0 && rv.root >= 0 && rv.root < j) rv.new_parent[rv.root] = -1;
    if (d < 0 || d >= j) return;
    for (int i = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); i < d; i += (int)gridDim.x * waves) {  // (i is wave-uniform)
        const int p = rv.path[i], c = rv.path[i + 1];  // the new parent and its new child
        if (p < 0 || p >= j || c < 0 || c >= j) continue;  // (the walk wrote neither)
        int cells;
        const bool ok = los_wave(rv.og, rv.H, rv.nodes[p], rv.nodes[c], lane, cells);
        if (lane == 0) {
            rv.ok[c] = ok ? (uint8_t)1 : (uint8_t)0;
            rv.new_parent[c] = p;
        }
    }
}

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_link_kernel(RerootView rv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= rv.j) return;
    const int p = rv.new_parent[k];
    const bool top = k == rv.root || p < 0 || p >= rv.j;
    if (top && k != rv.root) rv.ok[k] = (uint8_t)0;  // (a vertex without a parent that is not the root hangs on nothing)
    rv.anc[k] = top ? k : p;
    rv.dep[k] = top ? 0 : 1;
}

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_jump_kernel(const uint8_t *ok, const int32_t *anc, const int32_t *dep, uint8_t *ok2, int32_t *anc2,
                                                                     int32_t *dep2, int32_t j) {
    jump_round<true>(ok, anc, dep, ok2, anc2, dep2, j);
}

// How many segments the index range [0, j) is cut into for the order: the largest power of two up to REROOT_SEGS for which the keys
// (depth, segment) of all levels, (maxd + 1) * segments of them, still fit the arrays of j entries.  A chain gets 1, a bushy tree 64.
__device__ __forceinline__ int reroot_segments(int j, int maxd) {
    int segs = REROOT_SEGS;
    while (segs > 1 && (long long)(maxd + 1) * segs > (long long)j) segs >>= 1;
    return segs;
}
__device__ __forceinline__ int reroot_seglen(int j, int segs) { return (j + segs - 1) / segs; }  // vertices of a segment (the last may be shorter)

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_count_kernel(RerootView rv, const uint8_t *ok, const int32_t *anc, const int32_t *dep) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool in = k < rv.j;  // (no lane leaves early: the wavefront's maximum below is taken over all of them)
    const bool live = in && ok[k] != 0 && anc[k] == rv.root;
    int d = live ? dep[k] : -1;
    if (live && (d < 0 || d >= rv.j)) {
        atomicOr(&rv.head[REROOT_ERR], 1);
        d = -1;
    }
    if (in) rv.key[k] = d;
    const int deepest = wave_incl_max_i32(d);  // the deepest level: one atomic per wavefront
    if (((int)threadIdx.x & 63) == 63 && deepest >= 0) atomicMax(&rv.head[REROOT_MAXD], deepest);
}

// key[k] = depth * segments + segment of k, and the count of every key: one atomic per wavefront and key (a sum: no order hangs on it)
__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_level_kernel(RerootView rv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x), lane = (int)threadIdx.x & 63;
    const int j = rv.j, maxd = rv.head[REROOT_MAXD];
    if (maxd < 0 || maxd >= j) return;  // (uniform: nothing is alive, or the count kernel raised err)
    const int segs = reroot_segments(j, maxd), seglen = reroot_seglen(j, segs);
    const int d = k < j ? rv.key[k] : -1;
    const bool live = d >= 0 && d <= maxd;
    const int key = live ? d * segs + k / seglen : -1;  // (below (maxd + 1) * segs <= j)
    if (k < j) rv.key[k] = key;
    wave_each_key(live, key, [&](int kl, unsigned long long same, bool) {  // the first lane of a key adds its count
        if (lane == (int)__builtin_ctzll(same)) atomicAdd(&rv.level_cnt[kl], (int32_t)__builtin_popcountll(same));
    });
}

// exclusive scan of level_cnt[0, L) into level_start[0, L], L = the number of keys, (maxd + 1) * segments <= j: one workgroup of TPB
// threads, TPB values a pass.  Nothing reads level_start behind L.
__global__ __launch_bounds__(TPB) void rrt_reroot_scan_kernel(RerootView rv) {
    const int t = (int)threadIdx.x;
    const int maxd = rv.head[REROOT_MAXD];
    const int L = maxd < 0 || maxd >= rv.j ? 0 : (maxd + 1) * reroot_segments(rv.j, maxd);  // (uniform)
    uint32_t carry = 0;
    int par = 0;
    for (int base = 0; base < L; base += TPB) {
        const int k = base + t;
        const uint32_t v = k < L ? (uint32_t)rv.level_cnt[k] : 0u;
        const uint32_t incl = wave_incl_sum_u32(v);
        const WgScan s = wg_scan_step(incl, par);
        if (k < L) rv.level_start[k] = (int32_t)(carry + s.before + incl - v);
        carry += s.total;
    }
    if (t == 0) {
        rv.level_start[L] = (int32_t)carry;
        rv.head[REROOT_COUNT] = (int32_t)carry;
    }
}

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_place_kernel(RerootView rv) {
    __shared__ int32_t cur_lds[REROOT_TPB / 64][REROOT_OWN];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int gw = (int)blockIdx.x * (REROOT_TPB / 64) + wave;  // this wavefront's number: it owns the keys with key % REROOT_WAVES == gw
    if (gw >= REROOT_WAVES) return;                              // (a launch with more workgroups than REROOT_WG: nothing left to own)
    const int j = rv.j, maxd = rv.head[REROOT_MAXD];
    if (maxd < 0 || maxd >= j) return;  // (uniform)
    if (j > REROOT_WAVES * REROOT_OWN) {  // (uniform; the host refuses such a capacity before it launches)
        atomicOr(&rv.head[REROOT_ERR], 1);
        return;
    }
    const int segs = reroot_segments(j, maxd), seglen = reroot_seglen(j, segs), keys = (maxd + 1) * segs;
    if (gw >= keys) return;  // (wave-uniform: this wavefront owns no key that exists)
    // every key this wavefront owns has the segment gw % segs (segs divides REROOT_WAVES): it walks that segment alone
    const int seg = gw & (segs - 1);
    const int lo = seg * seglen, hi = min(j, lo + seglen);
    volatile RRT_LDS int32_t *cur = (volatile RRT_LDS int32_t *)&cur_lds[wave][0];  // of this wavefront alone
    for (int slot = lane; slot < REROOT_OWN; slot += 64) {
        const int key = slot * REROOT_WAVES + gw;
        cur[slot] = key < keys ? rv.level_start[key] : j;  // (j: a position nothing is stored at)
    }
    for (int base = lo; base < hi; base += 256) {  // (wave-uniform trip count; the four loads of a step are in flight together)
        int key4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = base + 64 * u + lane;
            key4[u] = k < hi ? rv.key[k] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = base + 64 * u + lane;
            const int key = key4[u];
            const bool mine = key >= 0 && key < keys && (key & (REROOT_WAVES - 1)) == gw;
            wave_place_by_key<REROOT_WAVES>(mine, key, cur, [&](int, int32_t pos) {
                if (pos >= 0 && pos < j) {
                    rv.rank[k] = pos;  // (stores only: nothing in this loop waits for global memory but the keys of a step)
                    rv.src[pos] = k;
                } else {
                    atomicOr(&rv.head[REROOT_ERR], 1);
                }
            });
        }
    }
}

__global__ __launch_bounds__(REROOT_TPB) void rrt_reroot_parent_kernel(RerootView rv) {
    const int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int count = rv.head[REROOT_COUNT];
    if (pos >= count || pos >= rv.j) return;
    int np = -1;
    const int k = rv.src[pos];
    if (k < 0 || k >= rv.j || (pos == 0) != (k == rv.root)) {
        atomicOr(&rv.head[REROOT_ERR], 1);
        rv.out_nodes[pos] = 0u;
        rv.out_id[pos] = -1;
        rv.out_parent[pos] = -1;
        return;
    }
    rv.out_nodes[pos] = rv.nodes[k];
    rv.out_id[pos] = rv.id ? rv.id[k] : k;
    if (pos > 0) {
        const int p = rv.new_parent[k];
        np = (p >= 0 && p < rv.j) ? rv.rank[p] : -1;
        if (np < 0 || np >= pos) {  // every ancestor of an alive vertex is alive and a level above it
            atomicOr(&rv.head[REROOT_ERR], 1);
            np = 0;
        }
    }
    rv.out_parent[pos] = np;
}

// The costs of the new numbers from the root down, by ONE workgroup of TPB threads: edge(p, pos) is the length of the edge from new
// number p to its child pos (rrt_reroot_cost_kernel: the straight line; rrt_pose_relax_cost_kernel, rrt_pose_relax.h: a Dubins word
// evaluated beforehand).
template <typename Edge>
__device__ __forceinline__ void reroot_cost_levels(const RerootView &rv, Edge edge) {
    const int t = (int)threadIdx.x;
    const int j = rv.j, count = rv.head[REROOT_COUNT];
    if (count < 1 || count > j || rv.head[REROOT_ERR] != 0) return;  // (uniform)
    if (t == 0) rv.out_vcost[0] = 0.0;
    const int maxd = rv.head[REROOT_MAXD];
    if (maxd < 0 || maxd >= j) return;  // (uniform)
    const int segs = reroot_segments(j, maxd);
    for (int level = 1; level <= maxd; ++level) {
        __syncthreads();  // the costs of the level before, written by this workgroup, are visible to it
        const int lo = rv.level_start[level * segs], hi = rv.level_start[(level + 1) * segs];  // (the scan wrote [0, (maxd + 1) * segs])
        if (lo >= count || hi > count || hi < lo) break;  // (uniform; the levels of alive vertices have no gap)
        for (int pos = lo + t; pos < hi; pos += TPB) {
            const int p = rv.out_parent[pos];
            if (p >= 0 && p < lo) rv.out_vcost[pos] = rv.out_vcost[p] + edge(p, pos);
        }
    }
}

__global__ __launch_bounds__(TPB) void rrt_reroot_cost_kernel(RerootView rv) {
    reroot_cost_levels(rv, [&](int p, int pos) { return sqrt_u32(dist2(rv.out_nodes[p], rv.out_nodes[pos])); });
}

}  // namespace rrtdev
