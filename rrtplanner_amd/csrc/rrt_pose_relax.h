// rrt_pose_relax.h -- relax a finished DUBINS tree to the shortest-path tree from its root over the graph of its own poses.
//
// rrt_relax.h serves the straight-line planners; its semantics are this file's with another edge.  A vertex's pose (x, y, h) is
// sampled and fixed, and the word u -> v is a function of the two poses alone: the directed graph of the poses has a shortest-path
// tree like any other.  The candidate edges into v != 0 are the u != v with d2(u, v) < R whose shortest word from pose u to pose v
// (dub_between_dev with the query's DubCfg: the planner's bits) is finite and sweeps free on the context's grid -- the sweep plan(),
// connect_poses and keep_pose_tree make, from u to v --, and the old parent edge, which is not swept again and may be longer than
// the radius.  Costs and parents are rrt_relax.h's rules with len(u -> v) for sqrt(d2).
//
// The buckets are rrt_relax.h's kernels (cell, scan, fill), launched as they are.  Then:
//
//   1. rrt_pose_relax_item_kernel    one vertex per lane: the heading byte of every item of the CSR beside its point, so that the stream of
//                                    a box loads nothing through the vertex number but the cost; and plen[v], the length of the old parent
//                                    edge, evaluated once: every round's bound needs it.
//   2. rrt_pose_relax_round_kernel   one round, one wavefront per vertex v, grid-stride, the dirty cells and the changed items of
//                                    rrt_relax_round_kernel.  A word costs some 2000 instructions, so the lanes that stream the 3 x 3
//                                    box screen first: chord_lower_bound(c[u], d2) (rrt_cell_stream.h) is a float never above
//                                    c[u] + len(u -> v), and a candidate whose screen is not below the bound min(c[v], c[p] + plen[v])
//                                    could not have improved.  The survivors go to a list in the wavefront's LDS (cost, number, point,
//                                    heading: POSE_RELAX_LIST entries); the list is taken 64 entries a step, every lane evaluating ONE
//                                    word, and the entries whose c[u] + len is still below the bound are swept in ascending (cand, u)
//                                    by dub_sweep_wave from u to v until one is free: the others of the step are larger, and the next
//                                    step meets the tightened bound.  More survivors than the list holds are taken in chunks, a hit
//                                    tightening the screen of the chunks behind it.  Costs are relaxed in place as rrt_relax.h says.
//   3. rrt_pose_relax_parent_kernel  the parent rule over the final costs by the same walk: the screen keeps the u whose bound is not
//                                    above c[v], the words pick those with c[u] + len == c[v], and they are swept in ascending
//                                    (c[u], u) below the old parent's key, if that one qualifies -- it needs no sweep.
//   4. behind the order of rrt_reroot.h (pointer jumping, level, scan, place, parent):
//      rrt_pose_relax_word_kernel    one new number per lane: its heading byte gathered into the new order, and the word from its new
//                                    parent's pose to its own -- the j words in parallel, not inside one workgroup's serial loop;
//      rrt_pose_relax_cost_kernel    reroot_cost_levels (rrt_reroot.h) over those words: vcost[parent] + word, level by level;
//      rrt_relax_check_kernel        as it is: the sums equal the fixpoint bit for bit, else err.
// Every index is checked before it is used; what cannot be placed raises err and is not stored.  No kernel waits for another workgroup.
// (The view, the constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_relax.h"
#include "rrt_reroot.h"
#include "rrt_cell_stream.h"
#include "rrt_dubins_dev.h"

namespace rrtdev {

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_item_kernel(PoseRelaxView pv) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    const RelaxView &xv = pv.xv;
    const DubCfg dc = dub_cfg_fill<RELAX_TPB>((RRT_LDS double *)htab_s, pv.rho, pv.nh, pv.W, xv.H);
    __syncthreads();
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= xv.j) return;
    const int hk = (int)pv.heading[k];
    const int pos = xv.pos_of[k], cell = xv.cell_of[k];
    if (cell >= 0 && pos >= 0 && pos < xv.j) pv.item_h[pos] = (uint8_t)hk;  // (a vertex outside the cells has no item: the cell kernel raised err)
    double len = 0.0;
    if (k > 0) {
        const int p = xv.parent[k];
        len = p >= 0 && p < xv.j ? dub_between_dev(xv.nodes[p], (int)pv.heading[p], xv.nodes[k], hk, dc).len : f64_inf();
    }
    pv.plen[k] = len;
}

// The LDS of one wavefront's list: what a survivor of the screen carries to its word and its sweep.
struct PoseRelaxList {
    volatile RRT_LDS double *c;    // c[u]
    volatile RRT_LDS uint32_t *u;  // the vertex
    volatile RRT_LDS uint32_t *p;  // its point
    volatile RRT_LDS uint8_t *h;   // its heading index
};

// relax_walk (rrt_relax.h) for poses: over the candidates u of vertex v (u != v, d2(u, v) < R, in v's box) whose key -- cand = c[u] +
// len(u -> v) in a round; c[u], for those with cand == c[v], in the parent pass -- lies strictly below the bound (bk, bu), the smallest
// (key, u) among those whose sweep u -> v is free.  Returns that u and leaves (key, u) in the bound; -1: none, the bound as it was.
// Uniform over the wavefront.  changed: as relax_walk's.
template <bool PARENTS>
__device__ __forceinline__ int pose_relax_walk(const PoseRelaxView &pv, const DubCfg &dc, const uint8_t *changed, const RelaxBox &box, int v, uint32_t xy, int hv,
                                               double cv, double &bk, uint32_t &bu, int lane, const PoseRelaxList &ls, uint32_t &n_sweeps, uint32_t &n_words) {
    const RelaxView &xv = pv.xv;
    const unsigned long long below = (1ull << lane) - 1ull;
    int found = -1;
    int c = 0, at = box.lo[0];  // where the scan stands: range c of the box, item `at` of the CSR (wave-uniform)
    for (;;) {
        int K = 0;  // entries of the list
        bool full = false;
        while (c < 3 && !full) {
            const int hi = c == 0 ? box.hi[0] : c == 1 ? box.hi[1] : box.hi[2];  // (selects: the box stays in registers)
            if (at >= hi) {
                ++c;
                at = c == 1 ? box.lo[1] : box.lo[2];
                continue;
            }
            int u4[4];
            uint32_t p4[4];
            uint8_t h4[4];
            double c4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = at + 64 * g + lane;
                int u = i < hi ? xv.items[i] : -1;
                if (u < 0 || u >= xv.j || u == v || (changed && changed[i] == 0)) u = -1;
                u4[g] = u;
                p4[g] = u >= 0 ? xv.item_xy[i] : 0u;
                h4[g] = u >= 0 ? pv.item_h[i] : (uint8_t)0;
                c4[g] = u >= 0 ? relax_load(&xv.cost[u]) : 0.0;
            }
            int done = 0;  // steps of 64 items listed
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (full || at + 64 * g >= hi) continue;  // (uniform)
                const uint32_t u = (uint32_t)u4[g], d2 = dist2(p4[g], xy);
                const bool near = u4[g] >= 0 && (int64_t)d2 < xv.R;
                // the screen: lb <= c[u] + len.  A round wants c[u] + len < bound; the parent pass c[u] + len == c[v] and (c[u], u) below the bound
                const double lb = (double)chord_lower_bound(c4[g], d2);
                const bool q = near && (PARENTS ? lb <= cv && key_lt(c4[g], u, bk, bu) : lb < bk);
                const unsigned long long mask = __ballot(q);
                const int n = (int)__builtin_popcountll(mask);
                if (K + n > POSE_RELAX_LIST) {  // (uniform) the list is full: this step's items from here on belong to the next chunk
                    full = true;
                    continue;
                }
                if (q) {
                    const int pos = K + (int)__builtin_popcountll(mask & below);
                    ls.c[pos] = c4[g];
                    ls.u[pos] = u;
                    ls.p[pos] = p4[g];
                    ls.h[pos] = h4[g];
                }
                K += n;
                ++done;
            }
            at += 64 * (full ? done : 4);
        }
        __builtin_amdgcn_wave_barrier();
        for (int base = 0; base < K; base += 64) {  // (uniform) one word per lane, then the sweeps of this step in ascending key
            const int t = base + lane;
            const bool have = t < K;
            const double cu = have ? ls.c[t] : f64_inf();
            const uint32_t u = have ? ls.u[t] : NONE, pu = have ? ls.p[t] : 0u;
            const int hu = have ? (int)ls.h[t] : 0;
            dub_path_t pth = dub_no_path();
            if (have && u < (uint32_t)xv.j) pth = dub_between_dev(pu, hu, xy, hv, dc);
            n_words += (uint32_t)(K - base < 64 ? K - base : 64);
            const double cand = cu + pth.len, key = PARENTS ? cu : cand;
            bool pend = have && pth.word != DUB_NONE && (!PARENTS || cand == cv) && key_lt(key, u, bk, bu);
            for (;;) {
                double mk = pend ? key : f64_inf();
                uint32_t mu = pend ? u : NONE;
                wave_min_f64_idx(mk, mu);
                if (mu == NONE) break;
                const int l = (int)__builtin_ctzll(__ballot(pend && u == mu));  // (a vertex sits in one lane)
                const dub_path_t wp = dub_path_from_lane(pth, l);
                const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)pu, l);
                const int ha = __builtin_amdgcn_readlane(hu, l);
                int cc = 0;
                ++n_sweeps;
                const bool ok = dub_sweep_wave(xv.og, dc, a, ha, xy, wp, lane, cc);
                if (lane == l) pend = false;
                if (ok) {  // the cheapest free one of the step: what is left of it is larger
                    bk = mk;
                    bu = mu;
                    found = (int)mu;
                    break;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (c >= 3) return found;
    }
}

#define RRT_POSE_RELAX_LDS(ls, dc)                                                                                                  \
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

// One round over the vertices of this workgroup's wavefronts.  OPEN (rrt_pose_reroot.h: the shortest-path tree from a root that the old
// tree does not hang on): a vertex other than the root may have no old parent (parent outside [0, j): its only edges are the swept
// ones), and a cost may be +inf -- chord_lower_bound(inf, d2) is inf, so an unreached u never survives a screen, and a bound of inf
// lets every finite candidate through.  With OPEN false the code is rrt_pose_relax_round_kernel's as it always was.
template <bool OPEN>
__device__ __forceinline__ void pose_relax_round(const PoseRelaxView &pv, const DubCfg &dc, const PoseRelaxList &ls, const uint8_t *dirty_in, uint8_t *dirty_out,
                                                 const uint8_t *changed_in, uint8_t *changed_out, int32_t first) {
    const RelaxView &xv = pv.xv;
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = xv.j, cells = xv.ncx * xv.ncy;
    uint32_t n_sweeps = 0, n_words = 0, n_changed = 0;
    for (int v = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); v < j; v += (int)gridDim.x * waves) {  // (v is wave-uniform)
        if (v == 0) continue;
        const uint32_t xy = xv.nodes[v];
        const int p = xv.parent[v], cell = xv.cell_of[v];
        const bool has_p = p >= 0 && p < j;
        if ((!OPEN && !has_p) || cell < 0 || cell >= cells) continue;  // (the cell kernel raised err)
        if (!first) {  // lanes 0 .. 8: the cells of the box; lane 9: the old parent's cell
            const int cx = cell / xv.ncy + lane / 3 - 1, cy = cell % xv.ncy + lane % 3 - 1;
            int look = lane < 9 && cx >= 0 && cx < xv.ncx && cy >= 0 && cy < xv.ncy ? cx * xv.ncy + cy : -1;
            if (lane == 9) look = has_p ? xv.cell_of[p] : -1;
            if (__ballot(look >= 0 && look < cells && dirty_in[look] != 0) == 0) continue;
        }
        const RelaxBox box = relax_box(xv, xy);
        const double cv = relax_load(&xv.cost[v]);
        const double pc = has_p ? relax_load(&xv.cost[p]) + pv.plen[v] : f64_inf();
        double bound = pc < cv ? pc : cv;
        uint32_t bu = 0;  // (strictly below the bound)
        pose_relax_walk<false>(pv, dc, first ? nullptr : changed_in, box, v, xy, (int)pv.heading[v], cv, bound, bu, lane, ls, n_sweeps, n_words);
        if (bound < cv) {
            const int at = xv.pos_of[v];
            if (lane == 0) {
                __hip_atomic_store(&xv.cost[v], bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                dirty_out[cell] = (uint8_t)1;
                if (at >= 0 && at < j) changed_out[at] = (uint8_t)1;
                else atomicOr(xv.err, 1);
            }
            ++n_changed;
        }
    }
    // the counters of the whole loop, once per wavefront: the walks are uniform, so lane 0's are the wavefront's
    if (lane == 0) {
        if (n_changed) atomicAdd(&xv.stats[RELAX_CHANGES], (unsigned long long)n_changed);
        if (n_sweeps) atomicAdd(&xv.stats[RELAX_LOS], (unsigned long long)n_sweeps);
        if (n_words) atomicAdd(&xv.stats[RELAX_PRICED], (unsigned long long)n_words);
    }
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_round_kernel(PoseRelaxView pv, const uint8_t *dirty_in, uint8_t *dirty_out, const uint8_t *changed_in,
                                                                         uint8_t *changed_out, int32_t first) {
    RRT_POSE_RELAX_LDS(ls, dc);
    pose_relax_round<false>(pv, dc, ls, dirty_in, dirty_out, changed_in, changed_out, first);
}

// The parent rule over the final costs.  OPEN: a vertex whose cost is +inf was not reached: it gets no parent and raises no err (the
// link kernel cuts it), and RELAX_FELL counts the vertices that were reached, the root among them, instead of those whose cost fell.
template <bool OPEN>
__device__ __forceinline__ void pose_relax_parents(const PoseRelaxView &pv, const DubCfg &dc, const PoseRelaxList &ls) {
    const RelaxView &xv = pv.xv;
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = xv.j, cells = xv.ncx * xv.ncy;
    uint32_t n_sweeps = 0, n_words = 0, n_fell = 0;
    for (int v = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); v < j; v += (int)gridDim.x * waves) {  // (v is wave-uniform)
        if (v == 0) {
            if (lane == 0) xv.new_parent[0] = -1;
            if (OPEN) ++n_fell;
            continue;
        }
        const uint32_t xy = xv.nodes[v];
        const int p = xv.parent[v], cell = xv.cell_of[v];
        const bool has_p = p >= 0 && p < j;
        if ((!OPEN && !has_p) || cell < 0 || cell >= cells) {  // (the cell kernel raised err)
            if (lane == 0) xv.new_parent[v] = -1;
            continue;
        }
        const double cv = xv.cost[v], pc = has_p ? xv.cost[p] : f64_inf();
        if (OPEN && !(cv < f64_inf())) {  // (uniform) not reached
            if (lane == 0) xv.new_parent[v] = -1;
            continue;
        }
        const RelaxBox box = relax_box(xv, xy);
        // the old parent qualifies without a sweep; then only a smaller (c[u], u) can take its place
        const bool keeps = has_p && pc + pv.plen[v] == cv && key_lt(pc, (uint32_t)p, cv, (uint32_t)v);
        double bk = keeps ? pc : cv;
        uint32_t bu = keeps ? (uint32_t)p : (uint32_t)v;
        const int u = pose_relax_walk<true>(pv, dc, nullptr, box, v, xy, (int)pv.heading[v], cv, bk, bu, lane, ls, n_sweeps, n_words);
        const int np = u >= 0 ? u : keeps ? p : -1;
        if (lane == 0) {
            xv.new_parent[v] = np;
            if (np < 0) atomicOr(xv.err, 1);  // (no edge gives the vertex its cost: the costs are no fixpoint)
        }
        if (OPEN) ++n_fell;
        else if (cv < xv.vcost[v]) ++n_fell;
    }
    // (the sweeps and words of this pass are not counted: the counters are the rounds', each of which meets a pair at most once)
    if (lane == 0 && n_fell) atomicAdd(&xv.stats[RELAX_FELL], (unsigned long long)n_fell);
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_parent_kernel(PoseRelaxView pv) {
    RRT_POSE_RELAX_LDS(ls, dc);
    pose_relax_parents<false>(pv, dc, ls);
}
#undef RRT_POSE_RELAX_LDS

// behind rrt_reroot_parent_kernel: the heading byte of every new number, and the word from its new parent's pose to its own
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_relax_word_kernel(PoseRelaxView pv, RerootView rv, uint8_t *out_heading, double *word) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    const DubCfg dc = dub_cfg_fill<RELAX_TPB>((RRT_LDS double *)htab_s, pv.rho, pv.nh, pv.W, pv.xv.H);
    __syncthreads();
    const int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int j = rv.j, count = rv.head[REROOT_COUNT];
    if (pos >= count || pos >= j) return;
    const int k = rv.src[pos];
    if (k < 0 || k >= j) {  // (rrt_reroot_parent_kernel raised err)
        out_heading[pos] = (uint8_t)0;
        word[pos] = f64_inf();
        return;
    }
    const int hk = (int)pv.heading[k];
    out_heading[pos] = (uint8_t)hk;
    double len = 0.0;
    if (pos > 0) {
        const int p = rv.out_parent[pos];
        const int kp = p >= 0 && p < pos ? rv.src[p] : -1;
        len = kp >= 0 && kp < j ? dub_between_dev(rv.nodes[kp], (int)pv.heading[kp], rv.nodes[k], hk, dc).len : f64_inf();
    }
    word[pos] = len;
}

__global__ __launch_bounds__(TPB) void rrt_pose_relax_cost_kernel(RerootView rv, const double *word) {
    reroot_cost_levels(rv, [&](int, int pos) { return word[pos]; });
}

}  // namespace rrtdev
