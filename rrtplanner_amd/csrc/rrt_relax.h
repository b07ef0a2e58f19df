// rrt_relax.h -- relax a finished straight-line tree to the shortest-path tree from its root over the graph of its own vertices: the
// edges u -> v with d2(u, v) < R that are free on the context's grid, walked from u to v, and every vertex's old parent edge (which
// stands tested on this grid and may be longer than the radius).  The vertices stay; every parent is chosen again.
//
//   costs    c[0] = 0,  c[v] = min over u in E(v) of c[u] + sqrt((double)d2(u, v))  in f64, the loop's own sum.  f64 addition is monotone
//            and no edge is negative, so the solution is unique and any order of relaxations that starts from the tree's own costs (a
//            valid upper bound: c[v] == c[parent[v]] + d bit for bit) reaches it.
//   parents  behind the costs, in a pass of its own: the u in E(v) with c[u] + d == c[v] and (c[u], u) < (c[v], v), the smallest (c[u], u).
//
// The input is dense: the tree arrays [0, j), or the kept view with its parents renumbered, as rrt_reroot.h takes them.  The kernels:
//
//   1. buckets  a CSR of the vertices by cell of edge 2^shift, 2^(2 shift) >= R, so that every u with d2(u, v) < R lies in the 3 x 3 cells
//      around v's.  The cell number is cx * ncy + cy: the three cells of a column of the box are one contiguous range of the CSR.
//      rrt_relax_cell_kernel     cell_of[k], the count of every cell (integer atomics: a sum), cost[k] = the input cost.
//      rrt_relax_scan_kernel     one workgroup: cell_start = exclusive scan of the counts; the counts become the cells' cursors.
//      rrt_relax_fill_kernel     items[cursor++] = k, with k's point beside it.  The order inside a cell is that of the atomics: no result depends on it, since
//                                every choice below is a minimum over the whole box in an order of its own.
//      (rrt_field.h runs the same three kernels for its buckets: without parents, cost and pos_of, which may be null, and with the two
//      arrays only it asks for, item_cost and cell_min.)
//   2. rrt_relax_round_kernel    one round, one wavefront per vertex v, grid-stride.  A vertex scans only if a cell of its box or its
//      old parent's cell changed in the round before (dirty_in; the first round scans all), and then only the candidates whose own
//      cost fell in that round (changed_in, a flag per item of the CSR): the others it has priced, against a c[v] no lower.  The bound is min(c[v], c[p] + d(p, v)): the
//      old parent needs no test.  The lanes stream the box and price cand = c[u] + d; the candidates below the bound go to a list in
//      the wavefront's LDS, which it walks in ascending (cand, u), testing u -> v (los_wave) until one is free (relax_walk):
//      lines of sight are walked for improving candidates only, in ascending order, and the first free one is the minimum.
//      Costs are relaxed in place (cin == cout): c[v] is written by v's wavefront alone, only ever falls, and is one aligned 8-byte
//      access, so a reader sees a value that some round wrote -- an upper bound that a later round lowers, because the writer marks
//      its cell in dirty_out.  (Between two arrays, cin != cout, a round reads the costs of the round before alone: the variant that
//      DESIGN.md 4.2f3 measured against this one.)  Every round adds its changes to a counter; the host stops after a round that
//      changed nothing.  No kernel waits for another workgroup: rounds are launches.
//   3. rrt_relax_parent_kernel   the parent rule over the final costs, one wavefront per vertex, the same ascending walk over the
//      qualifying u by (c[u], u); the old parent, if it qualifies, bounds the walk and needs no test.  Also counts the fallen vertices.
//   4. the stages of rrt_reroot.h from the pointer jumping on, with these parents and ok = 1 everywhere, and
//      rrt_relax_check_kernel    the costs that rrt_reroot_cost_kernel summed from the root down equal the fixpoint's bit for bit.
// Every index is checked before it is used; what cannot be placed raises err and is not stored.
#pragma once

#include "rrt_tree_dev.h"

namespace rrtdev {

__device__ __forceinline__ double relax_load(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int relax_cell(const RelaxView &xv, uint32_t xy) {
    const int cx = ux(xy) >> xv.shift, cy = uy(xy) >> xv.shift;
    return cx < xv.ncx && cy < xv.ncy ? cx * xv.ncy + cy : -1;
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_cell_kernel(RelaxView xv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= xv.j) return;
    const int cell = relax_cell(xv, xv.nodes[k]);
    const int p = k == 0 || !xv.parent ? 0 : xv.parent[k];  // (the buckets of rrt_field.h have no parents)
    if (cell < 0 || p < 0 || p >= xv.j) atomicOr(xv.err, 1);
    xv.cell_of[k] = cell;
    if (xv.cost) xv.cost[k] = k == 0 ? 0.0 : xv.vcost[k];
    if (cell >= 0) atomicAdd(&xv.cell_fill[cell], 1);
    if (xv.cell_min && cell >= 0) {  // the smallest cost of the cell: the bits of non-negative doubles order like unsigned integers
        const double c = xv.vcost[k];
        atomicMin(&xv.cell_min[cell], (unsigned long long)__double_as_longlong(c > 0.0 ? c : 0.0));  // (-0, a negative cost or a NaN: 0, which bounds them too)
    }
}

// cell_start[0, cells] = exclusive scan of cell_fill[0, cells), and cell_fill[c] = cell_start[c]: the cursor of the fill
__global__ __launch_bounds__(TPB) void rrt_relax_scan_kernel(RelaxView xv) {
    const int t = (int)threadIdx.x;
    const int cells = xv.ncx * xv.ncy;  // (uniform; the host keeps it within RELAX_MAX_CELLS)
    uint32_t carry = 0;
    int par = 0;
    for (int base = 0; base < cells; base += TPB) {
        const int c = base + t;
        const uint32_t v = c < cells ? (uint32_t)xv.cell_fill[c] : 0u;
        const uint32_t incl = wave_incl_sum_u32(v);
        const WgScan s = wg_scan_step(incl, par);
        if (c < cells) {
            const int32_t start = (int32_t)(carry + s.before + incl - v);
            xv.cell_start[c] = start;
            xv.cell_fill[c] = start;
        }
        carry += s.total;
    }
    if (t == 0) xv.cell_start[cells] = (int32_t)carry;
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_fill_kernel(RelaxView xv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= xv.j) return;
    const int cell = xv.cell_of[k];
    if (cell < 0 || cell >= xv.ncx * xv.ncy) return;  // (the cell kernel raised err)
    const int pos = atomicAdd(&xv.cell_fill[cell], 1);
    if (xv.pos_of) xv.pos_of[k] = pos;
    if (pos >= 0 && pos < xv.j) {
        xv.items[pos] = k;
        xv.item_xy[pos] = xv.nodes[k];
        if (xv.item_cost) xv.item_cost[pos] = xv.vcost[k];
    } else {
        atomicOr(xv.err, 1);
    }
}

// The box of v's cell: three ranges of the CSR, one per column cx - 1 .. cx + 1 (an empty range for a column outside the grid).
struct RelaxBox {
    int lo[3], hi[3];
};
__device__ __forceinline__ RelaxBox relax_box(const RelaxView &xv, uint32_t xy) {
    const int cx = ux(xy) >> xv.shift, cy = uy(xy) >> xv.shift;
    const int y0 = max(cy - 1, 0), y1 = min(cy + 1, xv.ncy - 1);
    RelaxBox b;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int x = cx - 1 + c;
        const bool in = x >= 0 && x < xv.ncx;
        b.lo[c] = in ? xv.cell_start[x * xv.ncy + y0] : 0;
        b.hi[c] = in ? min(xv.cell_start[x * xv.ncy + y1 + 1], xv.j) : 0;
        if (b.lo[c] < 0) b.lo[c] = b.hi[c];
    }
    return b;
}

// The walk both passes make over the candidates u of vertex v (u != v, d2(u, v) < R, in v's box) whose key -- cand = c[u] + d in a
// round; c[u], for those with cand == c[v], in the parent pass -- lies strictly below the bound (bk, bu): the smallest (key, u) among
// those whose line u -> v is free.  Returns that u and leaves (key, u) in the bound; -1: none, the bound as it was.
// The lanes stream the box, 256 items a step with the loads of a step in flight together, and list what qualifies in the wavefront's
// own LDS (lk, lu: RELAX_LIST entries, placed by ballot).  Then the list is walked in ascending (key, u), each entry tested by los_wave
// until one is free: the others of the list are larger.  A box with more qualifying candidates than the list holds is taken in
// chunks, each of what fits, in scan order; a free candidate found tightens the bound for the chunks behind it, so the result is
// the minimum over all of them.  Uniform over the wavefront.
// changed: null, or a flag per item of the CSR; then only the flagged items are candidates (a round: those whose cost fell in the
// round before.  The others were priced against a c[v] that has not risen since, and neither their cost nor their walk has changed).
template <bool PARENTS>
__device__ __forceinline__ int relax_walk(const RelaxView &xv, const double *cost, const uint8_t *changed, const RelaxBox &box, int v, uint32_t xy, double cv,
                                          double &bk, uint32_t &bu, int lane, volatile RRT_LDS double *lk, volatile RRT_LDS uint32_t *lu, uint32_t &n_los, uint32_t &n_priced) {
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
            double c4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = at + 64 * g + lane;
                int u = i < hi ? xv.items[i] : -1;
                if (u < 0 || u >= xv.j || u == v || (changed && changed[i] == 0)) u = -1;
                u4[g] = u;
                p4[g] = u >= 0 ? xv.item_xy[i] : 0u;
                c4[g] = u >= 0 ? relax_load(&cost[u]) : 0.0;
            }
            int done = 0;  // steps of 64 items listed
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (full || at + 64 * g >= hi) continue;  // (uniform)
                const uint32_t u = (uint32_t)u4[g], d2 = dist2(p4[g], xy);
                const bool near = u4[g] >= 0 && (int64_t)d2 < xv.R;
                const double cand = c4[g] + sqrt_u32(d2), key = PARENTS ? c4[g] : cand;
                n_priced += near ? 1u : 0u;
                const bool q = near && (!PARENTS || cand == cv) && key_lt(key, u, bk, bu);
                const unsigned long long mask = __ballot(q);
                const int n = (int)__builtin_popcountll(mask);
                if (K + n > RELAX_LIST) {  // (uniform) the list is full: this step's items from here on belong to the next chunk
                    full = true;
                    continue;
                }
                if (q) {
                    const int pos = K + (int)__builtin_popcountll(mask & below);
                    lk[pos] = key;
                    lu[pos] = u;
                }
                K += n;
                ++done;
            }
            at += 64 * (full ? done : 4);
        }
        __builtin_amdgcn_wave_barrier();
        double fk = -1.0;  // the last entry tested and found blocked: (fk, fu); every key is >= 0
        uint32_t fu = 0;
        for (;;) {
            double mk = f64_inf();
            uint32_t mu = NONE;
            for (int t = lane; t < K; t += 64) {
                const double key = lk[t];
                const uint32_t u = lu[t];
                if (key_lt(fk, fu, key, u) && key_lt(key, u, mk, mu)) {
                    mk = key;
                    mu = u;
                }
            }
            wave_min_f64_idx(mk, mu);
            if (mu == NONE || mu >= (uint32_t)xv.j) break;
            int cells;
            ++n_los;
            if (los_wave(xv.og, xv.H, xv.nodes[mu], xy, lane, cells)) {
                bk = mk;
                bu = mu;
                found = (int)mu;
                break;
            }
            fk = mk;
            fu = mu;
        }
        __builtin_amdgcn_wave_barrier();
        if (c >= 3) return found;
    }
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_round_kernel(RelaxView xv, const double *cin, double *cout, const uint8_t *dirty_in, uint8_t *dirty_out,
                                                                    const uint8_t *changed_in, uint8_t *changed_out, int32_t first) {
    __shared__ double lk_lds[RELAX_TPB / 64][RELAX_LIST];
    __shared__ uint32_t lu_lds[RELAX_TPB / 64][RELAX_LIST];
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    volatile RRT_LDS double *lk = (volatile RRT_LDS double *)&lk_lds[(threadIdx.x >> 6) & (RELAX_TPB / 64 - 1)][0];  // of this wavefront alone
    volatile RRT_LDS uint32_t *lu = (volatile RRT_LDS uint32_t *)&lu_lds[(threadIdx.x >> 6) & (RELAX_TPB / 64 - 1)][0];
    const int j = xv.j, cells = xv.ncx * xv.ncy;
    uint32_t n_los = 0, n_priced = 0, n_changed = 0;
    for (int v = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); v < j; v += (int)gridDim.x * waves) {  // (v is wave-uniform)
        if (v == 0) continue;
        const uint32_t xy = xv.nodes[v];
        const int p = xv.parent[v], cell = xv.cell_of[v];
        if (p < 0 || p >= j || cell < 0 || cell >= cells) continue;  // (the cell kernel raised err)
        if (!first) {  // lanes 0 .. 8: the cells of the box; lane 9: the old parent's cell
            const int cx = cell / xv.ncy + lane / 3 - 1, cy = cell % xv.ncy + lane % 3 - 1;
            int look = lane < 9 && cx >= 0 && cx < xv.ncx && cy >= 0 && cy < xv.ncy ? cx * xv.ncy + cy : -1;
            if (lane == 9) look = xv.cell_of[p];
            if (__ballot(look >= 0 && look < cells && dirty_in[look] != 0) == 0) continue;
        }
        const RelaxBox box = relax_box(xv, xy);
        const double cv = relax_load(&cin[v]);
        const double pc = relax_load(&cin[p]) + sqrt_u32(dist2(xv.nodes[p], xy));
        double bound = pc < cv ? pc : cv;
        uint32_t bu = 0;  // (strictly below the bound)
        relax_walk<false>(xv, cin, first ? nullptr : changed_in, box, v, xy, cv, bound, bu, lane, lk, lu, n_los, n_priced);
        // (between two arrays a vertex that scanned always stores: the array it writes holds its cost of two rounds ago)
        if (lane == 0 && (bound < cv || cout != cin)) __hip_atomic_store(&cout[v], bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bound < cv) {
            const int at = xv.pos_of[v];
            if (lane == 0) {
                dirty_out[cell] = (uint8_t)1;
                if (at >= 0 && at < j) changed_out[at] = (uint8_t)1;
                else atomicOr(xv.err, 1);
            }
            ++n_changed;
        }
    }
    // the counters of the whole loop, once per wavefront: the walks are uniform, so lane 0's n_los and n_changed are the wavefront's
    const uint32_t priced = wave_sum_u32(n_priced);
    if (lane == 0) {
        if (n_changed) atomicAdd(&xv.stats[RELAX_CHANGES], (unsigned long long)n_changed);
        if (n_los) atomicAdd(&xv.stats[RELAX_LOS], (unsigned long long)n_los);
        if (priced) atomicAdd(&xv.stats[RELAX_PRICED], (unsigned long long)priced);
    }
}

__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_parent_kernel(RelaxView xv) {
    __shared__ double lk_lds[RELAX_TPB / 64][RELAX_LIST];
    __shared__ uint32_t lu_lds[RELAX_TPB / 64][RELAX_LIST];
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    volatile RRT_LDS double *lk = (volatile RRT_LDS double *)&lk_lds[(threadIdx.x >> 6) & (RELAX_TPB / 64 - 1)][0];  // of this wavefront alone
    volatile RRT_LDS uint32_t *lu = (volatile RRT_LDS uint32_t *)&lu_lds[(threadIdx.x >> 6) & (RELAX_TPB / 64 - 1)][0];
    const int j = xv.j, cells = xv.ncx * xv.ncy;
    uint32_t n_los = 0, n_priced = 0, n_fell = 0;
    for (int v = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); v < j; v += (int)gridDim.x * waves) {  // (v is wave-uniform)
        if (v == 0) {
            if (lane == 0) xv.new_parent[0] = -1;
            continue;
        }
        const uint32_t xy = xv.nodes[v];
        const int p = xv.parent[v], cell = xv.cell_of[v];
        if (p < 0 || p >= j || cell < 0 || cell >= cells) {  // (the cell kernel raised err)
            if (lane == 0) xv.new_parent[v] = -1;
            continue;
        }
        const RelaxBox box = relax_box(xv, xy);
        const double cv = xv.cost[v], pc = xv.cost[p];
        // the old parent qualifies without a walk; then only a smaller (c[u], u) can take its place
        const bool keeps = pc + sqrt_u32(dist2(xv.nodes[p], xy)) == cv && key_lt(pc, (uint32_t)p, cv, (uint32_t)v);
        double bk = keeps ? pc : cv;
        uint32_t bu = keeps ? (uint32_t)p : (uint32_t)v;
        const int u = relax_walk<true>(xv, xv.cost, nullptr, box, v, xy, cv, bk, bu, lane, lk, lu, n_los, n_priced);
        const int np = u >= 0 ? u : keeps ? p : -1;
        if (lane == 0) {
            xv.new_parent[v] = np;
            if (np < 0) atomicOr(xv.err, 1);  // (no edge gives the vertex its cost: the costs are no fixpoint)
        }
        if (cv < xv.vcost[v]) ++n_fell;
    }
    const uint32_t priced = wave_sum_u32(n_priced);
    if (lane == 0) {
        if (n_fell) atomicAdd(&xv.stats[RELAX_FELL], (unsigned long long)n_fell);
        if (n_los) atomicAdd(&xv.stats[RELAX_LOS], (unsigned long long)n_los);
        if (priced) atomicAdd(&xv.stats[RELAX_PRICED], (unsigned long long)priced);
    }
}

// behind rrt_reroot_cost_kernel: the cost of every new number, summed from the root down, has the bits of the fixpoint's
__global__ __launch_bounds__(RELAX_TPB) void rrt_relax_check_kernel(RelaxView xv, const int32_t *src, const double *out_vcost, const int32_t *count) {
    const int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pos >= xv.j) return;
    if (*count != xv.j) {  // (every vertex hangs on the root: the old parent edge is always a candidate)
        atomicOr(xv.err, 1);
        return;
    }
    const int k = src[pos];
    if (k < 0 || k >= xv.j || __double_as_longlong(out_vcost[pos]) != __double_as_longlong(xv.cost[k])) atomicOr(xv.err, 1);
}

}  // namespace rrtdev
