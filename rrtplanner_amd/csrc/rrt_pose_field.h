// rrt_pose_field.h -- the pose cost field of a finished DUBINS tree: rrt_pose_field_kernel and the gather kernel in front of it.
//
// rrt_field.h serves the straight-line planners; a Dubins goal is a pose and its edge a Dubins word.  For every cell g of a window of
// the grid, what rrt_pose_goals.h decides for goal poses on g:
//
//   fixed arrival heading H   the pose (g, H): c[k] = vcost[k] + dub_between(pose_k, (g, H)).len over the vertices k in [0, j); the answer
//                             is the smallest (c, k) among the vertices whose sweep is free.  heading out: H.
//   any heading (-1)          over all pairs (heading a, vertex k) whose sweep pose_k -> (g, a) is free, the lexicographically smallest
//                             (cost, a, k).  That equals "per heading the (cost, index)-first vertex, then the (cost, heading)-first
//                             heading", which is what the planner's connect_poses answers for the pose (g, -1): the minimum over a of
//                             (min over k of (c, k), a) orders by cost first, then by a, and within one a by k.  heading out: that a.
//   A blocked cell, or a free one that nothing reaches: vertex -1, cost +inf, heading -1 (connect_poses echoes the heading it was asked
//   for an unconnected pose; the field writes -1 there).
//
// The pose goals kernel counting-sorts all j vertices for every pose.  A field has what a list of poses has not: the same vertices serve
// every cell, the same bound serves every heading of a cell, and neighbouring cells nearly always share their winner.  So:
//
//   1. buckets  rrt_relax.h's CSR over the dense input (rrt_relax_cell / scan / fill_kernel, launched by the host), by cell of edge
//      2^shift, with item_cost and cell_min as rrt_field.h takes them, and rrt_pose_field_item_kernel: the heading byte of every item
//      beside its point (item_h), one item per lane.
//   2. rrt_pose_field_kernel  one wavefront per cell; a wavefront takes a run of consecutive cells of one column (pv.run of them, at most
//      POSE_FIELD_RUN: the host shortens the runs of a small window until there are wavefronts for every CU -- a cell that nothing reaches
//      costs its wavefront a sweep for every pair, and the cells behind it in the run wait), runs grid-stride.  The key of a pair is (cost, a << 18 | k): j <= 2^18 and nh <= 256, so the 32-bit part orders by (a, k) and is never NONE.
//      first    the winner (k, a) of the cell before it in the run: one word, one sweep.  If it is free its key is the bound from the start.
//      buckets  lb(b) = chord_lower_bound(cell_min[b], d2min(g, square of b)) (rrt_cell_stream.h); the buckets with lb <= best are listed
//               in the wavefront's LDS and walked in ascending (lb, b) while lb <= best, which falls on the way.  Without a bound the
//               3 x 3 buckets around the cell come first, as in rrt_field.h, and the scan leaves them out: a pair is met once.
//      screen   the lanes stream the items of a bucket; a vertex with vb = chord_lower_bound(item_cost, d2(k, g)) <= best joins the
//               list of survivors (cost, number, point, heading: POSE_FIELD_LIST entries).
//      pairs    when the list is full, and behind the last bucket, the survivors are expanded to (vertex, heading) pairs, heading over
//               [heading_lo, heading_hi) -- one heading, or all nh --, vertex-major, 64 pairs a step, one per lane.  A lane whose vertex
//               still has vb <= best evaluates its word ONCE; the pairs whose key is below the best are swept by the wavefront in
//               ascending key until one is free (pose_goal_bounded's inner loop): the others of the step are larger, and the next step
//               meets the tightened bound.  In any-heading mode the best over all headings is one bound per cell: the first step is
//               all headings of the first survivor of the nearest bucket, and as soon as one of them connects every later vertex is
//               screened against it.
//
// Why the bounds hold.  chord_lower_bound(V, d2) is a float that lies below the f64 value V + sqrt(d2) by more than every rounding on
// its way (the margins are argued beside it; the Dubins loop and connect_poses stand on the same ones), and a word is never shorter
// than its chord.  So vb <= item_cost + len(k -> (g, a)) for EVERY heading a: the same bound serves all headings of the cell.  For a
// bucket, cell_min <= vcost[k] and d2min <= d2(k, g) for every k of b, so cell_min + sqrt(d2min) <= vcost[k] + sqrt(d2(k, g)) and lb lies
// below that too; moreover (float), the hardware root, the float sum and the product with a positive constant are monotone, so
// lb <= vb: bucket bound <= vertex bound <= every computed cost through that vertex, at every heading.  The comparisons are <=, not <:
// a bound clamped to 0 can equal a cost of 0, and a pair of equal cost and lower (heading, vertex) still wins.  (rrt_field.h's exact f64
// bound, field_may_beat, does not carry over: a computed word length can fall below the computed chord by a rounding, which the
// slackened float bound absorbs.)
// A pair is skipped only through such a bound above the cost of a pair that swept free, and left unswept only because its key is not
// below a key that swept free; the best only falls.  So the answer is the minimum over all free pairs whatever the order of the
// buckets, the chunks and the steps: connect_poses' bit for bit, the words being dub_between_dev's with the same DubCfg and the sweeps
// dub_sweep_wave's.
// The tree arrays are only read.  Every index is checked before it is used; what cannot be placed raises err or is skipped.  No kernel
// waits for another workgroup.  stats: free cells decided, buckets visited, words evaluated, sweeps run.
// (The view, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_cell_stream.h"
#include "rrt_dubins_dev.h"

namespace rrtdev {

// the heading byte of every item of the CSR beside its point: one item per lane
__global__ __launch_bounds__(RELAX_TPB) void rrt_pose_field_item_kernel(PoseFieldView pv) {
    const RelaxView &xv = pv.xv;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= xv.j) return;
    const int u = xv.items[i];
    if (u < 0 || u >= xv.j) {  // (a vertex outside the cells left a hole: the cell kernel raised err)
        pv.item_h[i] = (uint8_t)0;
        return;
    }
    const int h = (int)pv.heading[u];
    if (h >= pv.nh) atomicOr(xv.err, 1);
    pv.item_h[i] = (uint8_t)h;
}

constexpr int POSE_FIELD_VBITS = 18;  // the vertex in a pair's key: heading << 18 | vertex
static_assert((1 << POSE_FIELD_VBITS) == POSE_FIELD_MAX_J, "the vertex bits of a key hold every vertex the host lets through");

// The LDS of one wavefront: the buckets that may still beat the best, and the survivors of the screen.
struct PoseFieldLists {
    volatile RRT_LDS float *bk;    // lb of a listed bucket
    volatile RRT_LDS uint32_t *bb;  // ... and the bucket
    volatile RRT_LDS double *c;    // vcost of a survivor
    volatile RRT_LDS uint32_t *u;  // the vertex
    volatile RRT_LDS uint32_t *p;  // its point
    volatile RRT_LDS uint8_t *h;   // its heading index
};

struct PoseFieldCount {
    uint32_t cells = 0, buckets = 0, words = 0, sweeps = 0;  // (words: this lane's; the others: the wavefront's)
};

// One pair against the cell: the word from (a, ha) to (xy, hg) of lane-uniform operands, swept.  True: free, and then its key is the best.
__device__ __forceinline__ bool pose_field_try(const PoseFieldView &pv, const DubCfg &dc, uint32_t k, uint32_t a, int ha, double ck, uint32_t xy, int hg, double &bc,
                                               uint32_t &bi, int lane, PoseFieldCount &n) {
    const dub_path_t pth = dub_between_dev(a, ha, xy, hg, dc);
    n.words += lane == 0 ? 1u : 0u;
    ++n.sweeps;
    int cc = 0;
    if (!dub_sweep_wave(pv.xv.og, dc, a, ha, xy, pth, lane, cc)) return false;
    bc = ck + pth.len;
    bi = ((uint32_t)hg << POSE_FIELD_VBITS) | k;
    return true;
}

// The K survivors of the list against the cell xy, expanded to pairs: the smallest key among the free ones below the best (bc, bi)
// becomes the best.  Uniform over the wavefront.
__device__ __forceinline__ void pose_field_flush(const PoseFieldView &pv, const DubCfg &dc, uint32_t xy, double &bc, uint32_t &bi, int lane, const PoseFieldLists &ls,
                                                 int K, PoseFieldCount &n) {
    const RelaxView &xv = pv.xv;
    const int nhd = pv.heading_hi - pv.heading_lo;  // (the host: 1 or nh, at least 1)
    const int pairs = K * nhd;                      // (at most POSE_FIELD_LIST * 256)
    for (int base = 0; base < pairs; base += 64) {
        const int t = base + lane;
        const bool have = t < pairs;
        const int e = have ? t / nhd : 0;
        const int hg = pv.heading_lo + (have ? t - e * nhd : 0);
        const double cu = have ? ls.c[e] : f64_inf();
        const uint32_t u = have ? ls.u[e] : NONE, pu = have ? ls.p[e] : 0u;
        const int hu = have ? (int)ls.h[e] : 0;
        dub_path_t pth = dub_no_path();
        // the screen again: the best may have fallen since the vertex was listed
        const bool eval = have && u < (uint32_t)xv.j && hu < pv.nh && (double)chord_lower_bound(cu, dist2(pu, xy)) <= bc;
        if (eval) {
            pth = dub_between_dev(pu, hu, xy, hg, dc);
            ++n.words;
        }
        const double cand = cu + pth.len;
        const uint32_t key = ((uint32_t)hg << POSE_FIELD_VBITS) | (u & ((1u << POSE_FIELD_VBITS) - 1u));
        bool pend = eval && pth.word != DUB_NONE && key_lt(cand, key, bc, bi);
        for (;;) {
            double mk = pend ? cand : f64_inf();
            uint32_t mi = pend ? key : NONE;
            wave_min_f64_idx(mk, mi);
            if (mi == NONE) break;
            const int l = (int)__builtin_ctzll(__ballot(pend && key == mi));  // (a pair sits in one lane)
            const dub_path_t wp = dub_path_from_lane(pth, l);
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)pu, l);
            const int ha = __builtin_amdgcn_readlane(hu, l);
            int cc = 0;
            ++n.sweeps;
            const bool ok = dub_sweep_wave(xv.og, dc, a, ha, xy, wp, lane, cc);
            if (lane == l) pend = false;
            if (ok) {  // the cheapest free pair of the step: what is left of it is larger
                bc = mk;
                bi = mi;
                break;
            }
        }
    }
}

// The items [lo, hi) of one bucket for the cell xy: the vertices whose bound is not above the best join the list (K entries so far), which
// is flushed as soon as another 64 might not fit.  Uniform over the wavefront.
__device__ __forceinline__ void pose_field_bucket(const PoseFieldView &pv, const DubCfg &dc, int lo, int hi, uint32_t xy, double &bc, uint32_t &bi, int lane,
                                                  const PoseFieldLists &ls, int &K, PoseFieldCount &n) {
    const RelaxView &xv = pv.xv;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int at = lo; at < hi; at += 64) {
        const int i = at + lane;
        int u = i < hi ? xv.items[i] : -1;
        if (u < 0 || u >= xv.j) u = -1;
        const uint32_t p = u >= 0 ? xv.item_xy[i] : 0u;
        const double c = u >= 0 ? xv.item_cost[i] : 0.0;
        const uint8_t h = u >= 0 ? pv.item_h[i] : (uint8_t)0;
        const bool q = u >= 0 && ux(p) < pv.W && uy(p) < xv.H && (double)chord_lower_bound(c, dist2(p, xy)) <= bc;
        const unsigned long long mask = __ballot(q);
        if (q) {  // (K <= POSE_FIELD_LIST - 64 here and at most 64 join)
            const int pos = K + (int)__builtin_popcountll(mask & below);
            ls.c[pos] = c;
            ls.u[pos] = (uint32_t)u;
            ls.p[pos] = p;
            ls.h[pos] = h;
        }
        K += (int)__builtin_popcountll(mask);
        if (K > POSE_FIELD_LIST - 64) {
            __builtin_amdgcn_wave_barrier();
            pose_field_flush(pv, dc, xy, bc, bi, lane, ls, K, n);
            __builtin_amdgcn_wave_barrier();
            K = 0;
        }
    }
}

__device__ __forceinline__ void pose_field_range(const RelaxView &xv, int b, int &lo, int &hi) {
    hi = min(xv.cell_start[b + 1], xv.j);
    lo = xv.cell_start[b];
    if (lo < 0 || lo > hi) lo = hi;
}

// One cell against all buckets, from the best (bc, bi) it comes with.  Uniform over the wavefront.
__device__ __forceinline__ void pose_field_cell(const PoseFieldView &pv, const DubCfg &dc, uint32_t xy, double &bc, uint32_t &bi, int lane, const PoseFieldLists &ls,
                                                PoseFieldCount &n) {
    const RelaxView &xv = pv.xv;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int cells = xv.ncx * xv.ncy, ncx = xv.ncx, ncy = xv.ncy, shift = xv.shift, edge = 1 << shift;
    const int gx = ux(xy), gy = uy(xy);
    int at = 0;
    int L = 0;  // survivors listed and not flushed yet: at most POSE_FIELD_LIST - 64
    const int cbx = gx >> shift, cby = gy >> shift;
    const bool near_first = bi == NONE;
    if (near_first) {
        // No bound yet: whatever the 3 x 3 buckets around the cell give bounds the scan, which leaves them out: every pair of theirs has
        // been screened, and evaluated and swept if need be, by then.
        for (int t = 0; t < 9; ++t) {
            const int bx = cbx + t / 3 - 1, by = cby + t % 3 - 1;
            if (bx < 0 || bx >= ncx || by < 0 || by >= ncy) continue;  // (uniform)
            int lo, hi;
            pose_field_range(xv, bx * ncy + by, lo, hi);
            ++n.buckets;
            pose_field_bucket(pv, dc, lo, hi, xy, bc, bi, lane, ls, L, n);
        }
        __builtin_amdgcn_wave_barrier();
        pose_field_flush(pv, dc, xy, bc, bi, lane, ls, L, n);
        L = 0;
        __builtin_amdgcn_wave_barrier();
    }
    for (;;) {
        int K = 0;
        while (at < cells) {
            const int b = at + lane;
            bool q = false;
            float lb = 0.0f;
            if (b < cells) {
                const unsigned long long bits = xv.cell_min[b];
                const int bx = b / ncy, by = b - bx * ncy;
                const bool done = near_first && bx >= cbx - 1 && bx <= cbx + 1 && by >= cby - 1 && by <= cby + 1;
                if (bits != ~0ull && !done) {  // (an empty bucket keeps the host's fill)
                    const int x0 = bx << shift, y0 = by << shift;
                    const int dx = max(max(x0 - gx, gx - (x0 + edge - 1)), 0), dy = max(max(y0 - gy, gy - (y0 + edge - 1)), 0);
                    const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);  // (coordinates below 2^12: below 2^25)
                    lb = chord_lower_bound(__longlong_as_double((long long)bits), d2);
                    q = (double)lb <= bc;
                }
            }
            const unsigned long long mask = __ballot(q);
            const int cnt = (int)__builtin_popcountll(mask);
            if (K + cnt > POSE_FIELD_BUCKETS) break;  // (uniform) the list is full: these buckets belong to the next chunk
            if (q) {
                const int pos = K + (int)__builtin_popcountll(mask & below);
                ls.bk[pos] = lb;
                ls.bb[pos] = (uint32_t)b;
            }
            K += cnt;
            at += 64;
        }
        __builtin_amdgcn_wave_barrier();
        double fk = -1.0;  // the last bucket taken: (fk, fb); every bound is >= 0
        uint32_t fb = 0;
        for (;;) {
            double mk = f64_inf();
            uint32_t mb = NONE;
            for (int t = lane; t < K; t += 64) {
                const double key = (double)ls.bk[t];
                const uint32_t b = ls.bb[t];
                if (key_lt(fk, fb, key, b) && key_lt(key, b, mk, mb)) {
                    mk = key;
                    mb = b;
                }
            }
            wave_min_f64_idx(mk, mb);
            if (mb == NONE || mb >= (uint32_t)cells || !(mk <= bc)) break;  // (the others of the list are no smaller)
            ++n.buckets;
            int lo, hi;
            pose_field_range(xv, (int)mb, lo, hi);
            pose_field_bucket(pv, dc, lo, hi, xy, bc, bi, lane, ls, L, n);
            fk = mk;
            fb = mb;
        }
        __builtin_amdgcn_wave_barrier();
        pose_field_flush(pv, dc, xy, bc, bi, lane, ls, L, n);  // what is left of the list: the best is final for these buckets
        L = 0;
        __builtin_amdgcn_wave_barrier();
        if (at >= cells) return;
    }
}

__global__ __launch_bounds__(POSE_FIELD_TPB) void rrt_pose_field_kernel(PoseFieldView pv) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    __shared__ double lc_lds[POSE_FIELD_TPB / 64][POSE_FIELD_LIST];
    __shared__ float bk_lds[POSE_FIELD_TPB / 64][POSE_FIELD_BUCKETS];
    __shared__ uint32_t bb_lds[POSE_FIELD_TPB / 64][POSE_FIELD_BUCKETS];
    __shared__ uint32_t lu_lds[POSE_FIELD_TPB / 64][POSE_FIELD_LIST];
    __shared__ uint32_t lp_lds[POSE_FIELD_TPB / 64][POSE_FIELD_LIST];
    __shared__ uint8_t lh_lds[POSE_FIELD_TPB / 64][POSE_FIELD_LIST];
    const int wave_ = ((int)threadIdx.x >> 6) & (POSE_FIELD_TPB / 64 - 1);  // the lists of this wavefront alone
    const PoseFieldLists ls{(volatile RRT_LDS float *)&bk_lds[wave_][0],    (volatile RRT_LDS uint32_t *)&bb_lds[wave_][0], (volatile RRT_LDS double *)&lc_lds[wave_][0],
                            (volatile RRT_LDS uint32_t *)&lu_lds[wave_][0], (volatile RRT_LDS uint32_t *)&lp_lds[wave_][0], (volatile RRT_LDS uint8_t *)&lh_lds[wave_][0]};
    const RelaxView &xv = pv.xv;
    const DubCfg dc = dub_cfg_fill<POSE_FIELD_TPB>((RRT_LDS double *)htab_s, pv.rho, pv.nh, pv.W, xv.H);
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = xv.j, H = xv.H, W = pv.W;
    const bool sane = pv.nh >= 1 && pv.nh <= 256 && pv.heading_lo >= 0 && pv.heading_lo < pv.heading_hi && pv.heading_hi <= pv.nh &&
                      j <= POSE_FIELD_MAX_J;  // (the host refuses the rest; uniform)
    const int run_cells = min(max(pv.run, 1), POSE_FIELD_RUN);
    const int runs_col = (pv.h + run_cells - 1) / run_cells;
    const int runs = pv.w * runs_col;
    for (int run = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); run < runs; run += (int)gridDim.x * waves) {  // (run is wave-uniform)
        const int cx = run / runs_col, x = pv.x0 + cx;
        const int y_first = (run - cx * runs_col) * run_cells;
        uint32_t prev = NONE;  // the key of the winner of the last cell of this run that had one
        PoseFieldCount n;      // of this run: at most POSE_FIELD_RUN cells of 2^18 vertices at 256 headings, which 32 bits hold
        for (int yy = y_first; yy < min(y_first + run_cells, pv.h); ++yy) {
            const int y = pv.y0 + yy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;  // (the host keeps the window inside the grid)
            const uint32_t xy = pack_xy(x, y);
            double bc = f64_inf();
            uint32_t bi = NONE;
            if (sane && xv.og[(uint32_t)x * (uint32_t)H + (uint32_t)y] == 0) {  // (an obstacle cell: every sweep ends on it, nothing connects)
                ++n.cells;
                if (prev != NONE) {
                    const uint32_t k = prev & ((1u << POSE_FIELD_VBITS) - 1u);
                    const int hg = (int)(prev >> POSE_FIELD_VBITS);
                    if (k < (uint32_t)j && hg >= pv.heading_lo && hg < pv.heading_hi) {
                        const uint32_t a = xv.nodes[k];
                        const int ha = (int)pv.heading[k];
                        if (ha < pv.nh && ux(a) < W && uy(a) < H) pose_field_try(pv, dc, k, a, ha, xv.vcost[k], xy, hg, bc, bi, lane, n);
                    }
                }
                if (j > 0) pose_field_cell(pv, dc, xy, bc, bi, lane, ls, n);
                if (bi != NONE) prev = bi;
            }
            if (lane == 0) {
                const size_t out = (size_t)cx * (size_t)pv.h + (size_t)yy;
                pv.vertex[out] = bi == NONE ? -1 : (int32_t)(bi & ((1u << POSE_FIELD_VBITS) - 1u));
                pv.cost[out] = bc;
                pv.heading_out[out] = bi == NONE ? -1 : (int32_t)(bi >> POSE_FIELD_VBITS);
            }
        }
        // the counters once per run, in 64 bits from there on: the walks are uniform, so lane 0's counts are the wavefront's; the words
        // are summed over the lanes
        const uint32_t words = wave_sum_u32(n.words);
        if (lane == 0) {
            if (n.cells) atomicAdd(&xv.stats[POSE_FIELD_CELLS], (unsigned long long)n.cells);
            if (n.buckets) atomicAdd(&xv.stats[POSE_FIELD_BUCKETS_SEEN], (unsigned long long)n.buckets);
            if (words) atomicAdd(&xv.stats[POSE_FIELD_WORDS], (unsigned long long)words);
            if (n.sweeps) atomicAdd(&xv.stats[POSE_FIELD_SWEEPS], (unsigned long long)n.sweeps);
        }
    }
}

}  // namespace rrtdev
