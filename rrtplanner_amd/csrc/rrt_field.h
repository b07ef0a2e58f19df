// rrt_field.h -- the cost-to-come field of a finished straight-line tree: rrt_field_kernel and its form for grids up to 4096 x 4096.
//
// For every cell g of a window of the grid, what rrt_goals.h decides for the one goal g:
//
//   cost[k] = vcost[k] + sqrt(d2(k, g)) in f64 over the vertices k in [0, j); the answer is the smallest (cost, k) among the vertices whose
//   line k -> g is free -- the first in stable (cost, index) order that sees the goal is the minimum over those that see it.  A blocked
//   cell, or a free one that no vertex sees: vertex -1, cost +inf.
//
// The goals kernel sorts all j vertices for every goal.  A field has what a list of goals has not: the same vertices serve every cell,
// and neighbouring cells nearly always share their winner.  So the vertices are bucketed once per call and a cell looks only at the
// buckets whose lower bound can still beat what it has found:
//
//   1. buckets  rrt_relax.h's CSR over the dense input (rrt_relax_cell / scan / fill_kernel, launched by the host in front of this
//      kernel), by cell of edge 2^shift, with the cost of every item beside its point (item_cost) and the smallest vcost of every
//      bucket (cell_min).
//   2. rrt_field_kernel  one wavefront per cell.  A wavefront takes a run of FIELD_RUN consecutive cells of one column, runs grid-stride.
//      first    the winner of the cell before it in the run, priced and tested: if it sees this cell too, its (cost, k) is the bound
//               from the start -- and almost always the answer.
//      buckets  the lower bound of bucket b for cell g is lb = cell_min[b] + sqrt(d2min(g, square of b)).  cell_min <= vcost[k] and
//               d2min <= d2(k, g) for every k of b, and sqrt and the f64 sum are monotone, so lb <= cost[k] bit for bit.  The lanes
//               stream the buckets and list those with lb <= best (<=, not <: a vertex of equal cost and lower index still wins) in
//               the wavefront's LDS; the list is walked in ascending (lb, b) while lb <= best, which falls on the way.
//               (In front of the root a filter without one: lb <= best needs d2min <= (best - cell_min + slack)^2, see field_may_beat.)
//      inside   the lanes price the items of the bucket; those with (cost, k) < best join a list in the wavefront's LDS.  When the list is
//               full, and behind the last bucket, its entries are walked one line of sight per lane, a lane taking the next entry as soon
//               as its line is decided (field_flush): the smallest (cost, k) among the free ones becomes the best.  That is the minimum
//               the ascending walk stops at, without the order: on a cluttered map nearly every vertex cheaper than the winner is blocked
//               somewhere along its line, and each has to be shown blocked.
//      A bucket list that overflows is taken in chunks, each of what fits, in scan order; what a chunk finds tightens the bound for the
//      chunks behind it, so the result is the minimum over all of them whatever the order.
// The tree arrays are only read.  Every index is checked before it is used; what cannot be placed raises err (the bucket kernels) or is
// skipped.  No kernel waits for another workgroup.  stats: free cells decided, buckets visited, vertices priced, lines walked.
// (The views, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_device.h"

namespace rrtdev {

// b / ncy and b % ncy for 0 <= b < RELAX_MAX_CELLS without the integer division: the quotient of (b + 0.5) * (1 / ncy) in f32 is off by
// less than 2^-10 / ncy, the half keeps it 0.5 / ncy clear of the integers; the two steps behind it mend what a worse reciprocal leaves.
__device__ __forceinline__ void field_bucket_xy(int b, int ncy, float rcp_ncy, int &bx, int &by) {
    bx = (int)(((float)b + 0.5f) * rcp_ncy);
    by = b - bx * ncy;
    if (by < 0) {
        --bx;
        by += ncy;
    }
    if (by >= ncy) {
        ++bx;
        by -= ncy;
    }
}

// false only where cm + sqrt(d2) <= best cannot hold in f64.  With s = fl(sqrt(d2)) and fl(cm + s) <= best: cm + s <= best (1 + 2^-52), so
// s <= (best - cm) + best 2^-52 and, with the roundings of the difference and of the root, sqrt(d2) <= (t + best 2^-50) for t = fl(best - cm).
// The slack here is 1e-14 > 2^-47 of best and of the square: wider than all of them together.  cm > best never holds.  best = +inf: true.
__device__ __forceinline__ bool field_may_beat(double cm, uint32_t d2, double best) {
    const double t = best - cm, u = t + best * 1e-14;
    return !(t < 0.0) && !((double)d2 > u * u * (1.0 + 1e-14));
}

// The K listed candidates (lk, lu, lp: cost, vertex, point) against the cell xy, one line of sight per lane: the smallest (cost, k)
// among those that see the cell goes into the bound (bc, bi).
// A lane walks its own line a -> xy cell by cell, as collisionfree walks it, and leaves it at the first occupied cell; a lane without
// a line takes the next entry of the list, so the lanes stay busy while the list lasts and a long line holds up nobody but its own lane.
// The cell of step k is the closed form of include/rrt_line.h, (major: a + s k, minor: a + s floor((2 minor k + major) / (2 major))),
// taken forward in integers: the remainder starts at `major` and grows by 2 minor a step, at most one carry each since 2 minor <= 2 major
// -- exact on every grid, and three instructions a step instead of the closed form's eighteen.  Four cells a round, their loads in
// flight together.  Both ends lie inside the grid (checked here for the vertex, by the caller for the cell), so every cell of the walk does.
// All entries below the bound are walked whatever their order: the minimum over the free ones is what the ascending walk would have
// stopped at.  The bound is that of the call throughout: what the walk finds goes into it at the end.
// (A wavefront per line, los_wave, reads 64 cells of a line that is blocked at its fifth, and on a cluttered map nearly every candidate
// below the bound is such a line, thousands per cell: DESIGN.md 4.2c2 has the measurements that moved the field here.)
__device__ __forceinline__ void field_flush(const RelaxView &xv, int W, uint32_t xy, double &bc, uint32_t &bi, int lane, volatile RRT_LDS double *lk,
                                            volatile RRT_LDS uint32_t *lu, volatile RRT_LDS uint32_t *lp, int K, uint32_t &n_los) {
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint8_t *og = xv.og;
    const int H = xv.H, x1 = ux(xy), y1 = uy(xy);
    double fc = f64_inf(), c = f64_inf();  // the best free line of this lane so far; the entry it walks
    uint32_t fu = NONE, u = NONE;
    int off = 0, rem = 0, k = 0, major = 0, two_minor = 0, den = 0, smaj = 0, smin = 0;
    bool open = false;
    int next = 0;  // entries handed out (uniform)
    for (;;) {
        const unsigned long long idle = __ballot(!open);
        if (next < K && idle != 0) {  // (uniform) the idle lanes take the next entries, in lane order
            const int t = next + (int)__builtin_popcountll(idle & below);
            if (!open && t < K) {
                c = lk[t];
                u = lu[t];
                const uint32_t p = lp[t];
                const int x0 = ux(p), y0 = uy(p);
                const int dx = x1 - x0, dy = y1 - y0, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
                const bool xm = adx >= ady;
                const int stx = x0 < x1 ? H : -H, sty = y0 < y1 ? 1 : -1;  // (the steps of rrt_line_setup, as byte strides of the x-major grid)
                major = xm ? adx : ady;
                two_minor = 2 * (xm ? ady : adx);
                den = 2 * major;
                smaj = xm ? stx : sty;
                smin = xm ? sty : stx;
                off = x0 * H + y0;
                rem = major;
                k = 0;
                open = u < (uint32_t)xv.j && key_lt(c, u, bc, bi) && x0 < W && y0 < H;
            }
            next = min(K, next + (int)__builtin_popcountll(idle));
            n_los += (uint32_t)__builtin_popcountll(__ballot(open) & idle);
            continue;  // (lanes whose entry was no line to walk take another)
        }
        if (__ballot(open) == 0) break;  // (uniform: the list is handed out and no lane walks)
        int o[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            o[s] = off;
            off += smaj;
            rem += two_minor;
            if (rem >= den) {
                rem -= den;
                off += smin;
            }
        }
        uint8_t v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) v[s] = open && k + s <= major ? og[(uint32_t)o[s]] : (uint8_t)0;  // (past the last cell nothing is read)
        const bool blocked = (v[0] | v[1] | v[2] | v[3]) != 0;
        k += 4;
        if (open && (blocked || k > major)) {  // this lane's line is decided
            if (!blocked && key_lt(c, u, fc, fu)) {
                fc = c;
                fu = u;
            }
            open = false;
        }
    }
    wave_min_f64_idx(fc, fu);
    if (fu != NONE) {  // (below the bound: only such entries were walked)
        bc = fc;
        bi = fu;
    }
}

// The items [lo, hi) of one bucket for the cell xy: those with (cost, k) below the bound (bc, bi) join the list (K entries so far), which
// is walked as soon as another 64 might not fit.  Uniform over the wavefront.
__device__ __forceinline__ void field_bucket(const RelaxView &xv, int W, int lo, int hi, uint32_t xy, double &bc, uint32_t &bi, int lane,
                                             volatile RRT_LDS double *lk, volatile RRT_LDS uint32_t *lu, volatile RRT_LDS uint32_t *lp, int &K, uint32_t &n_los,
                                             uint32_t &n_priced) {
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int at = lo; at < hi; at += 64) {
        const int i = at + lane;
        int u = i < hi ? xv.items[i] : -1;
        if (u < 0 || u >= xv.j) u = -1;
        const uint32_t p = u >= 0 ? xv.item_xy[i] : 0u;
        const double c = u >= 0 ? xv.item_cost[i] : 0.0;
        const double cand = c + sqrt_u32(dist2(p, xy));
        const bool q = u >= 0 && key_lt(cand, (uint32_t)u, bc, bi);
        const unsigned long long mask = __ballot(q);
        n_priced += u >= 0 ? 1u : 0u;
        if (q) {  // (K <= FIELD_LIST - 64 here and at most 64 join)
            const int pos = K + (int)__builtin_popcountll(mask & below);
            lk[pos] = cand;
            lu[pos] = (uint32_t)u;
            lp[pos] = p;
        }
        K += (int)__builtin_popcountll(mask);
        if (K > FIELD_LIST - 64) {
            __builtin_amdgcn_wave_barrier();
            field_flush(xv, W, xy, bc, bi, lane, lk, lu, lp, K, n_los);
            __builtin_amdgcn_wave_barrier();
            K = 0;
        }
    }
}

// One cell against all buckets, from the bound (bc, bi) it comes with.  Uniform over the wavefront.
__device__ __forceinline__ void field_cell(const RelaxView &xv, int W, uint32_t xy, double &bc, uint32_t &bi, int lane, volatile RRT_LDS double *bk,
                                           volatile RRT_LDS uint32_t *bb, volatile RRT_LDS double *lk, volatile RRT_LDS uint32_t *lu, volatile RRT_LDS uint32_t *lp,
                                           uint32_t &n_buckets, uint32_t &n_los, uint32_t &n_priced) {
    const unsigned long long below = (1ull << lane) - 1ull;
    const int cells = xv.ncx * xv.ncy, ncy = xv.ncy, shift = xv.shift, edge = 1 << shift;
    const float rcp_ncy = 1.0f / (float)ncy;
    const int gx = ux(xy), gy = uy(xy);
    int at = 0;
    int L = 0;  // candidates listed and not walked yet: at most FIELD_LIST - 64
    if (bi == NONE) {
        // No bound yet (the first cell of a run, or the neighbour's winner does not see this one): the buckets are listed in scan order, so
        // the first chunk would be walked whole, far vertices and all.  The 3 x 3 buckets around the cell first: the winner is nearly
        // always there, and whatever they give bounds the scan.  The scan meets them again and lists only what is still below the bound.
        const int cbx = gx >> shift, cby = gy >> shift;
        for (int t = 0; t < 9; ++t) {
            const int bx = cbx + t / 3 - 1, by = cby + t % 3 - 1;
            if (bx < 0 || bx >= xv.ncx || by < 0 || by >= ncy) continue;  // (uniform)
            const int b = bx * ncy + by;
            const int hi = min(xv.cell_start[b + 1], xv.j);
            int lo = xv.cell_start[b];
            if (lo < 0) lo = hi;
            ++n_buckets;
            field_bucket(xv, W, lo, hi, xy, bc, bi, lane, lk, lu, lp, L, n_los, n_priced);
        }
        __builtin_amdgcn_wave_barrier();
        field_flush(xv, W, xy, bc, bi, lane, lk, lu, lp, L, n_los);
        L = 0;
        __builtin_amdgcn_wave_barrier();
    }
    for (;;) {
        int K = 0;
        while (at < cells) {
            const int b = at + lane;
            bool q = false;
            double lb = 0.0;
            if (b < cells) {
                const unsigned long long bits = xv.cell_min[b];
                if (bits != ~0ull) {  // (an empty bucket keeps the host's fill)
                    int bx, by;
                    field_bucket_xy(b, ncy, rcp_ncy, bx, by);
                    const int x0 = bx << shift, y0 = by << shift;
                    const int dx = max(max(x0 - gx, gx - (x0 + edge - 1)), 0), dy = max(max(y0 - gy, gy - (y0 + edge - 1)), 0);
                    const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);  // (coordinates below 2^12: below 2^25)
                    const double cm = __longlong_as_double((long long)bits);
                    if (field_may_beat(cm, d2, bc)) {
                        lb = cm + sqrt_u32(d2);
                        q = lb <= bc;
                    }
                }
            }
            const unsigned long long mask = __ballot(q);
            const int n = (int)__builtin_popcountll(mask);
            if (K + n > FIELD_BUCKETS) break;  // (uniform) the list is full: these buckets belong to the next chunk
            if (q) {
                const int pos = K + (int)__builtin_popcountll(mask & below);
                bk[pos] = lb;
                bb[pos] = (uint32_t)b;
            }
            K += n;
            at += 64;
        }
        __builtin_amdgcn_wave_barrier();
        double fk = -1.0;  // the last bucket taken: (fk, fb); every bound is >= 0
        uint32_t fb = 0;
        for (;;) {
            double mk = f64_inf();
            uint32_t mb = NONE;
            for (int t = lane; t < K; t += 64) {
                const double key = bk[t];
                const uint32_t b = bb[t];
                if (key_lt(fk, fb, key, b) && key_lt(key, b, mk, mb)) {
                    mk = key;
                    mb = b;
                }
            }
            wave_min_f64_idx(mk, mb);
            if (mb == NONE || mb >= (uint32_t)cells || !(mk <= bc)) break;  // (the others of the list are no smaller)
            ++n_buckets;
            const int hi = min(xv.cell_start[mb + 1], xv.j);
            int lo = xv.cell_start[mb];
            if (lo < 0) lo = hi;
            field_bucket(xv, W, lo, hi, xy, bc, bi, lane, lk, lu, lp, L, n_los, n_priced);
            fk = mk;
            fb = mb;
        }
        __builtin_amdgcn_wave_barrier();
        field_flush(xv, W, xy, bc, bi, lane, lk, lu, lp, L, n_los);  // what is left of the list: the bound is final for these buckets
        L = 0;
        __builtin_amdgcn_wave_barrier();
        if (at >= cells) return;
    }
}

template <bool LARGE>
__device__ __forceinline__ void field_body(const FieldView &fv, volatile RRT_LDS double *bk, volatile RRT_LDS uint32_t *bb, volatile RRT_LDS double *lk,
                                           volatile RRT_LDS uint32_t *lu, volatile RRT_LDS uint32_t *lp) {
    const RelaxView &xv = fv.xv;
    const int lane = (int)threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int j = xv.j, H = xv.H, W = fv.W;
    const int runs_col = (fv.h + FIELD_RUN - 1) / FIELD_RUN;
    const int runs = fv.w * runs_col;  // (at most 4096 columns of 256 runs)
    uint32_t n_cells = 0, n_buckets = 0, n_los = 0, n_priced = 0;
    for (int run = (int)blockIdx.x * waves + ((int)threadIdx.x >> 6); run < runs; run += (int)gridDim.x * waves) {  // (run is wave-uniform)
        const int cx = run / runs_col, x = fv.x0 + cx;
        const int y_first = (run - cx * runs_col) * FIELD_RUN;
        uint32_t prev = NONE;  // the winner of the last cell of this run that had one
        for (int yy = y_first; yy < min(y_first + FIELD_RUN, fv.h); ++yy) {
            const int y = fv.y0 + yy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;  // (the host keeps the window inside the grid)
            const uint32_t xy = pack_xy(x, y);
            double bc = f64_inf();
            uint32_t bi = NONE;
            if (xv.og[(uint32_t)x * (uint32_t)H + (uint32_t)y] == 0) {  // (an obstacle cell: every walk ends on it, no vertex sees it)
                ++n_cells;
                if (prev < (uint32_t)j) {
                    const uint32_t pxy = xv.nodes[prev];
                    int cells;
                    ++n_los;
                    n_priced += lane == 0 ? 1u : 0u;
                    if (LARGE ? los_wave_large(xv.og, H, pxy, xy, lane, cells) : los_wave(xv.og, H, pxy, xy, lane, cells)) {
                        bc = xv.vcost[prev] + sqrt_u32(dist2(pxy, xy));
                        bi = prev;
                    }
                }
                if (j > 0) field_cell(xv, W, xy, bc, bi, lane, bk, bb, lk, lu, lp, n_buckets, n_los, n_priced);
                if (bi != NONE) prev = bi;
            }
            if (lane == 0) {
                const size_t out = (size_t)cx * (size_t)fv.h + (size_t)yy;
                fv.vertex[out] = bi == NONE ? -1 : (int32_t)bi;
                fv.cost[out] = bc;
            }
        }
    }
    // the counters once per wavefront: the walks are uniform, so lane 0's counts are the wavefront's; the prices are summed over the lanes
    const uint32_t priced = wave_sum_u32(n_priced);
    if (lane == 0) {
        if (n_cells) atomicAdd(&xv.stats[FIELD_CELLS], (unsigned long long)n_cells);
        if (n_buckets) atomicAdd(&xv.stats[FIELD_BUCKETS_SEEN], (unsigned long long)n_buckets);
        if (priced) atomicAdd(&xv.stats[FIELD_PRICED], (unsigned long long)priced);
        if (n_los) atomicAdd(&xv.stats[FIELD_LOS], (unsigned long long)n_los);
    }
}

#define RRT_FIELD_LISTS                                                                                                                  \
    __shared__ double bk_lds[FIELD_TPB / 64][FIELD_BUCKETS];                                                                             \
    __shared__ uint32_t bb_lds[FIELD_TPB / 64][FIELD_BUCKETS];                                                                           \
    __shared__ double lk_lds[FIELD_TPB / 64][FIELD_LIST];                                                                                \
    __shared__ uint32_t lu_lds[FIELD_TPB / 64][FIELD_LIST];                                                                              \
    __shared__ uint32_t lp_lds[FIELD_TPB / 64][FIELD_LIST];                                                                              \
    const int wave_ = (int)(threadIdx.x >> 6) & (FIELD_TPB / 64 - 1); /* the lists of this wavefront alone */                            \
    volatile RRT_LDS double *bk = (volatile RRT_LDS double *)&bk_lds[wave_][0];                                                          \
    volatile RRT_LDS uint32_t *bb = (volatile RRT_LDS uint32_t *)&bb_lds[wave_][0];                                                      \
    volatile RRT_LDS double *lk = (volatile RRT_LDS double *)&lk_lds[wave_][0];                                                          \
    volatile RRT_LDS uint32_t *lu = (volatile RRT_LDS uint32_t *)&lu_lds[wave_][0];                                                      \
    volatile RRT_LDS uint32_t *lp = (volatile RRT_LDS uint32_t *)&lp_lds[wave_][0]

__global__ __launch_bounds__(FIELD_TPB) void rrt_field_kernel(FieldView fv) {
    RRT_FIELD_LISTS;
    field_body<false>(fv, bk, bb, lk, lu, lp);
}

// grids up to 4096 x 4096 (a batch created with RRT_FLAG_LARGE_GRID): the lines of sight by los_wave_large
__global__ __launch_bounds__(FIELD_TPB) void rrt_field_large_kernel(FieldView fv) {
    RRT_FIELD_LISTS;
    field_body<true>(fv, bk, bb, lk, lu, lp);
}
#undef RRT_FIELD_LISTS

}  // namespace rrtdev
