// rrt_routes.h -- finished routes to many goals over a finished tree, optionally shortened by line-of-sight shortcuts.
//
// rrt_goals_kernel (rrt_goals.h) answers which vertex a goal connects to.  These kernels turn that answer into polylines without
// leaving the device: per goal g with vertex[g] >= 0 the raw route is root = 0, ..., vertex[g] along the parent pointers, then the goal;
// k rows of (packed xy, id), the goal row with id -1.  vertex[g] == -1: no rows, length +inf.
//
//   1. rrt_route_depth_kernel   one goal per lane: walks the parents and counts, at most j steps.  A walk that is not at vertex 0 by
//                               then (a parent outside [0, j), a cycle) raises *err and counts 0 rows: nothing downstream walks it.
//   2. rrt_route_scan_kernel    exclusive scan of the counts into 64-bit row offsets, one workgroup.
//   3. rrt_route_fill_kernel    one goal per lane: walks again and writes its rows back to front; without shortcuts also the length.
//   4. rrt_route_cut_kernel     (shortcuts only) one workgroup per goal: greedy line-of-sight shortcutting, see cut_body.
//      ... and the scan again over the rows that were kept.
//   5. rrt_route_pack_kernel    one goal per wave: the kept rows to dense CSR rows (x, y as int32, id).
//
// Rows live in global memory (a route has up to j + 1 rows, far beyond LDS); the engine sizes it from the total the first scan gives.
// length[g] is the f64 sum, left to right from the root, of sqrt((double)d2) over the legs; d2 < 2^25 is exact in f64 and the root
// correctly rounded (sqrt_u32), so numpy gives the same bits.
// (The views, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_tree_dev.h"

namespace rrtdev {

// Greedy shortcutting of one route P[0..k) by the whole workgroup.  From the anchor a (row 0 first) the next row is the LARGEST
// b in (a, k-1] with b == a+1 or a free line P[a] -> P[b], walked from the start side (the walk is not symmetric).  Candidates go
// from the far end downwards in rounds of NW, one line per wave; the first round that holds a free line ends the anchor with its
// largest free b -- nothing nearer can be larger.  b == a+1 is never tested: a tree edge, or the goal edge go2goal tested.
// Emitted row e <= b goes to slot e of the same rows: slots below the anchor's successor are never read again, the anchor's point
// is held in a register, and slot e == b receives what it holds.
template <bool LARGE, int NW>
__device__ __forceinline__ void cut_body(const RoutesView &rv, RRT_LDS int *res /* [2][NW] */) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint8_t *og = rv.og;
    const int H = rv.H;
    int par = 0;  // which half of `res` the next round writes: a wave still reading round r cannot meet the writes of round r + 2,
                  // whose writers have passed the barrier of round r + 1
    for (int g = (int)blockIdx.x; g < rv.m; g += (int)gridDim.x) {
        const int k = rv.cnt[g];
        if (k == 0) {  // (uniform)
            if (t == 0) rv.kept[g] = 0;
            continue;
        }
        uint32_t *xy = rv.row_xy + rv.raw_off[g];
        int32_t *id = rv.row_id + rv.raw_off[g];
        int a = 0, e = 1;
        uint32_t pa = xy[0];
        double len = 0.0;
        while (a < k - 1) {
            int b = a + 1;
            for (int hi = k - 1; hi > a + 1; hi -= NW) {
                const int c = hi - wave;
                bool ok = false;
                if (c > a + 1) {  // (wave-uniform)
                    int cells;
                    const uint32_t pc = xy[c];
                    ok = LARGE ? los_wave_large(og, H, pa, pc, lane, cells) : los_wave(og, H, pa, pc, lane, cells);
                }
                if (lane == 0) res[par * NW + wave] = ok ? c : 0;
                __syncthreads();
                int best = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) best = max(best, res[par * NW + w]);
                par ^= 1;
                if (best) {
                    b = best;
                    break;
                }
            }
            const uint32_t pb = xy[b];
            if (t == 0) {
                const int32_t ib = id[b];
                xy[e] = pb;
                id[e] = ib;
                len += sqrt_u32(dist2(pa, pb));
            }
            ++e;
            a = b;
            pa = pb;
        }
        if (t == 0) {
            rv.kept[g] = e;
            rv.length[g] = len;
        }
    }
}

// one goal per lane: the rows of its raw route, 0 for a goal that nothing connects to
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_depth_kernel(RoutesView rv) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= rv.m) return;
    const int j = rv.j;
    int u = rv.vertex[g], rows = 0;
    if (u >= 0) {
        int steps = 0;
        while (u > 0 && u < j && steps < j) {
            u = rv.parent[u];
            ++steps;
        }
        if (u == 0) rows = steps + 2;  // the vertices root .. vertex[g], and the goal
        else atomicOr(rv.err, 1);
    }
    rv.cnt[g] = rows;
}

// exclusive scan of in[0, m) into out[0, m]: one workgroup of TPB threads, TPB values a pass (each at most j + 1 < 2^19: a pass sums
// below 2^32), the carry in 64 bits
__global__ __launch_bounds__(TPB) void rrt_route_scan_kernel(const int32_t *in, int64_t *out, int32_t m) {
    const int t = (int)threadIdx.x;
    int64_t carry = 0;
    int par = 0;
    for (int base = 0; base < m; base += TPB) {
        const int i = base + t;
        const uint32_t v = i < m ? (uint32_t)in[i] : 0u;
        const uint32_t incl = wave_incl_sum_u32(v);
        const WgScan s = wg_scan_step(incl, par);
        if (i < m) out[i] = carry + (int64_t)(s.before + incl - v);
        carry += (int64_t)s.total;
    }
    if (t == 0) out[m] = carry;
}

// one goal per lane: its rows, written from the goal back to the root; WITH_LEN (no shortcut pass follows): kept, and the length
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_fill_kernel(RoutesView rv, int32_t with_len) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= rv.m) return;
    const int k = rv.cnt[g];
    if (k == 0) {
        rv.kept[g] = 0;
        rv.length[g] = f64_inf();
        return;
    }
    uint32_t *xy = rv.row_xy + rv.raw_off[g];
    int32_t *id = rv.row_id + rv.raw_off[g];
    xy[k - 1] = rv.goals[g];
    id[k - 1] = -1;
    int u = rv.vertex[g];
    for (int i = k - 2; i >= 0; --i) {  // (k - 1 vertices, as the depth pass counted them: ends at vertex 0)
        xy[i] = rv.nodes[u];
        id[i] = u;
        if (i > 0) u = rv.parent[u];
    }
    if (with_len) {
        double len = 0.0;
        uint32_t pa = xy[0];
        for (int i = 1; i < k; ++i) {
            const uint32_t pb = xy[i];
            len += sqrt_u32(dist2(pa, pb));
            pa = pb;
        }
        rv.kept[g] = k;
        rv.length[g] = len;
    }
}

__global__ __launch_bounds__(TPB) void rrt_route_cut_kernel(RoutesView rv) {
    __shared__ int res[2 * NWAVE];
    cut_body<false, NWAVE>(rv, (RRT_LDS int *)res);
}

// grids up to 4096 x 4096 (a batch created with RRT_FLAG_LARGE_GRID): the lines of sight by los_wave_large
__global__ __launch_bounds__(TPB) void rrt_route_cut_large_kernel(RoutesView rv) {
    __shared__ int res[2 * NWAVE];
    cut_body<true, NWAVE>(rv, (RRT_LDS int *)res);
}

// one goal per wave: the first kept[g] rows of its raw rows to the dense rows fin_off[g] ...
__global__ __launch_bounds__(ROUTE_TPB) void rrt_route_pack_kernel(RoutesView rv) {
    const int lane = (int)threadIdx.x & 63;
    const int g = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (g >= rv.m) return;
    const int n = rv.kept[g];
    const uint32_t *xy = rv.row_xy + rv.raw_off[g];
    const int32_t *id = rv.row_id + rv.raw_off[g];
    const int64_t dst = rv.fin_off[g];
    for (int i = lane; i < n; i += 64) {
        const uint32_t p = xy[i];
        rv.out_xy[2 * (dst + i)] = ux(p);
        rv.out_xy[2 * (dst + i) + 1] = uy(p);
        rv.out_id[dst + i] = id[i];
    }
}

}  // namespace rrtdev
