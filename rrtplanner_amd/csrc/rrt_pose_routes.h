// rrt_pose_routes.h -- finished routes to many goal POSES over a finished Dubins tree, and the path the vehicle drives along them.
//
// rrt_pose_goals_kernel (rrt_pose_goals.h) answers which vertex a goal pose connects to.  These kernels turn that answer into routes
// without leaving the device, as rrt_routes.h does for the straight-line planners: per goal g with vertex[g] >= 0 the route is
// root = 0, ..., vertex[g] along the parent pointers, then the goal pose; k rows of (packed xy, heading byte, id), the goal row with
// id -1.  vertex[g] == -1: no rows, length +inf, no points.  Without shortcuts (rrt_batch_pose_routes) the rows are written straight
// into their final place and nothing is packed afterwards; with them (rrt_batch_pose_shortcuts) steps 2a - 2c come between 2 and 3.
//
//   1. rrt_route_depth_kernel, rrt_route_scan_kernel (rrt_routes.h, as they are): rows per goal, and their 64-bit offsets.
//   2. rrt_pose_route_fill_kernel    one goal per lane: walks the parents and writes its rows back to front.
//  2a. rrt_pose_route_cut_kernel     (shortcuts only) ONE WAVEFRONT PER GOAL, grid-stride: the greedy pass over the raw route P[0..k).
//                                    A shortcut from a pose of the route to a later one keeps both poses and replaces the legs between
//                                    them by the shortest word from the first to the second: the words change, the poses do not.  From
//                                    the anchor a (row 0 first) the next kept row is the LARGEST b in (a, k-1] with b == a + 1 -- never
//                                    tested: a tree edge that holds on the active grid, or the goal edge the decision swept -- or a free
//                                    sweep (dub_sweep_wave on the active grid) of dub_between_dev(P[a], P[b]) from P[a].  Candidates go
//                                    from the far end downwards in batches of 64: lane l evaluates the word to candidate hi - l once
//                                    (the 64-words-at-a-time form of rrt_pose_keep_edge_kernel), then the wavefront sweeps the batch
//                                    from the farthest candidate down, the word handed over by readlane, and stops at the first free
//                                    one: nothing nearer can be larger.  A word that is DUB_NONE, not finite or beyond
//                                    POSE_ROUTE_LEG_POINTS samples (none can be: dub_shortest tries six words) is not free and raises
//                                    nothing.  Kept row e <= b goes to slot e of the same rows: slots at or below a + 1 are never read
//                                    again (the candidates of the next anchor b are above b + 1 > e), the anchor's pose is held in
//                                    registers, and slot e == b receives what it holds.  kept[g] = e at the end, 0 without rows.  The
//                                    heading table is dub_cfg_fill's; behind its barrier there is none: routes differ in length
//                                    and no wavefront waits for another.
//  2b. rrt_route_scan_kernel again   (shortcuts only) over kept: the 64-bit offsets of the kept rows.
//  2c. rrt_pose_route_pack_kernel    (shortcuts only) one goal per wavefront: its kept rows to the dense rows that steps 3 - 6 read as
//                                    they read the rows of step 2.  The words and lengths of the kept legs are step 3's: one definition.
//   3. rrt_pose_route_leg_kernel     one ROW per lane, grid-stride.  A row with id -1 is the last of its route: leg length 0, one point
//                                    (the goal cell).  Any other row r evaluates dub_between_dev(row r, row r + 1) once, with the heading
//                                    table in LDS that dub_cfg_fill (rrt_dubins_dev.h) builds: the words are the planner's bits.  With
//                                    points it also runs the sweep set-up once (dub_sweep_setup_sc with the table's sine / cosine) and
//                                    stores the leg's dub_sweep_t and its nsamples = floor(len / DUB_DS) + 1.  DUB_NONE, a length that
//                                    is not finite or more than POSE_ROUTE_LEG_POINTS samples cannot happen on a valid tree (every
//                                    sample of an accepted word lies inside a grid of at most 2048 x 2048 cells: a word is shorter than
//                                    three full circles that fit in it, some 27 000 cells): *err is raised, the leg counts no points.
//   4. rrt_route_scan_kernel again   (points only) over the rows' point counts: the 64-bit point offset of every row.
//   5. rrt_pose_route_length_kernel  one goal per lane: length[g] = the f64 sum of its legs' lengths, left to right from 0.0.  The
//                                    Dubins loop sets vcost[child] = vcost[parent] + len and never rewires, and rrt_pose_goals_kernel
//                                    prices vcost[v] + len: without shortcuts this sum IS cost[g], bit for bit (with them it is at most
//                                    cost[g], up to rounding).  The order is the semantics: no fold.
//                                    Also the goal's point offset, which is that of its first row.
//   6. rrt_pose_route_points_kernel  (points only) ONE POINT PER LANE, grid-stride over all points of the call.  Tree legs are short (at
//                                    most r_rewire cells, a few dozen samples): a wavefront per leg would idle most of its lanes
//                                    (rrt_pose_keep.h notes the same of its sweep).  A lane finds its row by a binary search of the row
//                                    point offsets, loads that leg's dub_sweep_t -- neighbouring lanes mostly share it -- evaluates
//                                    dub_sweep_point (include/rrt_dubins_points.h: dub_sweep_cell before it floors, one series) and
//                                    stores (x, y) as one 16-byte store.  The point of a goal row is the goal cell as doubles.
//
// The points of a leg are the samples k * DUB_DS, k = 0 .. nsamples - 1, of its word: the very samples whose cells plan(),
// rrt_pose_goals_kernel and rrt_pose_keep_edge_kernel tested.  Sample 0 is the leg's start pose exactly; the end pose is the next
// leg's sample 0 and is not repeated -- except on a leg whose length is an exact multiple of DUB_DS, whose last sample IS its end
// pose: that point appears twice, and nothing here special-cases it.
// (The view, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_dubins_dev.h"
#include "rrt_dubins_points.h"

namespace rrtdev {

static_assert(sizeof(dub_sweep_t) == POSE_ROUTE_SWEEP_BYTES, "the host sizes the legs' sweeps by POSE_ROUTE_SWEEP_BYTES");

// one goal per lane: its rows, written from the goal pose back to the root
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_fill_kernel(PoseRoutesView pr) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= pr.m) return;
    const int k = pr.cnt[g];
    if (k == 0) return;
    const int64_t at = pr.raw_off[g];
    uint32_t *xy = pr.row_xy + at;
    uint8_t *hd = pr.row_h + at;
    int32_t *id = pr.row_id + at;
    xy[k - 1] = pr.goals[g];
    hd[k - 1] = pr.goal_h[g];
    id[k - 1] = -1;
    int u = pr.vertex[g];
    for (int i = k - 2; i >= 0; --i) {  // (k - 1 vertices, as the depth pass counted them: ends at vertex 0)
        xy[i] = pr.nodes[u];
        hd[i] = pr.heading[u];
        id[i] = u;
        if (i > 0) u = pr.parent[u];
    }
}

// one wavefront per goal: the greedy shortcut pass over its raw rows, the kept rows compacted to their front
__global__ __launch_bounds__(POSE_CUT_TPB) void rrt_pose_route_cut_kernel(PoseCutView pc) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    RRT_LDS double *htab = (RRT_LDS double *)htab_s;
    const int t = (int)threadIdx.x, lane = t & 63;
    const DubCfg dc = dub_cfg_fill<POSE_CUT_TPB>(htab, pc.rho, pc.nh, pc.W, pc.H);
    __syncthreads();  // the only barrier: from here on every wavefront is on its own
    const uint8_t *og = pc.og;
    const int waves = POSE_CUT_TPB / 64;
    for (int g = (int)blockIdx.x * waves + (t >> 6); g < pc.m; g += (int)gridDim.x * waves) {  // (g is wave-uniform)
        const int k = pc.cnt[g];
        if (k == 0) {
            if (lane == 0) pc.kept[g] = 0;
            continue;
        }
        const int64_t at = pc.raw_off[g];
        uint32_t *xy = pc.row_xy + at;
        uint8_t *hd = pc.row_h + at;
        int32_t *id = pc.row_id + at;
        int a = 0, e = 1;
        uint32_t pa = (uint32_t)__builtin_amdgcn_readfirstlane((int)xy[0]);
        int ha = __builtin_amdgcn_readfirstlane((int)hd[0]);
        while (a < k - 1) {
            int b = a + 1;
            for (int hi = k - 1; hi > a + 1 && b == a + 1; hi -= 64) {
                const int c = hi - lane;  // this lane's candidate: its word, once
                uint32_t pcell = 0;
                dub_path_t pth = dub_no_path();
                if (c > a + 1) {
                    pcell = xy[c];
                    pth = dub_between_dev(pa, ha, pcell, (int)hd[c], dc);
                    // (the comparison is false for a NaN, too)
                    if (!(pth.len >= 0.0 && pth.len < (double)POSE_ROUTE_LEG_POINTS * DUB_DS)) pth.word = DUB_NONE;
                }
                const int cnt = hi - (a + 1) < 64 ? hi - (a + 1) : 64;
                for (int l = 0; l < cnt; ++l) {  // (l is wave-uniform) the farthest candidate first
                    const dub_path_t wp = dub_path_from_lane(pth, l);
                    if (wp.word == DUB_NONE) continue;
                    const uint32_t pb = (uint32_t)__builtin_amdgcn_readlane((int)pcell, l);
                    int cc = 0;
                    if (dub_sweep_wave(og, dc, pa, ha, pb, wp, lane, cc)) {
                        b = hi - l;
                        break;
                    }
                }
            }
            const uint32_t pb = (uint32_t)__builtin_amdgcn_readfirstlane((int)xy[b]);
            const int hb = __builtin_amdgcn_readfirstlane((int)hd[b]);
            const int32_t ib = id[b];
            if (lane == 0) {  // (e <= b: slot e is never read again, or holds this row already)
                xy[e] = pb;
                hd[e] = (uint8_t)hb;
                id[e] = ib;
            }
            ++e;
            a = b;
            pa = pb;
            ha = hb;
        }
        if (lane == 0) pc.kept[g] = e;
    }
}

// one goal per wavefront: the first kept[g] rows of its raw rows to the dense rows fin_off[g] ...
__global__ __launch_bounds__(POSE_CUT_TPB) void rrt_pose_route_pack_kernel(PoseCutView pc) {
    const int lane = (int)threadIdx.x & 63;
    const int g = (int)(blockIdx.x * (POSE_CUT_TPB / 64) + (threadIdx.x >> 6));
    if (g >= pc.m) return;
    const int n = pc.kept[g];
    const int64_t src = pc.raw_off[g], dst = pc.fin_off[g];
    for (int i = lane; i < n; i += 64) {
        pc.out_xy[dst + i] = pc.row_xy[src + i];
        pc.out_h[dst + i] = pc.row_h[src + i];
        pc.out_id[dst + i] = pc.row_id[src + i];
    }
}

// one row per lane: the word from it to the next row of its route, its length, and with points its sweep and its samples
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_leg_kernel(PoseRoutesView pr) {
    __shared__ __attribute__((aligned(16))) double htab_s[3 * 256];
    RRT_LDS double *htab = (RRT_LDS double *)htab_s;
    const int t = (int)threadIdx.x;
    const DubCfg dc = dub_cfg_fill<POSE_ROUTE_TPB>(htab, pr.rho, pr.nh, pr.W, pr.H);
    __syncthreads();
    dub_sweep_t *sweep = static_cast<dub_sweep_t *>(pr.sweep_bytes);
    const int64_t rows = pr.rows, stride = (int64_t)gridDim.x * POSE_ROUTE_TPB;
    for (int64_t r = (int64_t)blockIdx.x * POSE_ROUTE_TPB + t; r < rows; r += stride) {
        double len = 0.0;
        int32_t np = 1;  // a goal row: the goal cell
        if (pr.row_id[r] != -1 && r + 1 < rows) {
            const uint32_t a = pr.row_xy[r], b = pr.row_xy[r + 1];
            const int ha = (int)pr.row_h[r], hb = (int)pr.row_h[r + 1];
            const dub_path_t pth = dub_between_dev(a, ha, b, hb, dc);
            len = pth.len;
            // (the comparison is false for a NaN, too)
            if (pth.word == DUB_NONE || !(len >= 0.0 && len < (double)POSE_ROUTE_LEG_POINTS * DUB_DS)) {
                atomicOr(pr.err, 2);
                np = 0;
            } else if (sweep) {
                const dub_sweep_t s = dub_sweep_setup_sc((double)ux(a), (double)uy(a), htab[ha], htab[256 + ha], htab[512 + ha], &pth, pr.rho);
                sweep[r] = s;
                np = s.nsamples;
            }
        }
        pr.leg_len[r] = len;
        if (pr.npts) pr.npts[r] = np;
    }
}

// one goal per lane: the sequential sum of its legs, and where its points begin
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_length_kernel(PoseRoutesView pr) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g > pr.m) return;
    if (pr.goal_pt_off) pr.goal_pt_off[g] = pr.pt_off[g < pr.m ? pr.raw_off[g] : pr.rows];  // (lane m: the end of the last route)
    if (g == pr.m) return;
    const int k = pr.cnt[g];
    if (k == 0) {
        pr.length[g] = f64_inf();
        return;
    }
    const double *leg = pr.leg_len + pr.raw_off[g];
    double len = 0.0;
    for (int i = 0; i < k - 1; ++i) len += leg[i];
    pr.length[g] = len;
}

// one point per lane
__global__ __launch_bounds__(POSE_ROUTE_TPB) void rrt_pose_route_points_kernel(PoseRoutesView pr) {
    const int64_t n = pr.npoints, rows = pr.rows, stride = (int64_t)gridDim.x * POSE_ROUTE_TPB;
    const int64_t *off = pr.pt_off;
    const dub_sweep_t *sweep = static_cast<const dub_sweep_t *>(pr.sweep_bytes);
    for (int64_t i = (int64_t)blockIdx.x * POSE_ROUTE_TPB + (int64_t)threadIdx.x; i < n; i += stride) {
        // the last row r of [0, rows) with off[r] <= i: off[0] == 0 <= i < n == off[rows], and a row without points (a leg that
        // raised err) shares its offset with the next one, which the search passes over
        int64_t lo = 0, hi = rows;
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (off[mid] <= i) lo = mid;
            else hi = mid;
        }
        const uint32_t c = pr.row_xy[lo];
        double px = (double)ux(c), py = (double)uy(c);  // a goal row: the goal cell
        if (pr.row_id[lo] != -1) dub_sweep_point(sweep + lo, (int32_t)(i - off[lo]), &px, &py);
        pr.points[i] = make_double2(px, py);
    }
}

}  // namespace rrtdev
