// rrt_pose_goals.h -- connect many goal POSES to a finished Dubins tree: rrt_pose_goals_kernel.
//
// rrt_goals.h serves the straight-line planners; a Dubins goal is a pose (x, y, h) and its edge a Dubins word, so the decision is
// go2goal_phase<DUB = true>'s (rrt_go2goal.h), the one plan() takes for its own goal pose, taken for M poses against the tree a
// finished query left on the device:
//
//   c[k] = vcost[k] + dub_between(pose_k, goal).len for the vertices k in [0, j), tried in stable (c, k) order; the first vertex
//   whose sweep is free (every sample k * DUB_DS inside the grid and on a free cell, the goal cell free) wins.  Nothing connects, or
//   the goal on an obstacle cell: vertex -1, cost +inf.  plan()'s fall-backs (vgoal = 0, the IndexError) are not reproduced.
//
// Equivalently: the (c, k)-minimum over the vertices with a free sweep -- which is what lets this kernel skip work.  go2goal_phase
// evaluates a word three times per vertex (range, histogram, scatter) before any sweep; a word is some 2000 instructions.  Here:
//
//   - the vertices are counting-sorted by chord_lower_bound(vcost[k], d2(k, goal)) (rrt_cell_stream.h), a float that is <= c[k] -- a
//     word is never shorter than its chord -- into the same G2G_NB buckets: the three passes are a few operations per vertex;
//   - the order is walked in rounds of one vertex per lane: every lane evaluates its word ONCE; each wave then sweeps, cheapest key
//     first, its lanes whose (c, k) is below the best passing key so far, and stops at its first free sweep; the waves exchange
//     their best key once per round;
//   - the walk ends at bend[bucket(best cost)]: a vertex behind that position has a bound in a later bucket than the best cost,
//     so bound > best cost (the bucket function is monotone and the same for bounds and costs), and c >= bound.  A vertex whose
//     bound EQUALS the best cost shares its bucket and stays inside.
//
// A vertex is left unevaluated only through that bound and unswept only because its key is not below a passing key, so the
// answers are go2goal_phase<true>'s bit for bit: the words are dub_between_dev's with the same DubCfg (heading table, rho, 1 / rho).
//
// One workgroup of TPB threads decides one goal pose at a time, goals g = blockIdx.x, blockIdx.x + gridDim.x, ...; `order` is this
// workgroup's slab.  Thread 0 writes, per goal, the words evaluated and the sweeps run (rrt_batch_connect_poses_counts).
// (The exhaustive form -- goals_body with go2goal_phase<true> -- was the correctness anchor and the other side of the measurement: the
// same answers at 313.4 ms against 160.6 ms per 4096 goal poses at bench scale.  profiles/poses_wall.json has both numbers,
// tools/archive/poses_exhaustive.patch the code.)
// (The view, the launch constants and the kernel's declaration: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_go2goal.h"
#include "rrt_cell_stream.h"

namespace rrtdev {

// The decision for one goal pose; pc / pi = +inf / NONE when nothing connects.  words / sweeps: what it evaluated (uniform).
__device__ __forceinline__ void pose_goal_bounded(const PoseGoalsView &pv, const DubCfg &dc, uint32_t xg, int hg, uint32_t *order, RRT_LDS uint32_t *lds16k,
                                                  BSlot *bslots, int t, int lane, int wave, double &pc, uint32_t &pi, uint32_t &words, uint32_t &sweeps) {
    RRT_LDS uint32_t *cursor = lds16k;         // [G2G_NB]
    RRT_LDS uint32_t *bend = lds16k + G2G_NB;  // [G2G_NB]
    const uint8_t *og = pv.og;
    const uint32_t *nodes = pv.nodes;
    const double *vcost = pv.vcost;
    const uint8_t *heading = pv.heading;
    const int cnt = pv.j;
    auto bound_of = [&](int k) -> float { return chord_lower_bound(vcost[k], dist2(nodes[k], xg)); };
    // ---- range of the bounds ----
    float lmin = __builtin_inff(), lmax = 0.0f;
    for (int k = t; k < cnt; k += TPB) {
        const float lb = bound_of(k);
        lmin = lb < lmin ? lb : lmin;
        lmax = lb > lmax ? lb : lmax;
    }
    lmin = wave_min_f32_nonneg(lmin);
    lmax = __uint_as_float(~wave_min_u32(~__float_as_uint(lmax)));  // (non-negative floats order like their bit patterns)
    if (lane == 0) {
        bslots[wave].pc = (double)lmin;
        bslots[wave].uc = (double)lmax;
    }
    __syncthreads();
    double bmin = f64_inf(), bmax = 0.0;
    for (int w = 0; w < NWAVE; ++w) {
        const double x = bslots[w].pc, y = bslots[w].uc;
        bmin = x < bmin ? x : bmin;
        bmax = y > bmax ? y : bmax;
    }
    __syncthreads();
    // ONE bucket function for bounds and costs, monotone non-decreasing in its f64 argument (a subtraction of one constant, a
    // product with one non-negative constant, a truncation); arguments are >= bmin, costs may lie beyond bmax
    const double scale = (bmax > bmin) ? (double)(G2G_NB - 1) / (bmax - bmin) : 0.0;
    auto bucket_of = [&](double c) -> uint32_t {
        const double f = (c - bmin) * scale;
        return f >= (double)(G2G_NB - 1) ? (uint32_t)(G2G_NB - 1) : (uint32_t)f;
    };
    // ---- histogram, exclusive scan, scatter (as go2goal_phase) ----
    for (int b = t; b < 2 * G2G_NB; b += TPB) lds16k[b] = 0;
    __syncthreads();
    for (int k = t; k < cnt; k += TPB) __hip_atomic_fetch_add(&cursor[bucket_of((double)bound_of(k))], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    {
        constexpr int PB = G2G_NB / TPB;  // thread t owns the PB consecutive buckets PB t .. PB t + PB - 1
        static_assert(PB * TPB == G2G_NB, "buckets per thread");
        uint32_t cb[PB], own = 0;
#pragma unroll
        for (int e = 0; e < PB; ++e) {
            cb[e] = cursor[PB * t + e];
            own += cb[e];
        }
        uint32_t incl = own;
        incl = wave_incl_sum_u32(incl);
        if (lane == 63) bslots[wave].pi = incl;  // wave total
        __syncthreads();
        uint32_t base = 0;
        for (int w = 0; w < wave; ++w) base += bslots[w].pi;
        uint32_t ex = base + incl - own;
#pragma unroll
        for (int e = 0; e < PB; ++e) {
            cursor[PB * t + e] = ex;
            ex += cb[e];
            bend[PB * t + e] = ex;
        }
        __syncthreads();
    }
    for (int k = t; k < cnt; k += TPB) {
        const uint32_t pos = __hip_atomic_fetch_add(&cursor[bucket_of((double)bound_of(k))], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        order[pos] = (uint32_t)k;  // (pos < cnt <= slab_words: the bucket ends sum to cnt)
    }
    __syncthreads();
    // ---- walk the order: one vertex per lane and round; lane l of wave w takes position pos0 + l * NWAVE + w, so that every wave
    // holds an even share of the round's cheap end ----
    pc = f64_inf();
    pi = NONE;
    words = 0;
    sweeps = 0;
    uint32_t limit = (uint32_t)cnt;
    int round = 0;
    for (uint32_t pos0 = 0; pos0 < limit; pos0 += TPB) {
        const uint32_t p = pos0 + (uint32_t)(lane * NWAVE + wave);
        uint32_t k = NONE, nk = 0;
        int hk = 0;
        double c = f64_inf();
        dub_path_t pth = dub_no_path();
        if (p < limit) {
            k = order[p];
            nk = nodes[k];
            hk = (int)heading[k];
            pth = dub_between_dev(nk, hk, xg, hg, dc);
            c = vcost[k] + pth.len;
        }
        words += (limit - pos0 < (uint32_t)TPB) ? limit - pos0 : (uint32_t)TPB;
        // this wave's candidates, cheapest first, until one passes (the cheapest passing one of the wave: nothing after it can beat it)
        bool pend = k != NONE && key_lt(c, k, pc, pi);
        double bc = f64_inf();
        uint32_t bi = NONE, nsw = 0;
        for (;;) {
            double mc = pend ? c : f64_inf();
            uint32_t mi = pend ? k : NONE;
            wave_min_f64_idx(mc, mi);
            if (mi == NONE) break;
            const int l = (int)__builtin_ctzll(__ballot(pend && k == mi));  // (a vertex sits in one lane)
            const dub_path_t wp = dub_path_from_lane(pth, l);
            const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)nk, l);
            const int ha = __builtin_amdgcn_readlane(hk, l);
            int cc = 0;
            const bool ok = dub_sweep_wave(og, dc, a, ha, xg, wp, lane, cc);
            ++nsw;
            if (lane == l) pend = false;
            if (ok) {
                bc = mc;
                bi = mi;
                break;
            }
        }
        BSlot *sl = bslots + (round & 1) * NWAVE;
        if (lane == 0) {
            sl[wave].pc = bc;
            sl[wave].pi = bi;
            sl[wave].cells = nsw;
        }
        __syncthreads();
        double rc = f64_inf();
        uint32_t ri = NONE, rs = 0;
        if (lane < NWAVE) {
            rc = sl[lane].pc;
            ri = sl[lane].pi;
            rs = sl[lane].cells;
        }
        wave_min_f64_idx(rc, ri);
        sweeps += wave_sum_u32(rs);
        ++round;
        if (key_lt(rc, ri, pc, pi)) {
            pc = rc;
            pi = ri;
            const uint32_t e = bend[bucket_of(pc)];  // every vertex whose bound is <= pc lies before this position
            limit = e < limit ? e : limit;
        }
    }
}

__device__ __forceinline__ void pose_goals_body(const PoseGoalsView &pv, RRT_LDS uint32_t *lds16k, BSlot *bslots, RRT_LDS double *htab) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const DubCfg dc = dub_cfg_fill<TPB>(htab, pv.rho, pv.nh, pv.W, pv.H);
    __syncthreads();
    uint32_t *order = pv.order + (size_t)blockIdx.x * (size_t)pv.slab_words;
    for (int g = (int)blockIdx.x; g < pv.m; g += (int)gridDim.x) {
        const uint32_t xg = pv.goals[g];
        const int hg = (int)pv.goal_h[g];
        double pc = f64_inf();
        uint32_t pi = NONE, words = 0, sweeps = 0;
        // a goal on an obstacle cell: every sweep ends on it, so no vertex connects (uniform branch: the barriers inside are safe)
        if (pv.j > 0 && pv.og[(uint32_t)ux(xg) * (uint32_t)pv.H + (uint32_t)uy(xg)] == 0) {
            pose_goal_bounded(pv, dc, xg, hg, order, lds16k, bslots, t, lane, wave, pc, pi, words, sweeps);
        }
        if (t == 0) {
            pv.vertex[g] = pi == NONE ? -1 : (int32_t)pi;
            pv.cost[g] = pc;
            pv.counts[2 * g] = words;
            pv.counts[2 * g + 1] = sweeps;
        }
        __syncthreads();  // the next goal rewrites the slots and tables that slower waves may still be reading
    }
}

__global__ __launch_bounds__(TPB) void rrt_pose_goals_kernel(PoseGoalsView pv) {
    __shared__ __attribute__((aligned(16))) uint32_t lds16k[2 * G2G_NB];
    __shared__ __attribute__((aligned(16))) BSlot bslots[2 * NWAVE];
    __shared__ __attribute__((aligned(16))) double htab[3 * 256];
    pose_goals_body(pv, (RRT_LDS uint32_t *)lds16k, bslots, (RRT_LDS double *)htab);
}

}  // namespace rrtdev
