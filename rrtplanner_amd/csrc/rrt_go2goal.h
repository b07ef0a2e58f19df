// rrt_go2goal.h -- the goal phase that every expansion kernel ends with and that the goals kernels (rrt_goals.h, rrt_pose_goals.h)
// run for many goals: go2goal_phase, and the slots its waves exchange.
#pragma once

#include "rrt_device.h"
#include "rrt_dubins_dev.h"

namespace rrtdev {

// Workgroup exchange for the (rare) extra branch-and-bound rounds.
struct BSlot {
    double pc, uc;  // passing key of this round (or inf), best still-untested key (or inf)
    uint32_t pi, ui;
    uint32_t cells, tested;
};

// ---------------------------------------------------------------------------------------------------------------
// go2goal (rrt.py:311-332): the goal connects to the first node, in stable (cost, index) order of
// cost = vcost[k] + dist(k, goal), that has line of sight to it.  Nodes are counting-sorted into G2G_NB cost buckets
// (LDS histogram, monotone bucket function), then tested in bucket order, 16 waves x G2G_U nodes per round; the
// search ends once every node of the bucket that holds the cheapest passing node has been tested.
constexpr int G2G_NB = 2048;  // cost buckets (2 x 8 KiB of LDS: fill cursors and bucket ends)
constexpr int G2G_U = 4;      // nodes a wave tests per round

// The nodes considered are kfirst + m * kstep, m < cnt (all of them: 0, 1, j; a team gives each member a stripe and takes the
// minimum of the stripes' answers).
// NT: threads of the calling workgroup (a pipelined team's committer may run as a workgroup of its own with fewer waves).
// LARGE: grids up to 4096 x 4096 (the lines of sight by los_wave_large; the costs are sqrt_u32's, exact for any radicand).
template <bool DUB = false, int NT = TPB, bool LARGE = false>
__device__ __forceinline__ void go2goal_phase(const uint8_t *og, int H, const uint32_t *nodes_g, const double *vcost, int kfirst, int kstep,
                                              int cnt, uint32_t xg, uint32_t *order, RRT_LDS uint32_t *lds16k, BSlot *bslots, int t, int lane,
                                              int wave, double &pc, uint32_t &pi, const uint8_t *heading = nullptr, int hg = 0, DubCfg dc = DubCfg{}) {
    RRT_LDS uint32_t *cursor = lds16k;          // [G2G_NB]
    RRT_LDS uint32_t *bend = lds16k + G2G_NB;   // [G2G_NB]
    auto cost_of = [&](int k) -> double {  // rrt.py:313-314
        if (DUB) return vcost[k] + dub_between_dev(nodes_g[k], heading[k], xg, hg, dc).len;
        return vcost[k] + sqrt_u32(dist2(nodes_g[k], xg));
    };
    // ---- cost range ----
    double cmin = f64_inf(), cmax = 0.0;
    for (int m = t; m < cnt; m += NT) {
        const double c = cost_of(kfirst + m * kstep);
        cmin = c < cmin ? c : cmin;
        cmax = c > cmax ? c : cmax;
    }
    {
        uint32_t dummy = 0;
        wave_min_f64_idx(cmin, dummy);
        // max of non-negative doubles == max of their bit patterns; reduce as min of the complement
        unsigned long long mb = ~(unsigned long long)__double_as_longlong(cmax);
        uint32_t hi = (uint32_t)(mb >> 32), lo = (uint32_t)mb;
        const uint32_t mh = wave_min_u32(hi);
        const uint32_t ml = wave_min_u32(hi == mh ? lo : NONE);
        cmax = __longlong_as_double((long long)~(((unsigned long long)mh << 32) | ml));
        if (lane == 0) {
            bslots[wave].pc = cmin;
            bslots[wave].uc = cmax;
        }
        __syncthreads();
        double a = f64_inf(), b = 0.0;
        for (int w = 0; w < NT / 64; ++w) {
            const double x = bslots[w].pc, y = bslots[w].uc;
            a = x < a ? x : a;
            b = y > b ? y : b;
        }
        cmin = a;
        cmax = b;
        __syncthreads();
    }
    const double scale = (cmax > cmin) ? (double)(G2G_NB - 1) / (cmax - cmin) : 0.0;
    auto bucket_of = [&](double c) -> uint32_t {  // monotone non-decreasing in c
        const double f = (c - cmin) * scale;
        uint32_t b = (uint32_t)f;
        return b > (uint32_t)(G2G_NB - 1) ? (uint32_t)(G2G_NB - 1) : b;
    };
    // ---- histogram, exclusive scan, scatter ----
    for (int b = t; b < 2 * G2G_NB; b += NT) lds16k[b] = 0;
    __syncthreads();
    for (int m = t; m < cnt; m += NT)
        __hip_atomic_fetch_add(&cursor[bucket_of(cost_of(kfirst + m * kstep))], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    {
        // thread t owns the PB consecutive buckets PB t .. PB t + PB - 1 (G2G_NB == PB * NT)
        constexpr int PB = G2G_NB / NT;
        static_assert(PB * NT == G2G_NB, "buckets per thread");
        uint32_t cb[PB], own = 0;
#pragma unroll
        for (int e = 0; e < PB; ++e) {
            cb[e] = cursor[PB * t + e];
            own += cb[e];
        }
        uint32_t incl = own;  // (a variable of its own, then the call: as the initialiser of a constant the same sum compiles to the loops below in another order)
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
    for (int m = t; m < cnt; m += NT) {
        const int k = kfirst + m * kstep;
        const uint32_t pos = __hip_atomic_fetch_add(&cursor[bucket_of(cost_of(k))], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        order[pos] = (uint32_t)k;
    }
    __syncthreads();
    // ---- test in bucket order ----
    pc = f64_inf();
    pi = NONE;
    uint32_t limit = (uint32_t)cnt;
    int round = 0;
    for (uint32_t pos0 = 0; pos0 < limit; pos0 += (NT / 64) * G2G_U) {
        double bc = f64_inf();
        uint32_t bi = NONE;
#pragma unroll
        for (int u = 0; u < G2G_U; ++u) {
            const uint32_t p = pos0 + (uint32_t)(u * (NT / 64) + wave);
            if (p < limit) {
                const uint32_t k = order[p];
                int cc = 0;
                bool free_k;
                if (DUB) {
                    const dub_path_t pth = dub_between_dev(nodes_g[k], heading[k], xg, hg, dc);
                    free_k = dub_sweep_wave(og, dc, nodes_g[k], heading[k], xg, pth, lane, cc);
                } else {
                    free_k = LARGE ? los_wave_large(og, H, nodes_g[k], xg, lane, cc) : los_wave(og, H, nodes_g[k], xg, lane, cc);
                }
                if (free_k) {  // rrt.py:318
                    const double c = cost_of((int)k);
                    if (key_lt(c, k, bc, bi)) {
                        bc = c;
                        bi = k;
                    }
                }
            }
        }
        BSlot *sl = bslots + (round & 1) * NWAVE;
        if (lane == 0) {
            sl[wave].pc = bc;
            sl[wave].pi = bi;
        }
        __syncthreads();
        double rc = f64_inf();
        uint32_t ri = NONE;
        if (lane < NT / 64) {
            rc = sl[lane].pc;
            ri = sl[lane].pi;
        }
        wave_min_f64_idx(rc, ri);
        ++round;
        if (key_lt(rc, ri, pc, pi)) {
            pc = rc;
            pi = ri;
            const uint32_t e = bend[bucket_of(pc)];  // every node that could sort before it lies before this position
            limit = e < limit ? e : limit;
        }
    }
}

}  // namespace rrtdev
