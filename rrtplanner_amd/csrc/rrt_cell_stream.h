// rrt_cell_stream.h -- the stream of 16-byte cell records {xy, index, vcost} around a sample, and what the one-CU pipelines
// (rrt_pipe.h, rrt_dubins_block.h) keep of it: the nearest record, |within|, the per-lane smallest lower bounds.  Each kernel keeps
// its own widening policy, pricing and retirement; the team kernels' near-set stream (rrt_block_nearset.inc) shares the cell lookup.
#pragma once

#include "rrt_device.h"

namespace rrtdev {

// (diagnostic build) cycles since the last stamp go to cyc[k]; the kernel declares `cyc` and `tstamp`
#ifdef RRT_STAMPS
#define DSTAMP(k)                                               \
    do {                                                        \
        unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        cyc[k] += now_ - tstamp;                                \
        tstamp = now_;                                          \
    } while (0)
#else
#define DSTAMP(k) \
    do {          \
    } while (0)
#endif

// what a stream reads: the cell grid, the live fill counts (LDS), this wave's 64 slot words (LDS), the records and the vertex arrays
struct CellStreamView {
    int cshift, ncy, ccap, W, H;
    const RRT_LDS uint32_t *cellcnt;
    volatile RRT_LDS uint32_t *slots;  // (lanes talk to each other through it: every access as written)
    const u32x4 *cellrec;
    const uint32_t *nodes;
    const double *vcost;
};

// Which cell of a slab (lane c: `tcnt` records, the first one is record `pre` of the packed stream) the record base + lane belongs
// to, without a search and without a loop over the cells: every non-empty cell whose first record falls into this step writes its
// number into that record's slot (64 words of LDS per wave), the lanes read their slots and a running maximum over the lanes (DPP)
// carries the number to the records behind it; the lanes in front of the step's first cell start belong to the cell the last step
// ended in (`cur_c`: lane 63's answer of the step before, 0 at first).
__device__ __forceinline__ int stream_cell_of(volatile RRT_LDS uint32_t *slots, uint32_t pre, uint32_t tcnt, uint32_t base, int lane, int cur_c) {
    slots[lane] = NONE;
    const uint32_t rel = pre - base;
    __builtin_amdgcn_wave_barrier();
    if (tcnt != 0u && rel < 64u) slots[rel] = (uint32_t)lane;
    __builtin_amdgcn_wave_barrier();
    const int cv = wave_incl_max_i32((int)slots[lane]);  // (NONE = -1)
    return cv < 0 ? cur_c : cv;
}

// The records of the cells that the box of half-width `rad` around X touches, as ONE packed stream: lane l of a step takes
// record 64 * step + l of the concatenation of the cells' arrays (exclusive prefix sum of the fill counts over the lanes),
// 64 cells at a time, SD steps in flight.  f(record, live) once per step.
// Records of vertices at or above `jsnap` (inserted after the caller's snapshot) are dealt as dead lanes.
// `keep_d2`: every vertex at a squared distance up to this must be dealt (cells farther away than that are left out: the corners
// of the box, a third of its records where the cells are small against the radius).
// A tree of up to TINY (<= 64) vertices: all of them in one step, from the vertex arrays instead of the cells' (the same answers; a
// start pose that nothing can be connected to, and the first samples of every run, would otherwise walk ever larger boxes).
template <int SD, uint32_t TINY, typename F>
__device__ __forceinline__ void cell_stream_box(const CellStreamView &v, uint32_t X, int rad, uint32_t keep_d2, uint32_t jsnap, int lane, F &&f) {
    const int cshift = v.cshift, W = v.W, H = v.H;
    const bool tiny = jsnap <= TINY;
    const int x = ux(X), y = uy(X);
    const int cx0 = (x - rad < 0 ? 0 : x - rad) >> cshift, cx1 = (x + rad > W - 1 ? W - 1 : x + rad) >> cshift;
    const int cy0 = (y - rad < 0 ? 0 : y - rad) >> cshift, cy1 = (y + rad > H - 1 ? H - 1 : y + rad) >> cshift;
    const int ny = cy1 - cy0 + 1, ncr = tiny ? 1 : (cx1 - cx0 + 1) * ny;
    for (int cbase = 0; cbase < ncr; cbase += 64) {
        uint32_t tcnt = 0, toff = 0;
        if (tiny) {
            tcnt = lane == 0 ? jsnap : 0u;  // (one "cell": the vertex arrays)
        } else if (cbase + lane < ncr) {
            const int ci = cbase + lane, ccx = cx0 + ci / ny, ccy = cy0 + ci % ny, cell = ccx * v.ncy + ccy;
            // squared distance of the sample to the cell's rectangle
            const int xl = ccx << cshift, xh = xl + (1 << cshift) - 1, yl = ccy << cshift, yh = yl + (1 << cshift) - 1;
            const int ddx = x < xl ? xl - x : (x > xh ? x - xh : 0), ddy = y < yl ? yl - y : (y > yh ? y - yh : 0);
            const uint32_t md2 = (uint32_t)(ddx * ddx + ddy * ddy);
            tcnt = md2 <= keep_d2 ? v.cellcnt[cell] : 0u;
            toff = (uint32_t)cell * (uint32_t)v.ccap;
        }
        const uint32_t incl = wave_incl_sum_u32(tcnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t pre = incl - tcnt;
        int cur_c = 0;
        auto fetch = [&](uint32_t base) -> u32x4 {
            const uint32_t idx = base + (uint32_t)lane;
            const int cv = stream_cell_of(v.slots, pre, tcnt, base, lane, cur_c);
            cur_c = __builtin_amdgcn_readlane(cv, 63);
            const uint32_t cpre = (uint32_t)__builtin_amdgcn_ds_bpermute(cv << 2, (int)pre);
            const uint32_t coff = (uint32_t)__builtin_amdgcn_ds_bpermute(cv << 2, (int)toff);
            if (tiny) {
                const uint32_t k = idx < total ? idx : 0u;
                const unsigned long long cbits = (unsigned long long)__double_as_longlong(v.vcost[k]);
                return u32x4{v.nodes[k], k, (uint32_t)cbits, (uint32_t)(cbits >> 32)};
            }
            return v.cellrec[idx < total ? coff + (idx - cpre) : 0u];  // {xy, index, vcost}
        };
        // the records of the next steps are requested before this step's are looked at
        u32x4 rq[SD];
#pragma unroll
        for (int k = 0; k < SD; ++k) rq[k] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k + 1 < SD; ++k)
            if ((uint32_t)k * 64u < total) rq[k] = fetch((uint32_t)k * 64u);
        for (uint32_t base = 0; base < total; base += 64u) {
            const uint32_t ahead = base + (uint32_t)(SD - 1) * 64u;
            if (ahead < total) rq[SD - 1] = fetch(ahead);
            f(rq[0], base + (uint32_t)lane < total && rq[0].y < jsnap);
#pragma unroll
            for (int k = 0; k + 1 < SD; ++k) rq[k] = rq[k + 1];
        }
    }
}

// Radius of the first record stream and its square (the stream deals every vertex nearer than that): the rewire radius, but at
// least two cells (the planners without a near set, `star` false, have no radius, and a tiny one would leave the nearest-vertex
// search to the widening).  Without `large` r2 <= 2^24 and the radius saturates at 4096; with it r2 <= 2^26, and the float root of
// rr - 1 < 2^26 is within one of the integer root, which the two loops then reach (rad0 <= 8191).
struct StreamRadius {
    int rad0;
    uint32_t rr0;
};
__device__ __forceinline__ StreamRadius stream_radius(bool star, uint32_t r2, int cshift, bool large) {
    const uint32_t two = (uint32_t)((2 << cshift) * (2 << cshift));
    const uint32_t rr = (star && r2 > two) ? r2 : two;
    int rad0 = (!large && rr >= (1u << 23)) ? 4096 : (int)sqrtf((float)(rr - 1));
    while (rad0 > 0 && (uint32_t)(rad0 * rad0) > rr - 1) --rad0;
    while ((uint32_t)((rad0 + 1) * (rad0 + 1)) <= rr - 1) ++rad0;
    return StreamRadius{rad0, rr};
}

// Conservative single-precision lower bound of vcost + sqrt(d2) -- the cost through a vertex along the straight edge, and a bound
// of the cost along a Dubins word, which is never shorter than its chord -- below the f64 value by more than every rounding on the
// way, for costs up to ~1e5 cells (the same margins as the block kernel's screens, rrt_block.h).
// With d2 up to 2^25 (the large-grid pipeline) the conversion (float)d2 rounds too.  The relative errors on the way are then at
// most: (float)V 2^-24 of V; (float)d2 2^-24, i.e. 2^-25 of the root, plus the hardware root's one ulp 2^-23; the sum, the product
// and the difference 2^-24 each.  Together below 4 * 2^-24 + 2^-23 + 2^-25 < 3.9e-7 of the value, against a factor of 1 - 1.0e-6
// (as a float: 1 - 17 * 2^-24) and 4.0e-3 on top: the bound stays below the f64 cost with the margins as they are.
__device__ __forceinline__ float chord_lower_bound(double V, uint32_t d2) {
    const float s = ((float)V + __builtin_amdgcn_sqrtf((float)d2)) * (1.0f - 1.0e-6f) - 4.0e-3f;
    return s > 0.0f ? s : 0.0f;
}

__device__ __forceinline__ double rec_vcost(const u32x4 rc) { return __longlong_as_double((long long)(((unsigned long long)rc.w << 32) | rc.z)); }

// This lane's nearest record of a stream (smallest d2, lowest index among equals), and the wave's.
struct NearestRec {
    uint32_t d2 = NONE, idx = NONE, xy = 0, vl = 0, vh = 0;
    // a new search; the record words are only read for the lane that wins the next reduction
    __device__ __forceinline__ void restart() {
        d2 = NONE;
        idx = NONE;
    }
    // one record of a stream step; returns its squared distance to xq (NONE for a dead lane)
    __device__ __forceinline__ uint32_t take(const u32x4 rc, bool live, uint32_t xq) {
        const uint32_t rd2 = live ? dist2(rc.x, xq) : NONE;
        const bool nearer = rd2 < d2 || (rd2 == d2 && live && rc.y < idx);
        d2 = nearer ? rd2 : d2;
        idx = nearer ? rc.y : idx;
        xy = nearer ? rc.x : xy;
        vl = nearer ? rc.z : vl;
        vh = nearer ? rc.w : vh;
        return rd2;
    }
    // the wave's nearest (NONE / NONE: no lane holds a record)
    __device__ __forceinline__ void reduce(uint32_t &nn_d2, uint32_t &nn_idx) const {
        nn_d2 = d2;
        nn_idx = idx;
        wave_min_key_idx(nn_d2, nn_idx);
    }
    // the winner's record {xy, vcost}, uniform
    __device__ __forceinline__ void winner(uint32_t nn_d2, uint32_t nn_idx, uint32_t &nn_xy, uint32_t &nn_vl, uint32_t &nn_vh) const {
        const unsigned long long m = __ballot(idx == nn_idx && d2 == nn_d2);
        const int src = (int)__builtin_ctzll(m);
        nn_xy = (uint32_t)__shfl((int)xy, src);
        nn_vl = (uint32_t)__shfl((int)vl, src);
        nn_vh = (uint32_t)__shfl((int)vh, src);
    }
};

// Pass 1 over the ball (RRT*): |within| and, among this lane's hits, the entry with the smallest lower bound of its cost (lowest
// index among equals) and the second smallest bound.
struct BoundPair {
    uint32_t hits = 0;
    float m1f = __builtin_inff(), m2f = __builtin_inff();
    uint32_t m1idx = NONE, m1xy = 0, m1vl = 0, m1vh = 0;
    // d2: what NearestRec::take returned for the record (NONE for a dead lane: never below r2 <= 2^24, large grids 2^26)
    __device__ __forceinline__ void take(const u32x4 rc, uint32_t d2, uint32_t r2) {
        const bool hit = d2 < r2;  // within(), rrt.py:176-181
        hits += hit ? 1u : 0u;
        const float lb = hit ? chord_lower_bound(rec_vcost(rc), d2) : __builtin_inff();
        const bool first = lb < m1f || (lb == m1f && hit && rc.y < m1idx);
        m2f = first ? m1f : __builtin_fminf(m2f, lb);
        m1f = first ? lb : m1f;
        m1idx = first ? rc.y : m1idx;
        m1xy = first ? rc.x : m1xy;
        m1vl = first ? rc.z : m1vl;
        m1vh = first ? rc.w : m1vh;
    }
};

// Every vertex of the snapshot in turn -- 4 bytes and six instructions per vertex, four loads in flight -- where ever larger boxes
// would deal out every record of the map: the lane's nearest into `nr` (restarted here), vcost included.
__device__ __forceinline__ void scan_all_vertices(const uint32_t *nodes, const double *vcost, uint32_t jsnap, uint32_t xq, int lane, NearestRec &nr) {
    nr.restart();
    for (uint32_t b0 = 0; b0 < jsnap; b0 += 256u) {
        uint32_t xy4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = b0 + 64u * (uint32_t)u + (uint32_t)lane;
            xy4[u] = nodes[k < jsnap ? k : 0u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // (a lane meets its vertices in index order: strict < keeps the lowest index)
            const uint32_t k = b0 + 64u * (uint32_t)u + (uint32_t)lane;
            const uint32_t d2 = k < jsnap ? dist2(xy4[u], xq) : NONE;
            const bool nearer = d2 < nr.d2;
            nr.d2 = nearer ? d2 : nr.d2;
            nr.idx = nearer ? k : nr.idx;
            nr.xy = nearer ? xy4[u] : nr.xy;
        }
    }
    const unsigned long long cbits = (unsigned long long)__double_as_longlong(vcost[nr.idx != NONE ? nr.idx : 0u]);
    nr.vl = (uint32_t)cbits;
    nr.vh = (uint32_t)(cbits >> 32);
}

}  // namespace rrtdev
