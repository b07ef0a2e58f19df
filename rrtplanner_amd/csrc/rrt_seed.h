// rrt_seed.h -- grow a finished tree with new samples: turn the tree (or the view of its alive vertices, rrt_keep.h) into the loop
// state that the expansion kernels resume from.
//
// The expansion kernels keep all loop state in HBM and start at (D->i, D->j): rrt_init_kernel does nothing when D->i != 0.  What a
// finished query left there is not that state any more once branches were cut (and even uncut: slot j holds the goal row).  For the
// seed vertices 0 .. j0-1 -- the alive vertices in their original order, or the whole tree [0, j) -- these kernels write
//
//   nodes / vcost / parent   the alive vertices moved to the front, parents renumbered (the root keeps -1); slots [j0, node_stride)
//                            hold a copy of node 0 again, as rrt_init_kernel leaves them (the block kernel scans whole chunks)
//   bitmap (`sampled`)       cleared, then the cells of vertices 1 .. j0-1: the reference never puts xstart into the set
//                            (rrt.py:407-413), and the cell of a vertex that was cut can be sampled again
//   cellcnt / cellrec        the near-set records {xy, index, vcost} of the query's own cell geometry, the records of a cell in
//                            ascending vertex index, which is the order insertion leaves them in
//
//   1. rrt_seed_rank_kernel      rank[live_id[k]] = k  (rank was filled with -1: a vertex that is not alive has none)
//   2. rrt_seed_parent_kernel    new_parent[k] = rank[parent[live_id[k]]] into scratch.  Nothing is compacted in place: rank[k] <= k,
//                                so a parallel move inside one array would overwrite vertices that were not read yet.  The points and
//                                costs are already dense in the view (rrt_keep_compact_kernel gathered them).
//   3. rrt_seed_install_kernel   scratch -> tree arrays, one slot of [0, node_stride) per lane.  Without a view 1. and 2. are the
//                                identity and are not launched; this kernel then only refills the slots from j0 on.
//   4. rrt_seed_bitmap_kernel    the bits of vertices 1 .. j0-1 (atomicOr, the layout of the expansion kernels: cell = x * H + y,
//                                word cell >> 5, bit cell & 31); the words were cleared by a memset in front of it
//   5. rrt_seed_records_kernel   every wavefront OWNS the cells c with c % SEED_WAVES == its number and walks ALL vertices in index
//                                order, 64 a step: the owned ones of a step are placed behind the cell's count
//                                (wave_place_by_key, rrt_tree_dev.h).
// Every store is bounds-checked; a vertex outside the record grid or a cell past its capacity sets *err and stores nothing.
// (The views, the launch constants and the kernels' declarations: rrt_kernel_abi.h, which is all a host unit sees of this file.)
#pragma once

#include "rrt_tree_dev.h"

namespace rrtdev {

__global__ __launch_bounds__(SEED_TPB) void rrt_seed_rank_kernel(SeedView sv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= sv.j0) return;
    const int id = sv.live_id[k];
    if (id < 0 || id >= sv.j_old) {
        *sv.err = 1;
        return;
    }
    sv.rank[id] = k;
}

__global__ __launch_bounds__(SEED_TPB) void rrt_seed_parent_kernel(SeedView sv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= sv.j0) return;
    const int id = sv.live_id[k];
    int np = -1;
    if (k > 0 && id >= 0 && id < sv.j_old) {
        const int p = sv.parent[id];
        np = (p >= 0 && p < sv.j_old) ? sv.rank[p] : -1;
        if (np < 0 || np >= k) *sv.err = 1;  // every ancestor of an alive vertex is alive, and the order is kept: rank[p] < k
    }
    sv.new_parent[k] = np;
}

__global__ __launch_bounds__(SEED_TPB) void rrt_seed_install_kernel(SeedView sv) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= sv.node_stride) return;
    if (sv.live_id) {
        sv.nodes[k] = sv.live_nodes[k < sv.j0 ? k : 0];
        if (k < sv.j0) {
            sv.vcost[k] = sv.live_vcost[k];
            sv.parent[k] = sv.new_parent[k];
        }
    } else if (k >= sv.j0) {
        sv.nodes[k] = sv.nodes[0];  // (slot 0 is written by nobody: j0 >= 1)
    }
}

__global__ __launch_bounds__(SEED_TPB) void rrt_seed_bitmap_kernel(SeedView sv) {
    const int k = 1 + (int)(blockIdx.x * blockDim.x + threadIdx.x);  // (never vertex 0: rrt.py:407-413)
    if (k >= sv.j0) return;
    const uint32_t xy = sv.nodes[k];
    const uint32_t cell = (uint32_t)ux(xy) * (uint32_t)sv.H + (uint32_t)uy(xy);
    if ((cell >> 5) >= (uint32_t)sv.bitmap_words) {
        *sv.err = 1;
        return;
    }
    atomicOr(&sv.bitmap[cell >> 5], 1u << (cell & 31));  // rrt.py:426
}

__global__ __launch_bounds__(SEED_TPB) void rrt_seed_records_kernel(SeedRecords sr) {
    __shared__ uint32_t cnt_lds[SEED_TPB / 64][SEED_OWN];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int gw = (int)blockIdx.x * (SEED_TPB / 64) + wave;  // this wavefront's number: it owns the cells c with c % SEED_WAVES == gw
    if (gw >= SEED_WAVES) return;                              // (a launch with more workgroups than SEED_WG: nothing left to own)
    volatile RRT_LDS uint32_t *cnt = (volatile RRT_LDS uint32_t *)&cnt_lds[wave][0];  // of this wavefront alone
    if (lane < SEED_OWN) cnt[lane] = 0u;
    const int j0 = sr.j0;
    for (int base = 0; base < j0; base += 64) {  // (wave-uniform trip count)
        const int k = base + lane;
        const bool live = k < j0;
        const uint32_t xy = live ? sr.nodes[k] : 0u;
        const int cx = ux(xy) >> sr.cshift, cy = uy(xy) >> sr.cshift;
        const int c = cx * sr.ncy + cy;
        const bool inside = cx < sr.ncx && cy < sr.ncy;  // (then c < ncx * ncy <= MAX_CELLS)
        if (live && !inside) *sr.err = 1;
        const bool mine = live && inside && (c & (SEED_WAVES - 1)) == gw;
        wave_place_by_key<SEED_WAVES>(mine, c, cnt, [&](int cl, uint32_t pos) {
            const int64_t at = (int64_t)cl * (int64_t)sr.ccap + (int64_t)pos;
            if (pos < (uint32_t)sr.ccap && at < sr.rec_stride) {
                const unsigned long long cb = (unsigned long long)__double_as_longlong(sr.vcost[k]);
                sr.cellrec[at] = u32x4{xy, (uint32_t)k, (uint32_t)cb, (uint32_t)(cb >> 32)};
            } else {
                *sr.err = 1;
            }
        });
    }
    if (lane < SEED_OWN) sr.cellcnt[lane * SEED_WAVES + gw] = cnt[lane];  // every cell of [0, MAX_CELLS), the empty ones too
}

}  // namespace rrtdev
