// rrt_pose_seed.h -- grow a finished Dubins tree with new pose samples: the one thing the seed of rrt_seed.h does not carry, the
// heading byte of every seed vertex.  Everything else of the seed (rank, parent, install, bitmap, records) is rrt_seed.h's, unchanged:
// those kernels are keyed on the cell of a vertex, as the Dubins loop's nearest vertex, near set and `sampled` are.
//
//   rrt_pose_seed_heading_kernel   heading[k] = live_heading[k] for the slots k of [0, j0), one per lane.  The source is the dense copy
//                                  that rrt_pose_keep_gather_kernel left in the view (live_heading[k] = heading[live_id[k]]), never
//                                  heading[] itself: live_id[k] >= k, so a gather inside the one array would read slots that another
//                                  lane has already overwritten -- the hazard rrt_seed_parent_kernel avoids for the parents.
//                                  Without a view heading[0, j0) already holds the seed's headings and nothing is launched.
//
// It waits on no other workgroup, and the store is bounds-checked against node_stride like its neighbours'.
// Slots [j0, node_stride) of heading[] are left as they are (after a finished run slot j holds the goal's heading, the slots behind a
// cut tree's j0 hold headings of vertices that moved to the front): no kernel reads a heading before it is written.  Both expansion
// kernels read heading[v] only for a vertex v of the tree as they see it -- rrt_dubins_block_kernel for the index of a cell record
// or of a vertex below its snapshot's j, rrt_expand_kernel<false, true> through node_h(v) for v < j --, both write heading[j] when
// they insert vertex j, before j is published, and go2goal reads [0, j) and then writes slot j.
#pragma once

#include "rrt_device.h"

namespace rrtdev {

__global__ __launch_bounds__(SEED_TPB) void rrt_pose_seed_heading_kernel(uint8_t *heading, const uint8_t *live_heading, int32_t j0, int32_t node_stride) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= j0 || k >= node_stride) return;
    heading[k] = live_heading[k];
}

}  // namespace rrtdev
