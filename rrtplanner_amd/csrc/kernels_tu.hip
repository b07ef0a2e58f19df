// kernels_tu.hip -- the definitions of the expansion kernels, dealt to translation units (make passes -DRRT_TU=k) so that they
// compile side by side; the host units only launch them, through the declarations of rrt_kernel_abi.h.  No unit calls device code of
// another, so the objects link without relocatable device code.
#include <hip/hip_runtime.h>

#ifndef RRT_TU
#error "kernels_tu.hip is compiled once per unit: pass -DRRT_TU=k (the Makefile's TUS)"
#endif

#if RRT_TU == 1  // one CU per query, no barrier in the loop (RRTStandard / RRTStar)
#include "rrt_pipe.h"

#elif RRT_TU == 4  // the same pipeline for grids up to 4096 x 4096 (RRT_FLAG_LARGE_GRID): rrt_pipe_large_kernel
#define RRT_PIPE_LARGE_TU
#include "rrt_pipe.h"

#elif RRT_TU == 2  // Dubins planners: the pipeline, and the one-sample-per-iteration kernel kept as its cross-check
#include "rrt_dubins_block.h"
#include "rrt_serial.h"
namespace rrtdev {
template __global__ void rrt_expand_kernel<false, true>(BatchView);
}

#elif RRT_TU == 3  // one sample per iteration: cross-check of the block kernel, and the opt-in true rewire
#include "rrt_serial.h"
namespace rrtdev {
template __global__ void rrt_expand_kernel<false, false>(BatchView);
template __global__ void rrt_expand_kernel<true, false>(BatchView);
}

#elif RRT_TU == 5  // many goals against a finished tree (rrt_goals_kernel, rrt_goals_large_kernel), and every cell of a window of the map
                   // against it (rrt_field_kernel, rrt_field_large_kernel): not team kernels
#include "rrt_goals.h"
#include "rrt_field.h"

#elif RRT_TU == 6  // finished routes to many goals, with line-of-sight shortcuts (rrt_route_*_kernel): not a team kernel
#include "rrt_routes.h"

#elif RRT_TU == 7  // keep a finished tree when the map changes: the view of its alive vertices (rrt_keep_*_kernel): not a team kernel
#include "rrt_keep.h"

#elif RRT_TU == 8  // grow a finished tree: its loop state rebuilt from the alive vertices (rrt_seed_*_kernel), and the heading bytes of
                   // a Dubins tree's seed (rrt_pose_seed_heading_kernel): not team kernels
#include "rrt_seed.h"
#include "rrt_pose_seed.h"

#elif RRT_TU == 9  // a finished Dubins tree: many goal poses against it (rrt_pose_goals_kernel), the tree kept when the map changes
                   // (rrt_pose_keep_*_kernel), routes to many goal poses, their shortcuts and the vehicle's path along them (rrt_pose_route_*_kernel):
                   // not team kernels
#include "rrt_pose_goals.h"
#include "rrt_pose_keep.h"
#include "rrt_pose_routes.h"

#elif RRT_TU == 0  // re-root a finished tree at one of its vertices: the reversed path tested, the alive vertices ordered by depth and
                    // repriced (rrt_reroot_*_kernel), in front of the seed of unit 8; and a finished tree relaxed to shortest paths over
                    // its r-disc (rrt_relax_*_kernel), which runs the same later stages: not team kernels.  (Units 0 to 9 are taken and
                    // the numbers from 10 on are the team kernels' by tests/test_variant_matrix.py, so the relax kernels live here.)
                    // And a finished Dubins tree relaxed the same way (rrt_pose_relax_*_kernel): it launches the relax kernels' buckets
                    // and check and shares their device functions, so it lives beside them.  And a finished Dubins tree re-rooted at
                    // one of its poses (rrt_pose_reroot_*_kernel): the round and the parent pass of rrt_pose_relax.h from another root.
#include "rrt_reroot.h"
#include "rrt_relax.h"
#include "rrt_pose_relax.h"
#include "rrt_pose_reroot.h"

#elif RRT_TU == -1  // the pose cost field of a finished Dubins tree: every cell of a window of the map against it (rrt_pose_field_kernel
                    // and the gather kernel in front of it), a unit of its own: not a team kernel.  (The numbers 0 to 9 are taken and those from
                    // 10 on are the team kernels', so this one counts down.)
#include "rrt_pose_field.h"

#else  // teams of compute units: the variants that rrt_block_variants.def (included by rrt_block.h) deals to this unit
#include "rrt_block.h"
namespace rrtdev {
#define K(G, BSM, PIPE, INF) template __global__ void rrt_expand_block_kernel<G, BSM, PIPE, INF>(BatchView);
// a pipelined team as two kernels: the committer (8 waves, 256 vector registers) and the workers
#define S(G, BSM, INF)                                                        \
    template __global__ void rrt_block_commit_kernel<G, BSM, INF>(BatchView); \
    template __global__ void rrt_block_work_kernel<G, BSM, INF>(BatchView);
#define RRT_PASTE_(a, b) a##b
#define RRT_PASTE(a, b) RRT_PASTE_(a, b)
RRT_PASTE(RRT_UNIT_, RRT_TU)(K, S)  // (a unit that rrt_block_variants.def does not define is a compile error here)
#undef K
#undef S
}
#endif
