// rrt_kernel_decls.h -- the expansion kernels that are plain (non-template) functions, declared for the translation unit that
// launches them (rrt_engine.hip).  Definitions: rrt_pipe.h and rrt_dubins_block.h, compiled by kernels_tu.hip.
// (The kernels of rrt_goals.h, rrt_routes.h, rrt_keep.h and rrt_seed.h come with their view structs: the engine includes those headers in
// their RRT_GOALS_DECL_ONLY / RRT_ROUTES_DECL_ONLY / RRT_KEEP_DECL_ONLY / RRT_SEED_DECL_ONLY form, units 5 to 8 of kernels_tu.hip define them.)
#pragma once

#include "rrt_kernels.h"

namespace rrtdev {

__global__ __launch_bounds__(TPB) void rrt_pipe_kernel(BatchView bv);
__global__ __launch_bounds__(TPB) void rrt_pipe_large_kernel(BatchView bv);  // grids up to 4096 x 4096 (unit 4)
__global__ __launch_bounds__(TPB) void rrt_dubins_block_kernel(BatchView bv);

}  // namespace rrtdev
