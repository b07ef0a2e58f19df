"""CPU: the parts of the large-grid path (grids up to 4096 x 4096 on rrt_pipe_large_kernel) that need no GPU.

  * include/rrt_line.h, rrt_line_cell_u26 (the walk of los_wave_large: numerators below 2^26, 32-bit integers and a float
    reciprocal) against rrt_line_cell_wide (64-bit division) on a 4096 x 4096 grid, and against rrt_line_cell on a 2048 grid;
  * which planners `plan()` sends to the large kernel (RRT._on_the_large_grid_kernel)."""
import os
import subprocess

import numpy as np
import pytest

from rrtplanner_amd import rrt as amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "rrt_line.h"
static long tot = 0;
/* every k of the segment: u26 against wide (or, small = 1, against rrt_line_cell) */
static long check(int x0, int y0, int x1, int y1, int small) {
    long bad = 0;
    rrt_line_t l = rrt_line_setup(x0, y0, x1, y1);
    for (int k = 0; k <= l.major; k++) {
        int x, y, u, v;
        rrt_line_cell_u26(&l, k, &x, &y);
        if (small) rrt_line_cell(&l, k, &u, &v); else rrt_line_cell_wide(&l, k, &u, &v);
        tot++;
        if (x != u || y != v) bad++;
    }
    return bad;
}
static unsigned long long s = 88172645463325252ull;
static int rnd(int m) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (int)((s >> 11) % (unsigned)m); }
int main(void) {
    long bad = 0; const int N = 4096, M = N - 1;
    /* from three corners to every cell of the opposite two edges */
    const int corner[3][2] = {{0, 0}, {M, 0}, {0, M}};
    for (int c = 0; c < 3; c++) {
        const int cx = corner[c][0], cy = corner[c][1], ox = M - cx, oy = M - cy;
        for (int t = 0; t < N; t++) bad += check(cx, cy, ox, t, 0) + check(cx, cy, t, oy, 0);
    }
    for (int t = 0; t < 200000; t++) bad += check(rnd(N), rnd(N), rnd(N), rnd(N), 0);
    for (int t = 0; t < 20000; t++) bad += check(rnd(2048), rnd(2048), rnd(2048), rnd(2048), 1);
    printf("%ld %ld\n", tot, bad);
    return bad != 0;
}
'''


def test_u26_walk_equals_the_wide_walk(tmp_path):
    src = tmp_path / "linecheck26.c"
    src.write_text(SRC)
    exe = tmp_path / "linecheck26"
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-lm"])
    out = subprocess.check_output([str(exe)]).decode().split()
    # 3 corners x 2 edges x 4096 segments of 4096 cells, and ~2730 cells per random segment
    assert int(out[0]) > 3 * 2 * 4096 * 4096 + 200_000 * 2000 and int(out[1]) == 0


def _og(W, H):
    og = np.ones((W, H), dtype=np.int64)  # (few free cells: the planner keeps argwhere(og == 0))
    og[0, :4] = 0
    return og


@pytest.mark.parametrize("shape", [(4096, 4096), (2049, 10), (2600, 2200), (10, 2049)])
def test_large_grids_go_to_the_large_kernel(shape):
    og = _og(*shape)
    assert amd.RRTStar(og, 100, 30, pbar=False)._on_the_large_grid_kernel()
    assert amd.RRTStandard(og, 100, pbar=False)._on_the_large_grid_kernel()
    assert amd.RRTStar(og, 262143, 30, pbar=False)._on_the_large_grid_kernel()


def test_everything_else_does_not():
    big = _og(2600, 2200)
    assert not amd.RRTStar(_og(2048, 2048), 100, 30, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStandard(_og(2048, 10), 100, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStar(_og(4097, 8), 100, 30, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStandard(_og(8, 4097), 100, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStarInformed(big, 100, 30, 10, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStar(big, 100, 30, costfn=lambda vcosts, points, v, x: 1.0, pbar=False)._on_the_large_grid_kernel()
    assert not amd.RRTStar(big, 100, 30, pbar=False, rewire="correct")._on_the_large_grid_kernel()
    assert not amd.RRTStar(big, 262144, 30, pbar=False)._on_the_large_grid_kernel()
    # the existing limits stay what they were
    assert amd.RRT.FAST_GRID_MAX == 2048 and amd.RRT.FAST_N_MAX == 262143
    assert amd.RRTStar(big, 100, 30, pbar=False)._beyond_the_kernels()
    assert amd.RRTStar(big, 100, 30, pbar=False).last_route is None


def test_the_flag_and_the_new_symbols_are_bound():
    from rrtplanner_amd import _ffi

    assert _ffi.FLAG_LARGE_GRID == 65536 and _ffi.kernel_flags(large_grid=True) == 65536 and _ffi.kernel_flags() == 0
    assert "rrt_prim_sqrt_u25" in _ffi.SYMBOLS and "rrt_prim_collisionfree_walk" in _ffi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    assert "#define RRT_FLAG_LARGE_GRID 65536u" in hdr
