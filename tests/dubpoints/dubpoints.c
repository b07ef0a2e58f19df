/* dubpoints.c -- test infrastructure: the points of one Dubins leg on the host, in the arithmetic of include/rrt_dubins.h.
 *
 * tests/poseroutesref.py restates rrt_batch_pose_routes; everything but the points it takes from the oracle.  A point is
 * fma(x, rho, x0) of a position built from fused multiply-adds (include/rrt_dubins_points.h), and neither Python nor numpy has a
 * fused multiply-add, so this one step is C: gcc with the oracle's flags (-ffp-contract=off), loaded by ctypes (build.py).
 * It shares dub_sweep_point with the kernel on purpose -- bit-exact points need bit-identical arithmetic -- and says nothing about
 * whether those formulas are right: tests/test_pose_routes_cpu.py holds the points to the oracle's own sweep cells and to numpy.
 */
#include "rrt_dubins_points.h"

/* The shortest word from pose 0 to pose 1 (angles in radians), its sweep set up as the planners do, and the points of its samples
 * k = 0 .. nsamples - 1 into out[2 * k], out[2 * k + 1] for k < cap.  *len = the word's length.  Returns nsamples, or -1 when no
 * word applies or the length is not finite. */
int32_t dubpoints_leg(double x0, double y0, double th0, double x1, double y1, double th1, double rho, double *out, int32_t cap, double *len) {
    const dub_path_t path = dub_shortest(x0, y0, th0, x1, y1, th1, rho);
    *len = path.len;
    if (path.word == DUB_NONE || !(path.len >= 0.0 && path.len < 1e9)) return -1;
    const dub_sweep_t s = dub_sweep_setup(x0, y0, th0, &path, rho);
    for (int32_t k = 0; k < s.nsamples && k < cap; ++k) dub_sweep_point(&s, k, &out[2 * k], &out[2 * k + 1]);
    return s.nsamples;
}
