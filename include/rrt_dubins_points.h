/*
 * rrt_dubins_points.h -- the points of a Dubins word's collision sweep, as doubles.
 *
 * dub_sweep_cell (rrt_dubins.h) forms the position of sample k of a prepared sweep and floors it to a grid cell.  dub_sweep_point
 * is that function up to, and not including, the two floor(... + 0.5): the same operands in the same order, so
 * floor(*px + 0.5), floor(*py + 0.5) ARE the cell dub_sweep_cell returns for the same (s, k), bit for bit, on the host and on the
 * device.  The vehicle's path along a route is made of these points (rrt_pose_routes.h); the planners keep using dub_sweep_cell,
 * which this header leaves alone.
 *
 * Plain C, usable from HIP device code and from gcc, under the rules of rrt_dubins.h (-ffp-contract=off, explicit DUB_FMA).
 */
#ifndef RRT_DUBINS_POINTS_H
#define RRT_DUBINS_POINTS_H

#include "rrt_dubins.h"

/* position of sample k (arc length k * DUB_DS from the start), before dub_sweep_cell rounds it to a cell */
RRT_DUB_FN void dub_sweep_point(const dub_sweep_t *s, int32_t k, double *px, double *py) {
    const double tau = ((double)k * DUB_DS) * s->inv_rho;
    double bx = s->x2, by = s->y2, bth = s->th2, bs = s->sn2, bc = s->cs2, dt = tau - (s->t + s->p), x, y;
    int32_t kind = s->k2;
    if (tau < s->t) {
        bx = 0.0;
        by = 0.0;
        bth = s->th0;
        bs = s->sn0;
        bc = s->cs0;
        kind = s->k0;
        dt = tau;
    } else if (tau < s->t + s->p) {
        bx = s->x1;
        by = s->y1;
        bth = s->th1;
        bs = s->sn1;
        bc = s->cs1;
        kind = s->k1;
        dt = tau - s->t;
    }
    dub_advance_pre(bx, by, bth, bs, bc, kind, dt, &x, &y);
    *px = DUB_FMA(x, s->rho, s->x0);
    *py = DUB_FMA(y, s->rho, s->y0);
}

#endif /* RRT_DUBINS_POINTS_H */
