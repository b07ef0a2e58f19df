"""The inputs of the pose re-root tests (tests/test_pose_reroot_cpu.py, tests/test_pose_reroot_gpu.py): the workloads and fixtures of
poserelaxcases.py with the roots each is re-rooted at, and the restatement's answer for each (poserootref.reroot), cached per process.
test_pose_reroot_cpu.py asserts what each case is for."""
import numpy as np

import poserelaxcases as pc
import poserootref
import poseref

_cache = {}


def depths(parent, j):
    d = np.zeros(j, dtype=np.int64)
    for k in range(1, j):
        d[k] = d[int(parent[k])] + 1  # (a parent has the lower number)
    return d


def deepest_leaf(w):
    return int(np.argmax(depths(w.ro.parent, w.j)))  # the first of the deepest


def midway(w):
    """the vertex midway on the route from the root to the vertex the goal hangs on (the last vertex, where the goal was not found)"""
    v = int(w.ro.parent[w.ro.vgoal]) if w.ro.found else w.j - 1
    route = [v]
    while route[-1] != 0:
        route.append(int(w.ro.parent[route[-1]]))
    return route[len(route) // 2]


def roots_of(w):
    """0, j - 1, the deepest leaf and the vertex midway on the route to the goal, without repeats"""
    out = []
    for r in (0, w.j - 1, deepest_leaf(w), midway(w)):
        if r not in out:
            out.append(r)
    return out


def rerooted(w, root, r, og8=None, view=False):
    """poserootref.reroot of the oracle's tree of workload w at `root` with radius r (0: the old edges alone), on its own map or on og8
    (view: the tree was kept on og8)"""
    key = (w.name, root, r, None if og8 is None else og8.tobytes(), view)
    if key not in _cache:
        m = w.og8 if og8 is None else og8
        _cache[key] = poserootref.reroot(m, *pc.tree(w), root, pc.R_of(r) if r else 0, w.rho, w.nh, og8_view=m if view else None)
    return _cache[key]


def workload(name):
    """(workload, radius) of a name of poserelaxcases: a workload of poseref, a crafted fixture, or sized<j>"""
    if name in pc.WORKLOADS:
        return poseref.workload(name), pc.WORKLOADS[name]
    if name.startswith("sized"):
        return pc.sized(int(name[5:])), pc.SIZES_R
    make, r = pc.FIXTURES[name]
    return make(), r


def certified(w, r, X, og8=None):
    return poserootref.poserelaxref.certify(w.og8 if og8 is None else og8, X.pts, X.head, X.parent, X.vcost, pc.R_of(r) if r else 0, w.rho, w.nh,
                                            poserootref.old_edges_of(X), prev=X.order)
