"""Host restatement of go2goal's decision (rrt.py:311-319) for many goals against one tree: the check of the connect_goals tests.

cost[k] = vcost[k] + sqrt(d2(k, goal)) in f64 over the vertices [0, j) -- d2 is an integer below 2^25, so numpy's root is the
correctly rounded one, as the device's is --, np.argsort(kind="stable"), then the oracle's literal line walk in that order until
one is free.  Nothing here is shortened: a goal on an obstacle cell walks every vertex and finds none."""
import numpy as np

import oracle


def connect_one(og8, pts, vcost, j, goal):
    """(vertex or -1, cost or inf, lines walked) for one goal"""
    p = np.asarray(pts[:j], dtype=np.int64)
    d = p - np.asarray(goal, dtype=np.int64)
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    cost = np.asarray(vcost[:j], dtype=np.float64) + np.sqrt(d2.astype(np.float64))
    for tried, k in enumerate(np.argsort(cost, kind="stable").tolist()):
        if oracle.collisionfree(og8, p[k], goal)[0]:
            return k, cost[k], tried + 1
    return -1, np.inf, j


def connect(og8, pts, vcost, j, goals):
    """(vertex int32[M], cost float64[M], tried int64[M]): tried[g] == 1 means the (cost, index)-smallest vertex saw the goal,
    more than 1 that it was blocked"""
    goals = np.asarray(goals).reshape(-1, 2)
    out = [connect_one(og8, pts, vcost, j, g) for g in goals]
    return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.int64))
