"""Shared by tests/test_occupancy_region_cpu.py and tests/test_gpu_occupancy_region.py: the grids, the windows and boxes at the
edges where an index error would sit, 3-D previous states and images, the callers' list route in 3-D, and the numpy statement of the
rule of epic_hip_set_occupancy_region_* (include/epic_hip.h) for n in {2, 3}, masked to a region.  Everything 2-D that exists
already comes from occupancy_cases.py."""
import ctypes as ct

import numpy as np

import _oracle as O
import occupancy_cases as C
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic_map import LOG_SPACE_FREE, LOG_SPACE_GOAL, LOG_SPACE_OBSTACLE
from epic_amd.synthetic import synthetic_grid

UP = C.UP
GRIDS_2D = [[3, 5], [5, 257], [37, 301], [130, 515]]
GRIDS_3D = [[3, 3, 5], [4, 5, 257], [6, 7, 300], [5, 9, 515]]
RULES = {"node": C.NODE, "costmap": C.COSTMAP}


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v)


def windows_2d(m):
    """{name: (origin, extent)} in the order of m = [rows, cols], those that fit the grid: a single interior cell; a window anchored at
    {0, 0} (it covers border cells); one ending on the last row and column; one crossing columns 127 / 128 and 255 / 256 / 257; one with
    an odd column origin and a width that is no multiple of 4; one whose column origin and width are multiples of 4."""
    rows, cols = m
    h = min(rows - 2, 5) if rows > 3 else 1
    w = {"cell": ((min(2, rows - 2), min(3, cols - 2)), (1, 1)),
         "anchored": ((0, 0), (min(rows, 4), min(cols, 6))),
         "last": ((rows - 3, cols - 5), (3, 5))}
    if cols > 250:
        w["crossing"] = ((1, 120), (h, min(140, cols - 120)))          # columns 127 / 128 and 255 / 256 (/ 257)
    if cols >= 12:
        w["odd"] = ((1, 3), (h, 7))                                   # odd column origin, width % 4 != 0
        w["fours"] = ((1, 252), (h, 12)) if cols >= 264 else ((1, 4), (h, 8))   # origin and width multiples of 4
    return w


def boxes_3d(m):
    """{name: (origin, extent)} in the order of m, those that fit the grid: a single voxel; a box touching each of the six faces; one
    spanning every plane; one crossing x2 = 255 / 256; one with three different extents; one whose x2 origin and width are multiples of 4."""
    m0, m1, m2 = m

    def span(lo, hi):
        lo = [min(a, b - 1) for a, b in zip(lo, m)]
        hi = [max(min(a, b), l + 1) for a, b, l in zip(hi, m, lo)]
        return tuple(lo), tuple(b - a for a, b in zip(lo, hi))

    b = {"voxel": ((1, 1, min(2, m2 - 2)), (1, 1, 1)),
         "face_x0_lo": span((0, 1, 1), (2, m1 - 1, m2 - 1)),
         "face_x0_hi": span((m0 - 2, 1, 1), (m0, m1 - 1, m2 - 1)),
         "face_x1_lo": span((1, 0, 1), (m0 - 1, 2, m2 - 1)),
         "face_x1_hi": span((1, m1 - 2, 1), (m0 - 1, m1, m2 - 1)),
         "face_x2_lo": span((1, 1, 0), (m0 - 1, m1 - 1, 3)),
         "face_x2_hi": span((1, 1, m2 - 3), (m0 - 1, m1 - 1, m2)),
         "planes": span((0, 1, 2), (m0, m1 - 1, 40)),
         "extents": ((1, 1, 1), (2, 3, 5) if m0 >= 4 and m1 >= 5 else (1, 2, 3))}     # three different extents: a swapped axis order fails
    if m2 > 256:
        b["crossing"] = span((1, 1, 250), (m0 - 1, 3, 262))           # x2 = 255 / 256
    if m2 >= 16:
        b["fours"] = span((1, 1, 252), (m0 - 1, m1 - 1, 264)) if m2 >= 264 else span((1, 1, 4), (m0 - 1, m1 - 1, 12))
    return b


def state_3d(m, seed=5, density=0.08, iterations=4):
    """(u, locked), flat: a seeded 3-D grid with a few more goals, advanced a few iterations by the checker."""
    u, locked = synthetic_grid(list(m), seed, density)
    rng = np.random.default_rng(seed + 1000)
    for _ in range(min(4, (m[0] - 2) * (m[1] - 2) * (m[2] - 2) // 2)):
        cell = (int(rng.integers(1, m[0] - 1)) * m[1] + int(rng.integers(1, m[1] - 1))) * m[2] + int(rng.integers(1, m[2] - 1))
        u[cell] = LOG_SPACE_GOAL
        locked[cell] = 1
    p = O.Problem(m, u, locked)
    for _ in range(iterations):
        O.oracle().oracle_update(ct.byref(p.h))
    return p.u.copy(), p.locked.copy()


def image_nd(m, seed=9):
    """prod(m) bytes drawn from occupancy_cases.BYTES, shape m."""
    return C.image([int(np.prod(m[:-1])), m[-1]], seed).reshape(m)


def cut(full, origin, extent):
    """The region's bytes as the caller hands them in: contiguous, shape extent."""
    return np.ascontiguousarray(full[tuple(slice(o, o + e) for o, e in zip(origin, extent))])


def inside(m, origin, extent):
    box = np.zeros(m, dtype=bool)
    box[tuple(slice(o, o + e) for o, e in zip(origin, extent))] = True
    return box


def rule_nd(m, full, box, u, locked, thr, no_change, flags):
    """occupancy_cases.rule for n axes, masked to `box` (bool, shape m): the cells off every face that lie in the box are decided by
    their byte of `full` (shape m); returns (u, locked, changed), flat."""
    m = tuple(m)
    full = np.asarray(full).reshape(m)
    v = (full.view(np.uint8) if flags & C.UNSIGNED else full.view(np.int8)).astype(np.int32)
    u0 = np.asarray(u, dtype=np.float32).reshape(m)
    l0 = np.asarray(locked, dtype=np.uint32).reshape(m)
    inner = np.zeros(m, dtype=bool)
    inner[(slice(1, -1),) * len(m)] = True
    goal = (l0 != 0) & (u0 == 0.0)
    touched = inner & box & (v != no_change) & ~(goal & (not flags & C.OVER))
    obstacle = touched & (v >= thr)
    free = touched & ~obstacle
    u1, l1 = u0.copy(), l0.copy()
    u1[obstacle] = LOG_SPACE_OBSTACLE
    l1[obstacle] = 1
    l1[free] = 0
    u1[free & ~((l0 == 0) & bool(flags & C.KEEP))] = LOG_SPACE_FREE
    changed = ((l1 != 0) != (l0 != 0)) | ((l1 != 0) & (l0 != 0) & (u1.view(np.uint32) != u0.view(np.uint32)))
    return u1.ravel(), l1.ravel(), int(changed.sum())


def node_lists_3d(m, occ, u, locked, box=None, thr=50, no_change=-2):
    """The /map callback's lists plane by plane (occupancy_cases.node_lists on every interior plane), as (x, y, z) triples: (v, types).
    box (bool, shape m): only the cells inside it."""
    m0, m1, m2 = m
    occ, u, locked = (np.asarray(a).reshape(m) for a in (occ, u, locked))
    vs, ts = [], []
    for z in range(1, m0 - 1):
        v, t = C.node_lists([m1, m2], occ[z], u[z], locked[z], thr, no_change)
        v = v.reshape(-1, 2)
        if box is not None and len(t):
            keep = box[z][v[:, 1], v[:, 0]]
            v, t = v[keep], t[keep]
        vs.append(np.concatenate([v, np.full((len(t), 1), z, dtype=np.uint32)], axis=1))
        ts.append(t)
    return np.ascontiguousarray(np.concatenate(vs).astype(np.uint32)).ravel(), np.concatenate(ts).astype(np.uint32)


def node_lists_2d(m, occ, u, locked, box=None, thr=50, no_change=-2):
    """occupancy_cases.node_lists, only the cells inside box (bool, shape m)."""
    v, t = C.node_lists(m, occ, u, locked, thr, no_change)
    if box is not None and len(t):
        v = v.reshape(-1, 2)
        keep = box[v[:, 1], v[:, 0]]
        v, t = np.ascontiguousarray(v[keep]).ravel(), t[keep]
    return v, t


def costmap_lists_nd(m, cost, box=None, thr=250):
    """setCellsFromCostmap as a list for n axes: every cell off the faces (inside box), obstacle from the threshold on, free otherwise;
    entries are (x, y[, z]): the fastest axis first."""
    m = tuple(m)
    cost = np.asarray(cost).reshape(m)
    take = np.zeros(m, dtype=bool)
    take[(slice(1, -1),) * len(m)] = True
    if box is not None:
        take &= box
    idx = np.argwhere(take)                      # in the order of m
    v = np.ascontiguousarray(idx[:, ::-1].astype(np.uint32)).ravel()
    types = np.where(cost[take] >= thr, eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_CELL_TYPE_FREE).astype(np.uint32)
    return v, types


def reset_lists_3d(m, locked):
    """Every unlocked cell off the faces as an (x, y, z) triple, type free."""
    L = np.asarray(locked).reshape(m)
    take = np.zeros(m, dtype=bool)
    take[1:-1, 1:-1, 1:-1] = L[1:-1, 1:-1, 1:-1] == 0
    idx = np.argwhere(take)
    return np.ascontiguousarray(idx[:, ::-1].astype(np.uint32)).ravel(), np.full(len(idx), eh.EPIC_CELL_TYPE_FREE, dtype=np.uint32)


def bad_regions(m):
    """(origin, extent) pairs that do not lie inside the grid, or come with one pointer only (None)"""
    n = len(m)
    ones, zeros = [1] * n, [0] * n
    out = []
    for axis in range(n):
        def at(base, value):
            return [value if i == axis else base[i] for i in range(n)]
        out += [(zeros, at(ones, 0)),                       # an extent of 0
                (at(zeros, m[axis]), ones),                 # an origin at m[i]
                (at(zeros, m[axis] - 1), at(ones, 2)),      # origin + extent one past the end
                (zeros, at(ones, m[axis] + 1)),
                (at(zeros, 0xffffffff), at(ones, 2)),       # an origin of 0xffffffff: origin + extent wraps around
                (at(zeros, 2), at(ones, 0xffffffff))]
    return out + [(zeros, None), (None, ones)]


def uints(values):
    return (ct.c_uint * len(values))(*[int(x) for x in values])
