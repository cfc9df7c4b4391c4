"""Shared by the two test_*occupancy_points*.py: boxes whose fastest axis crosses the 64-cell words of the bit planes, clouds with the points
that sit on an edge of the rule, sensors, and an independent statement of epic_hip_set_occupancy_points_* (include/epic_hip.h): the rule of
epic_amd/csrc/occupancy_points_rule.h restated step by step in np.float32, its block handed to the existing epic_hip_set_occupancy_inflated_cpu."""
import ctypes as ct

import numpy as np

import occupancy_cases as C
import occupancy_inflate_cases as I
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic

F = np.float32
WIDTHS = [1, 63, 64, 65, 129]
GEOMS = {"%dd-%d" % (n, w): ((40, 200), (3, 5), (30, w)) if n == 2 else ((12, 20, 140), (1, 2, 5), (9, 15, w)) for n in (2, 3) for w in WIDTHS}
GEOMS.update({"2d-grid": ((40, 200), None, None), "3d-grid": ((12, 20, 140), None, None)})   # origin 0: a coordinate of -0.0 is inside
PLUGIN = dict(C.COSTMAP, no_change=255)   # unsigned bytes, over goals; no_change must be a byte here, and X is 254
RULES = [(0, C.NODE), (1, PLUGIN), (9, C.NODE), (9, dict(C.NODE, flags=C.OVER)), (1, dict(C.NODE, flags=C.KEEP))]   # (radius_sq, rule)
SENSORS = ["none", "corner", "hit"]


def box(geom):
    m, origin, extent = GEOMS[geom]
    return m, np.array(origin or (0,) * len(m)), np.array(extent or m), (origin, extent)


def cloud(geom, count=65, sensor="none"):
    """(points, sensor), float32 in (x, y[, z]) order.  The first points: on integer coordinates (the box's first cell), on the last face, at -0.0,
    just outside on either side, NaN, +-inf, 3e9, and one behind a goal as seen from the sensor; then random ones in and around the box.
    count 5000: most of them in three words of the planes."""
    m, o, e, _ = box(geom)
    rng, lo, hi = np.random.default_rng(len(geom) + count), o[::-1].astype(F), (o + e)[::-1].astype(F)
    s = {"none": None, "corner": lo + F(0.25), "hit": lo + F(0.5)}[sensor]   # "hit": in the cell of the first point
    special = [lo, hi - 1, np.where(np.arange(len(m)) == 0, F(-0.0), lo), hi, lo - F(1e-3), lo + F(np.nan), lo + F(np.inf), lo - F(np.inf),
               np.where(np.arange(len(m)) == 0, F(3e9), lo), np.where(np.arange(len(m)) == 1, F(-3e9), lo + 1)]
    u, locked = I.state(m)
    goals = [g for g in np.argwhere(((locked != 0) & (u == 0.0)).reshape(m)) if np.all(g >= o) and np.all(g < o + e)]
    if goals and s is not None:
        special.append(s + F(1.5) * ((goals[0][::-1] + 0.5).astype(F) - s))
    pts = rng.uniform(lo - 2, hi + 2, size=(max(count - len(special), 0), len(m)))
    if count == 5000:
        pts[500:, 0] = rng.uniform(lo[0], min(lo[0] + 64, hi[0]), size=len(pts) - 500)
        pts[500:, 1:] = lo[1:] + rng.integers(0, 3, size=(len(pts) - 500, 1)) + 0.5
    return np.ascontiguousarray(np.concatenate([np.array(special, dtype=F), pts.astype(F)])[:count]), s


def cell(v):
    return int(np.floor(v)) if np.isfinite(v) and abs(float(v)) < 2.0 ** 31 else None


def ray_cells(o, e, s, p):
    """The cells a ray clears, in the order of m; s, p: float32 in the order of m"""
    n, cs, ce = len(o), [cell(v) for v in s], [cell(v) for v in p]
    rem = [abs(b - a) if b is not None else 2 ** 32 - 1 for a, b in zip(cs, ce)]
    step = [int(np.sign(b - a)) if b is not None else (1 if v > 0 else -1) for a, b, v in zip(cs, ce, p)]
    with np.errstate(all="ignore"):
        d = np.abs(p - s)
        tmax = np.array([(F(a + 1) - v if k > 0 else v - F(a)) for a, v, k in zip(cs, s, step)], dtype=F) / d
        tdelta = F(1.0) / d
    cur = list(cs)
    for _ in range(min(sum(rem), int(sum(e)))):
        yield tuple(cur)
        a = min((a for a in range(n) if rem[a]), key=lambda a: tmax[a])   # the first of the smallest
        cur[a], rem[a], tmax[a] = cur[a] + step[a], rem[a] - 1, tmax[a] + tdelta[a]
        if not o[a] <= cur[a] < o[a] + e[a]:
            return


def block(geom, points, sensor, no_change, flags):
    """B by the rule, uint8 of shape extent"""
    m, o, e, _ = box(geom)
    top = 255 if flags & C.UNSIGNED else 127
    B = np.full(tuple(e), no_change & 0xff, dtype=np.uint8)
    pts = points.reshape(-1, len(m))[:, ::-1]
    pts = pts[np.all(np.isfinite(pts), axis=1)]
    for c in (c for p in pts for c in ray_cells(o, e, sensor[::-1], p)) if sensor is not None else ():
        B[tuple(np.array(c) - o)] = 0
    for c in ([cell(v) for v in p] for p in pts):
        if all(ci is not None and oi <= ci < oi + ei for ci, oi, ei in zip(c, o, e)):
            B[tuple(np.array(c) - o)] = top - 1 if top == no_change else top
    return B


def points_cpu(h, geom, points, sensor, thr, no_change, flags, r2, fn=eh._epic.epic_hip_set_occupancy_points_cpu, tail=(), expect=0, count=None):
    """fn on h; returns changed (777 where the call left it alone)"""
    changed, where = ct.c_ulonglong(777), box(geom)[3]
    o, e = (I.R.uints(where[0]), I.R.uints(where[1])) if where[0] is not None else (None, None)
    n = len(points) if count is None else count
    assert fn(h, n, points.ctypes.data if points is not None else None, sensor.ctypes.data if sensor is not None else None, o, e, thr, no_change, flags,
              r2, ct.byref(changed), *tail) == expect
    return int(changed.value)


def twin(geom, points, sensor, r2, rule=None, **kw):
    """(u, locked, changed) of the CPU twin on a host copy of the state; the rule as a dict or as keywords"""
    h = Harmonic()
    h.set_grid(list(box(geom)[0]), *I.state(box(geom)[0]))
    changed = points_cpu(h, geom, points, sensor, r2=r2, **(rule or {}), **kw)
    return h.u_array().ravel().copy(), h.locked_array().ravel().copy(), changed


def bad_calls(geom):
    """{name: arguments of points_cpu} that must return EPIC_ERROR_INVALID_DATA and touch nothing"""
    points, sensor = cloud(geom, 65, "corner")
    good = dict(points=points, sensor=sensor, r2=1, **C.NODE)
    return {"sensor-outside": dict(good, sensor=sensor - F(1)), "sensor-nan": dict(good, sensor=sensor * F(np.nan)), "no_change": dict(good, no_change=-129),
            "threshold": dict(good, thr=0), "null-points": dict(good, points=None, count=3), "radius": dict(good, r2=257)}
