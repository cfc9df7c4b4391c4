"""Shared by the two test_*occupancy_inflate*.py: grids and windows, blocks of bytes, and the reference of epic_hip_set_occupancy_inflated_*
(include/epic_hip.h): B' by a brute-force loop over the sources in int64, handed to the existing epic_hip_set_occupancy_region_cpu.  The kernel's bricks are
32 rows x 128 columns (2-D), 8 x 16 x 128 (3-D): every axis of the large blocks spans two and is no multiple of one; the tiny block is smaller than a halo."""
import ctypes as ct
import functools
import math

import numpy as np

import occupancy_cases as C
import occupancy_region_cases as R
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic

RADII = [0, 1, 2, 3, 5, 9, 256]
GEOMS = {"2d-window": ([70, 200], (3, 5), (61, 190)), "2d-grid": ([70, 200], None, None), "2d-tiny": ([9, 11], (2, 3), (3, 4)),
         "3d-window": ([20, 37, 150], (1, 2, 3), (18, 33, 140)), "3d-grid": ([20, 37, 150], None, None)}
FLAVOURS = {   # name: (the rule, a source byte, the other bytes)
    "node": (C.NODE, 100, [0, 0, 0, 49, -1, -2]),                 # -1 unknown, -2 no_change: never a source, an obstacle when near
    "plugin": (C.COSTMAP, 254, [0, 0, 0, 100, 249]),              # unsigned, over goals; X = 255
    "keep": (dict(C.NODE, flags=C.KEEP), 127, [0, 0, 0, -1, -2]),  # far cells keep their potential
    "x126": (dict(thr=50, no_change=127, flags=0), 100, [0, 0, 0, 127, -1])}   # the largest byte is no_change: X = 126


@functools.lru_cache(maxsize=None)
def state(m):
    """(u, locked), flat: a relaxed field with goals and obstacles, computed once per grid (m a tuple)"""
    return C.previous_state(list(m)) if len(m) == 2 else R.state_3d(list(m))


def region(geom):
    m, origin, extent = GEOMS[geom]   # -> (m, origin, extent, (origin, extent) as the call takes them)
    return tuple(m), tuple(origin or (0,) * len(m)), tuple(extent or m), (origin, extent)


def block(geom, pattern, flavour):
    """uint8, shape extent.  "marks": sources in the middle, the corners, on the edges, at columns 63 / 64 / 127 / 128, beside a goal."""
    m, origin, extent, _ = region(geom)
    _, src, other = FLAVOURS[flavour]
    rng = np.random.default_rng(11)
    b = np.array(other, dtype=np.int64)[rng.integers(0, len(other), size=extent)]
    e = np.array(extent)
    if pattern == "sprinkle":
        b[rng.random(extent) < 0.02] = src
        return b.astype(np.uint8)
    marks = [e // 2] + [np.array(c) * (e - 1) for c in np.ndindex(*(2,) * len(e))]
    marks += [np.where(np.arange(len(e)) == axis, e // 2, 0) for axis in range(len(e))]
    marks += [np.append(e[:-1] // 3, x) for x in (63, 64, 127, 128) if x < e[-1]]
    u, locked = state(m)
    goals = np.argwhere(((locked != 0) & (u == 0.0)).reshape(m)) - np.array(origin)
    marks += [g + np.eye(len(e), dtype=np.int64)[-1] for g in goals if np.all(g >= 1) and np.all(g + 2 < e)][:1]
    for c in marks:
        b[tuple(c)] = src
    return b.astype(np.uint8)


def inflate(b, thr, no_change, flags, r2):
    """B' by the definition: every source marks the cells of its ball, in int64."""
    v = (b if flags & C.UNSIGNED else b.view(np.int8)).astype(np.int64)
    src = (v != no_change) & (v >= thr)
    top, reach = 255 if flags & C.UNSIGNED else 127, math.isqrt(r2)
    near = np.zeros(b.shape, dtype=bool)
    for s in np.argwhere(src):
        box = tuple(slice(max(int(c) - reach, 0), min(int(c) + reach + 1, n)) for c, n in zip(s, b.shape))
        near[box] |= sum((g.astype(np.int64) - int(c)) ** 2 for g, c in zip(np.ogrid[box], s)) <= r2
    out = b.copy()
    out[near & ~src] = top - 1 if top == no_change else top
    return out


def region_cpu(m, b, origin, extent, thr, no_change, flags, fn=eh._epic.epic_hip_set_occupancy_region_cpu, r2=(), expect=0):
    """fn (with the radius r2 = (radius_sq,)) on a host copy of state(m); returns (u, locked, changed)"""
    h, changed = Harmonic(), ct.c_ulonglong(777)
    h.set_grid(list(m), *state(m))
    o, e = (R.uints(origin), R.uints(extent)) if origin is not None else (None, None)
    assert fn(h, np.ascontiguousarray(b).ctypes.data, o, e, thr, no_change, flags, *r2, ct.byref(changed)) == expect
    return h.u_array().ravel().copy(), h.locked_array().ravel().copy(), int(changed.value)


@functools.lru_cache(maxsize=None)
def expected(geom, pattern, flavour, r2):
    m, _, _, where = region(geom)
    rule = FLAVOURS[flavour][0]
    return region_cpu(m, inflate(block(geom, pattern, flavour), r2=r2, **rule), *where, **rule)


def same(got, want):
    return np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]) and got[2] == want[2]
