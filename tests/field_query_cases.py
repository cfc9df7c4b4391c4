"""Shared inputs of the field-query tests (tests/test_field_query_cpu.py, test_gpu_field_query.py, test_gpu_field_query_states.py):
grids, seeded points, edge points, regions, and thin wrappers of the C calls (include/epic_hip.h, "Field queries").

Grids: the faces are locked obstacles (epic_amd.synthetic), seeded interior obstacles, a goal at the centre, and a walled-off pocket
whose free cells stay at -1e6 -- every difference inside it is exactly 0, which is EPIC_HIP_QUERY_FLAT.  2-D: 37 x 300 (two
256-column strips of u and of the lane masks) and 20 x 70; 3-D: (12, 20, 37) and (6, 9, 300), the shapes of tests/test_gpu_field3d.py.
Seeds, densities and the mix of the drawn points were chosen on the host so that the floors of test_field_query_cpu.py hold."""
import ctypes as ct

import numpy as np

from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

E = eh._epic
OK, INVALID_LOCATION, INVALID_GRADIENT, FLAT = 0, 1, 2, 3
UP = ct.POINTER(ct.c_uint)
CDS = (0.5, 0.25, 0.3)
N_POINTS = 2400

# m -> (seed, density, pocket): pocket = per axis of m the first and last FREE index of the walled-off box
GRIDS_2D = {(37, 300): (20240601, 0.04, ((4, 10), (262, 275))), (20, 70): (20240602, 0.04, ((3, 8), (5, 14)))}
GRIDS_3D = {(12, 20, 37): (20240601, 0.02, ((2, 5), (3, 8), (4, 10))), (6, 9, 300): (20240601, 0.02, ((1, 4), (1, 4), (250, 262)))}
GRIDS = {**GRIDS_2D, **GRIDS_3D}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).ravel().view(np.uint32)


def initial(m):
    """(u, locked, pocket mask) of grid m before any relaxation: free cells scrambled to distinct values, the pocket at -1e6"""
    import _oracle as O

    seed, density, pocket = GRIDS[tuple(m)]
    u, locked = synthetic_grid(list(m), seed, density)
    U, L = u.reshape(m), locked.reshape(m)
    goal = tuple(d // 2 for d in m)
    wall = tuple(slice(max(lo - 1, 0), min(hi + 2, d)) for (lo, hi), d in zip(pocket, m))
    inside = tuple(slice(lo, hi + 1) for lo, hi in pocket)
    assert not all(s.start <= g < s.stop for s, g in zip(wall, goal)), "the goal must stay outside the pocket"
    L[wall] = 1
    U[wall] = -1e6
    L[inside] = 0
    pocket_mask = np.zeros(m, dtype=bool)
    pocket_mask[inside] = True
    # the faces stay locked obstacles whatever the pocket did
    for ax in range(len(m)):
        for face in (0, m[ax] - 1):
            idx = [slice(None)] * len(m)
            idx[ax] = face
            L[tuple(idx)] = 1
            U[tuple(idx)] = -1e6
            pocket_mask[tuple(idx)] = False
    O.scramble_free(list(m), u, locked, seed=77)
    U[pocket_mask] = -1e6
    return u, locked, pocket_mask


def make(m, u, locked, eps=1e-4, stagger=100):
    h = Harmonic()
    h.set_grid(list(m), u, locked)
    h.epsilon = eps
    h.numIterationsToStaggerCheck = stagger
    return h


def host_field(m, iterations=40):
    """A Harmonic on grid m after a few dozen host iterations: rough enough that no two free cells agree, smooth enough to have
    gradients"""
    u, locked, _ = initial(m)
    h = make(m, u, locked)
    for _ in range(iterations):
        assert E.harmonic_update_cpu(h) == 0
    return h


def points(m, n=N_POINTS, seed=5):
    """n seeded points (x, y[, z]) with every coordinate in [1.5, dim - 2.5]: 64 % uniform, 12 % inside the pocket, 12 % on obstacle
    cells, 12 % within a cell of an obstacle"""
    _, _, pocket = GRIDS[tuple(m)]
    _, locked, pocket_mask = initial(m)
    rng = np.random.default_rng(seed)
    dims = np.array(m[::-1], dtype=np.float64)                      # extent along x, y[, z]
    lo, hi = np.full(len(m), 1.5), dims - 2.5
    L = locked.reshape(m)
    obst = np.argwhere((L[tuple(slice(1, -1) for _ in m)] != 0)) + 1   # interior obstacle cells, in the order of m
    n_pocket = n_obst = n_near = n * 12 // 100
    pts = [rng.uniform(lo, hi, (n - n_pocket - n_obst - n_near, len(m)))]
    plo = np.array([p[0] for p in pocket][::-1]) + 0.6
    phi = np.array([p[1] for p in pocket][::-1]) - 0.6
    pts.append(rng.uniform(plo, phi, (n_pocket, len(m))))
    pick = obst[rng.choice(len(obst), n_obst)]
    pts.append(pick[:, ::-1] + rng.uniform(-0.3, 0.3, (n_obst, len(m))))
    pick = obst[rng.choice(len(obst), n_near)]
    pts.append(pick[:, ::-1] + rng.uniform(-1.2, 1.2, (n_near, len(m))))
    p = np.clip(np.concatenate(pts), lo, hi).astype(np.float32)
    p = np.clip(p, np.float32(1.5), (dims - 2.5).astype(np.float32))   # (the rounding to f32 must not leave the range)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def edge_points(m):
    """Points with one coordinate that is NaN, +-inf, negative, at or past the far face, or at least 2^63 in magnitude; the other
    coordinates sit on a free-looking interior position.  No status at any of them may be OK."""
    dims = m[::-1]
    base = [float(d // 2) + 0.25 for d in dims]
    bad = [np.nan, np.inf, -np.inf, -0.2, -0.7, -3.0, -1e9, 2.0 ** 63, -2.0 ** 63, 1e19, -1e19, 3e38, -3e38]
    pts = []
    for ax in range(len(m)):
        for v in bad + [dims[ax] - 0.6, dims[ax] + 0.0, dims[ax] + 7.5, 4294967296.0 + 3.0]:
            p = list(base)
            p[ax] = v
            pts.append(p)
    pts.append([np.nan] * len(m))
    pts.append([-np.inf] * len(m))
    return np.ascontiguousarray(np.array(pts, dtype=np.float32))


def regions(m):
    """(origin, extent) pairs in the order of m: the grid (None, None), a single cell, both corners, and a window whose column origin
    and width are not multiples of 4 -- crossing column 256 where the grid has one"""
    n = len(m)
    out = [(None, None), (tuple(d // 2 for d in m), (1,) * n), ((0,) * n, tuple(min(3, d) for d in m[:-1]) + (5,)),
           tuple(zip(*[(d - e, e) for d, e in zip(m, (2,) * (n - 1) + (7,))]))]
    col = (251, 13) if m[-1] > 270 else (5, 13)
    lead = [(1, min(4, d - 2)) for d in m[:-1]]
    out.append((tuple(o for o, _ in lead) + (col[0],), tuple(e for _, e in lead) + (col[1],)))
    if m[-1] > 270:
        out.append((tuple(o for o, _ in lead) + (0,), tuple(e for _, e in lead) + (m[-1],)))   # full rows: two strips, the second partial
    return out


def region_args(origin, extent):
    if origin is None:
        return None, None, ()
    o, e = np.array(origin, dtype=np.uint32), np.array(extent, dtype=np.uint32)
    return o.ctypes.data_as(UP), e.ctypes.data_as(UP), (o, e)


def region_slices(m, origin, extent):
    if origin is None:
        return tuple(slice(0, d) for d in m)
    return tuple(slice(o, o + e) for o, e in zip(origin, extent))


# ---- the calls: outputs start from a sentinel so that an untouched element shows -----------------------------------
def sample_potential(h, pts, process, status=True):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    v = np.full(len(pts), np.float32(-7.5), dtype=np.float32)
    st = np.full(len(pts), 99, dtype=np.uint8)
    call = E.epic_hip_sample_potential_gpu if process == 'gpu' else E.epic_hip_sample_potential_cpu
    rc = call(h, len(pts), pts.ctypes.data, v.ctypes.data, st.ctypes.data if status else None)
    return rc, v, st


def sample_gradient(h, pts, cd, process, status=True):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    g = np.full((len(pts), pts.shape[1]), np.float32(-7.5), dtype=np.float32)
    st = np.full(len(pts), 99, dtype=np.uint8)
    call = E.epic_hip_sample_gradient_gpu if process == 'gpu' else E.epic_hip_sample_gradient_cpu
    rc = call(h, len(pts), pts.ctypes.data, cd, g.ctypes.data, st.ctypes.data if status else None)
    return rc, g, st


def flow_field(h, origin, extent, cd, process, status=True):
    m = h.shape
    o, e, keep = region_args(origin, extent)
    shape = tuple(extent) if extent is not None else m
    g = np.full(shape + (len(m),), np.float32(-7.5), dtype=np.float32)
    st = np.full(shape, 99, dtype=np.uint8)
    call = E.epic_hip_flow_field_gpu if process == 'gpu' else E.epic_hip_flow_field_cpu
    rc = call(h, o, e, cd, 0, g.ctypes.data, st.ctypes.data if status else None)
    return rc, g, st
