"""The host statement of the 3-D consumers and edits (epic_amd/csrc/harmonic_path3d_cpu.cpp; include/epic_hip.h, "3-D fields"):
epic_hip_compute_potential_3d_cpu / _gradient_3d_cpu / _path_3d_cpu and epic_hip_set_cells_3d_cpu.

The reference has no 3-D walker, so the anchor is the extrusion identity: a 3-D field whose planes all equal a 2-D field, walked
from an integer z with cdPrecision 0.5, must reproduce the 2-D walk -- itself pinned to the reference bit for bit
(tests/test_path_cpu.py) -- in every byte.  A second test swaps two axes to catch a wrong stride, the rest is the contract."""
import ctypes as ct
import os

import numpy as np
import pytest

import _oracle as O
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

E = eh._epic
G = os.path.join(O.ROOT, "tests", "golden")
F, U = ct.c_float, ct.c_uint
PF = ct.POINTER(F)
UP = ct.POINTER(U)
PLANES, Z = 5, 2.0


def bits(a):
    return np.asarray(a, dtype=np.float32).ravel().view(np.uint32)


@pytest.fixture(scope="module")
def paths():
    return np.load(os.path.join(G, "paths.npz"))


def flat_and_extruded(goldens, name):
    """(the 2-D Harmonic over the map's converged golden field, the 3-D Harmonic whose PLANES planes all equal it)"""
    m, _, locked = O.load_png_reference_rule(os.path.join(G, "maps", name + ".png"))
    u = np.asarray(goldens["maps"][name + "/converged_1e-06"], dtype=np.float32).reshape(m)
    flat, solid = Harmonic(), Harmonic()
    flat.set_grid(m, u, locked)
    solid.set_grid([PLANES] + list(m), np.repeat(u[None], PLANES, axis=0), np.repeat(np.asarray(locked).reshape(m)[None], PLANES, axis=0))
    return flat, solid


def walk3(h, x, y, z, step, cd, max_length=1000000):
    """(code, way-points as a (k, 3) array or None) of epic_hip_compute_path_3d_cpu; the array is released by harmonic_free_path_cpu."""
    k, raw = U(0), PF()
    rc = E.epic_hip_compute_path_3d_cpu(h, x, y, z, step, cd, max_length, ct.byref(k), ct.byref(raw))
    if rc != 0:
        assert not raw
        return rc, None
    pts = np.ctypeslib.as_array(raw, shape=(3 * k.value,)).copy().reshape(-1, 3)
    assert E.harmonic_free_path_cpu(ct.byref(raw)) == 0 and not raw
    return rc, pts


def walk2(lib, h, x, y, step, cd, max_length=1000000):
    k, raw = U(0), PF()
    rc = lib.harmonic_compute_path_2d_cpu(h, F(x), F(y), F(step), F(cd), U(max_length), ct.byref(k), ct.byref(raw))
    if rc != 0:
        return rc, None
    pts = np.ctypeslib.as_array(raw, shape=(2 * k.value,)).copy().reshape(-1, 2)
    E.harmonic_free_path_cpu(ct.byref(raw))   # (the same operator delete[] whichever library made it)
    return rc, pts


@pytest.mark.parametrize("name", ["basic", "maze"])
def test_extruded_field_reproduces_the_2d_walk_bit_for_bit(goldens, paths, name):
    flat, solid = flat_and_extruded(goldens, name)
    # where the compiled reference exists, its own 2-D functions are on the other side as well
    ref = O.ref()
    m2, _, locked2 = O.load_png_reference_rule(os.path.join(G, "maps", name + ".png"))
    p = O.Problem(m2, goldens["maps"][name + "/converged_1e-06"], locked2)
    walked = 0
    for j in range(6):
        sx, sy, step, _ = (float(v) for v in paths[f"{name}/path{j}_start"])
        want_rc, want = walk2(E, flat, sx, sy, step, 0.5)
        rc, pts = walk3(solid, sx, sy, Z, step, 0.5)
        assert rc == want_rc, (name, j)
        if ref is not None:
            ref_rc, ref_pts = walk2(ref, ct.byref(p.h), sx, sy, step, 0.5)
            assert ref_rc == rc and (rc != 0 or ref_pts.tobytes() == pts[:, :2].tobytes()), (name, j)
        if rc != 0:
            continue
        walked += 1
        assert len(pts) == len(want)
        assert np.array_equal(bits(pts[:, 2]), bits(np.full(len(pts), Z)))
        assert pts[:, :2].tobytes() == want.tobytes(), (name, j)
    assert walked >= 3   # the goldens' starts are mostly walkable: the identity was really exercised
    # potential and gradient at the goldens' probe points
    xs, ys = paths[name + "/probe_x"], paths[name + "/probe_y"]
    good = 0
    for x, y in zip(xs, ys):
        v2, v3 = F(7), F(7)
        rc = E.harmonic_compute_potential_2d_cpu(flat, x, y, ct.byref(v2))
        assert E.epic_hip_compute_potential_3d_cpu(solid, x, y, Z, ct.byref(v3)) == rc
        if rc == 0:
            assert bits(v3.value)[0] == bits(v2.value)[0]
        if ref is not None:
            r2 = F(7)
            assert ref.harmonic_compute_potential_2d_cpu(ct.byref(p.h), F(x), F(y), ct.byref(r2)) == rc
            assert rc != 0 or bits(r2.value)[0] == bits(v3.value)[0]
        a2, b2, a3, b3, c3 = F(7), F(7), F(7), F(7), F(7)
        rc = E.harmonic_compute_gradient_2d_cpu(flat, x, y, 0.5, ct.byref(a2), ct.byref(b2))
        assert E.epic_hip_compute_gradient_3d_cpu(solid, x, y, Z, 0.5, ct.byref(a3), ct.byref(b3), ct.byref(c3)) == rc
        if rc == 0 and not np.isnan(a2.value):
            good += 1
            assert bits(c3.value)[0] == 0                      # +0.0 exactly
            assert bits([a3.value, b3.value]).tobytes() == bits([a2.value, b2.value]).tobytes()
    assert good >= 3


@pytest.fixture(scope="module")
def relaxed():
    """synthetic_grid((12, 20, 37)), one goal, relaxed on the host to 1e-4: (m, u, locked), never modified."""
    m = [12, 20, 37]
    u, locked = synthetic_grid(m)
    h = Harmonic()
    h.set_grid(m, u, locked)
    h.epsilon = 1e-4
    assert E.harmonic_complete_cpu(h) == 0
    return m, h.u_array().copy(), h.locked_array().copy()


def test_swapping_two_axes_swaps_the_walk(relaxed):
    m, u, locked = relaxed
    a, b = Harmonic(), Harmonic()
    a.set_grid(m, u, locked)
    b.set_grid(m[::-1], np.transpose(u, (2, 1, 0)), np.transpose(locked, (2, 1, 0)))
    compared = 0
    for start in ((33.0, 14.0, 7.0), (34.0, 12.0, 5.0), (31.0, 2.0, 9.0), (12.0, 6.0, 8.0), (8.0, 8.0, 8.0), (5.0, 15.0, 9.0), (-1.0, 3.0, 3.0)):
        rc_a, pa = walk3(a, *start, 0.2, 0.5)
        rc_b, pb = walk3(b, *start[::-1], 0.2, 0.5)
        assert rc_a == rc_b, start
        if rc_a != 0:
            continue
        n = min(len(pa), len(pb)) - 2
        assert n > 10 and abs(len(pa) - len(pb)) <= 2
        # the association differs per axis, so not bit for bit: the same cells, except possibly within the last two points
        assert np.array_equal(np.floor(pa[:n] + 0.5), np.floor(pb[:n, ::-1] + 0.5)), start
        compared += 1
    assert compared >= 5


def test_codes_and_contract(relaxed, capfd):
    m, u, locked = relaxed
    h = Harmonic()
    h.set_grid(m, u, locked)
    k, raw, v = U(0), PF(), F(0)
    flat = Harmonic()
    flat.set_grid(m[1:], u[0], locked[0])
    for bad in (Harmonic(), flat):
        assert E.epic_hip_compute_path_3d_cpu(bad, 5.0, 5.0, 5.0, 0.2, 0.5, 100, ct.byref(k), ct.byref(raw)) == 2 and not raw
        assert E.epic_hip_compute_potential_3d_cpu(bad, 5.0, 5.0, 5.0, ct.byref(v)) == 2
        assert E.epic_hip_compute_gradient_3d_cpu(bad, 5.0, 5.0, 5.0, 0.5, ct.byref(v), ct.byref(v), ct.byref(v)) == 2
    assert E.epic_hip_compute_path_3d_cpu(None, 5.0, 5.0, 5.0, 0.2, 0.5, 100, ct.byref(k), ct.byref(raw)) == 2
    obstacle = np.argwhere(locked[1:-1, 1:-1, 1:-1] & (u[1:-1, 1:-1, 1:-1] < 0))[0] + 1          # (z, y, x)
    for x, y, z in ((float(obstacle[2]), float(obstacle[1]), float(obstacle[0])), (-5.0, 5.0, 5.0), (5.0, 25.0, 5.0), (5.0, 5.0, 12.0)):
        assert E.epic_hip_compute_path_3d_cpu(h, x, y, z, 0.2, 0.5, 100, ct.byref(k), ct.byref(raw)) == 10 and not raw
        assert E.epic_hip_compute_potential_3d_cpu(h, x, y, z, ct.byref(v)) == 10
    assert E.epic_hip_compute_gradient_3d_cpu(h, 1.0, 5.0, 5.0, 0.6, ct.byref(v), ct.byref(v), ct.byref(v)) == 12   # x- lands in the border obstacle
    keep = (F * 3)()
    busy = ct.cast(keep, PF)                                  # *path must be NULL on entry
    assert E.epic_hip_compute_path_3d_cpu(h, 5.0, 5.0, 5.0, 0.2, 0.5, 100, ct.byref(k), ct.byref(busy)) == 2
    # an unrelaxed field: every free cell EPIC_LOG_SPACE_FREE -- the degenerate gradient gives what it gives in 2-D (12 or 13)
    u0, l0 = synthetic_grid(m)
    raw_h, raw_flat = Harmonic(), Harmonic()
    raw_h.set_grid(m, u0, l0)
    raw_flat.set_grid(m[1:], u0.reshape(m)[5], l0.reshape(m)[5])
    free = np.argwhere(l0.reshape(m)[5, 2:-2, 2:-2] == 0)[0] + 2
    rc2, _ = walk2(E, raw_flat, float(free[1]), float(free[0]), 0.2, 0.5, 100)
    rc3, _ = walk3(raw_h, float(free[1]), float(free[0]), 5.0, 0.2, 0.5, 100)
    assert rc2 in (12, 13) and rc3 in (12, 13)
    # a successful walk ends on the goal and respects maxLength
    rc, pts = walk3(h, 12.0, 3.0, 2.0, 0.2, 0.5)
    assert rc == 0 and len(pts) > 10
    ex, ey, ez = (int(c + 0.5) for c in pts[-1])
    assert locked[ez, ey, ex] == 1 and u[ez, ey, ex] == 0.0
    rc, short = walk3(h, 12.0, 3.0, 2.0, 0.2, 0.5, 7)
    assert rc == 0 and len(short) == 7 and short.tobytes() == pts[:7].tobytes()
    assert walk3(h, 12.0, 3.0, 2.0, 0.2, 0.5, 2)[0] == 13
    err = capfd.readouterr().err
    for line in ("Error[epic_hip_compute_path_3d_cpu]: Invalid data.", "Error[epic_hip_compute_path_3d_cpu]: Invalid location.",
                 "Error[epic_hip_compute_potential_3d_cpu]: Invalid location.", "Error[epic_hip_compute_potential_3d_cpu]: Invalid data.",
                 "Error[epic_hip_compute_gradient_3d_cpu]: Failed to compute potential values.",
                 "Error[epic_hip_compute_path_3d_cpu]: Could not compute a valid path."):
        assert line in err, line


def numpy_set_cells(m, u, locked, v, types):
    """The rule in three lines: entries inside the grid with a valid type write (value, lock) of that type, in list order."""
    for (x, y, z), t in zip(v, types):
        if x < m[2] and y < m[1] and z < m[0] and t <= 2:
            u[z, y, x], locked[z, y, x] = (0.0, 1) if t == 0 else (-1e6, 1) if t == 1 else (-1e6, 0)


def test_set_cells_3d_cpu(capfd):
    m = [6, 9, 40]
    u0, l0 = synthetic_grid(m, seed=11, density=0.1)
    rng = np.random.default_rng(5)
    k = 300
    v = np.stack([rng.integers(0, m[2] + 3, k), rng.integers(0, m[1] + 2, k), rng.integers(0, m[0] + 2, k)], axis=1).astype(np.uint32)
    types = rng.integers(0, 5, k).astype(np.uint32)
    outside = int(((v[:, 0] >= m[2]) | (v[:, 1] >= m[1]) | (v[:, 2] >= m[0])).sum())
    invalid = int(((types > 2) & ~((v[:, 0] >= m[2]) | (v[:, 1] >= m[1]) | (v[:, 2] >= m[0]))).sum())
    assert outside > 10 and invalid > 10
    h = Harmonic()
    h.set_grid(m, u0, l0)
    want_u, want_l = u0.reshape(m).copy(), l0.reshape(m).copy()
    numpy_set_cells(m, want_u, want_l, v.tolist(), types.tolist())
    capfd.readouterr()
    assert E.epic_hip_set_cells_3d_cpu(h, k, v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 0
    err = capfd.readouterr().err
    assert err.count("Warning[epic_hip_set_cells_3d_cpu]: Provided vector has invalid values outside area.") == outside
    assert err.count("Warning[epic_hip_set_cells_3d_cpu]: Type is invalid. No change made.") == invalid
    assert np.array_equal(bits(h.u_array()), bits(want_u)) and np.array_equal(h.locked_array(), want_l)
    assert not np.array_equal(want_l, l0.reshape(m))
    # return codes
    assert E.epic_hip_set_cells_3d_cpu(None, k, v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 2
    assert E.epic_hip_set_cells_3d_cpu(h, 0, v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 2
    assert E.epic_hip_set_cells_3d_cpu(h, k, None, types.ctypes.data_as(UP)) == 2
    flat = Harmonic()
    flat.set_grid(m[1:], u0.reshape(m)[0], l0.reshape(m)[0])
    assert E.epic_hip_set_cells_3d_cpu(flat, k, v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 2
    assert "Error[epic_hip_set_cells_3d_cpu]: Invalid data." in capfd.readouterr().err


# Start points whose x is no index at all.  to_index is (unsigned)(long long)v: for NaN, +-inf and |v| >= 2^63 the conversion is undefined
# in C++ and x86-64 resolves it to 0x8000000000000000, a low word of 0 -- column 0, like 2^32 and -2^32, whose low words are 0 by
# arithmetic, and like -0.75 .. -0.49, which truncate to 0 after the + 0.5.  3e9 fits and lies outside the grid.  With FACE_GOAL, a cell of
# the x == 0 face, made a goal, column 0 is a usable start on which the walk ends at once (one point: EPIC_ERROR_INVALID_PATH);
# tests/test_gpu_field_states.py holds the device to the same codes.
FACE_GOAL = (0, 9, 5)
WILD_X = [float("nan"), float("inf"), float("-inf"), 1e20, -1e20, 9.3e18, 2.0 ** 32, -2.0 ** 32, 3e9, -0.75, -0.5, -0.49]
WILD_X_CODES = [13, 13, 13, 13, 13, 13, 13, 13, 10, 13, 13, 13]


def test_start_points_that_are_no_index_land_in_column_zero(relaxed):
    m, u, locked = relaxed
    h = Harmonic()
    h.set_grid(m, u, locked)
    _, y, z = FACE_GOAL
    assert [walk3(h, x, float(y), float(z), 0.2, 0.5, 300)[0] for x in WILD_X] == [10] * len(WILD_X)   # column 0 is an obstacle: the border
    v, t = np.array([FACE_GOAL], dtype=np.uint32), np.array([eh.EPIC_CELL_TYPE_GOAL], dtype=np.uint32)
    assert E.epic_hip_set_cells_3d_cpu(h, 1, v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0
    assert [walk3(h, x, float(y), float(z), 0.2, 0.5, 300)[0] for x in WILD_X] == WILD_X_CODES


def test_python_methods_on_the_host(relaxed):
    """Harmonic.compute_paths(process='cpu') and Harmonic.set_cells(process='cpu') against the ctypes calls, n == 2 and n == 3."""
    m, u, locked = relaxed
    h = Harmonic()
    h.set_grid(m, u, locked)
    starts = np.array([(30.0, 4.0, 3.0), (-5.0, 5.0, 5.0), (5.0, 15.0, 9.0)], dtype=np.float32)
    got, codes = h.compute_paths(starts, 0.2, 0.5, 4000, process='cpu')
    for i, s in enumerate(starts):
        rc, pts = walk3(h, *(float(c) for c in s), 0.2, 0.5, 4000)
        assert codes[i] == rc
        assert got[i].shape == ((0, 3) if rc else pts.shape) and (rc or got[i].tobytes() == pts.tobytes())
    assert codes[0] == 0 and codes[1] == 10
    v = np.array([(3, 4, 5), (99, 1, 1), (7, 7, 7)], dtype=np.uint32)
    t = np.array([0, 1, 1], dtype=np.uint32)
    h.set_cells(v, t, process='cpu')
    assert h.u_array()[5, 4, 3] == 0.0 and h.locked_array()[5, 4, 3] == 1 and h.u_array()[7, 7, 7] == np.float32(-1e6)
    # n == 2: the same two methods go to the reference's 2-D functions
    flat = Harmonic()
    flat.set_grid(m[1:], u[5], locked[5])
    flat.set_cells(np.array([(3, 4)], dtype=np.uint32), [0], process='cpu')
    assert flat.u_array()[4, 3] == 0.0 and flat.locked_array()[4, 3] == 1
    got, codes = flat.compute_paths(np.array([(3.0, 4.0), (-2.0, 1.0)], dtype=np.float32), 0.2, 0.5, 100, process='cpu')
    assert list(codes) == [13, 10] and got[0].shape == (0, 2)
    with pytest.raises(ValueError):
        h.compute_paths(np.zeros((2, 2), dtype=np.float32), 0.2, 0.5, 10, process='cpu')
