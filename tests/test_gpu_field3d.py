"""Consumers and sparse edits of a device-resident 3-D field (include/epic_hip.h, "3-D fields"; epic_amd/csrc/field_3d.hip,
field3d_driver.hip): epic_hip_compute_paths_3d_gpu / _path_3d_gpu / epic_hip_set_cells_3d_gpu against their host statements
(epic_amd/csrc/harmonic_path3d_cpu.cpp), byte for byte.

Grids: (12, 20, 37) -- a row's mask bits cross a 32-bit word boundary and the pitch (256) is far wider than the row; (6, 9, 300)
-- the pitch is 512, so columns 256.. live in a second 256-column strip of u and of the lane masks."""
import ctypes as ct
import os

import numpy as np
import pytest

import _oracle as O
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E = eh._epic
NT = 1024
F, U = ct.c_float, ct.c_uint
PF, UP, PI = ct.POINTER(F), ct.POINTER(U), ct.POINTER(ct.c_int)
GRIDS = [(12, 20, 37), (6, 9, 300)]
SEED, DENSITY = 20240601, 0.02        # chosen on the host: at least half of seeded_starts() walk successfully (asserted below)
GOAL, OBSTACLE, FREE = eh.EPIC_CELL_TYPE_GOAL, eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_CELL_TYPE_FREE
MAX_LEN = 600


def bits(a):
    return np.asarray(a, dtype=np.float32).ravel().view(np.uint32)


def make(m, u, locked, eps=1e-4, stagger=100):
    h = Harmonic()
    h.set_grid(list(m), u, locked)
    h.epsilon = eps
    h.numIterationsToStaggerCheck = stagger
    return h


def gpu_init(h):
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0


def gpu_fini(h):
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0, fn.__name__


def relax_on_device(h, blocks=400):
    """Blocks of 99 plain iterations and a check until the check converges; then the host arrays are made the resident field."""
    for _ in range(blocks):
        rc = E.epic_hip_update_n_gpu(h, 100, 1)
        assert rc in (0, 1)
        if rc == 1:
            break
    else:
        raise AssertionError("no convergence")
    assert E.harmonic_get_potential_values_gpu(h) == 0


def seeded_starts(m, locked, n=200, seed=3):
    """n start points (x, y, z): 70 % at interior free cells (off-centre), 10 % each on obstacles, outside the grid and in the cells
    next to a face."""
    rng = np.random.default_rng(seed)
    dims = np.array([m[2], m[1], m[0]])                       # extent along x, y, z
    L = np.asarray(locked).reshape(m)
    n_obst = n_out = n_edge = n // 10
    free = np.argwhere(L[2:-2, 2:-2, 2:-2] == 0) + 2          # (z, y, x)
    obst = np.argwhere(L[1:-1, 1:-1, 1:-1] != 0) + 1
    pts = []
    for c in free[rng.choice(len(free), n - n_obst - n_out - n_edge, replace=False)]:
        pts.append(c[::-1] + rng.uniform(-0.3, 0.3, 3))
    for c in obst[rng.choice(len(obst), n_obst, replace=len(obst) < n_obst)]:
        pts.append(c[::-1].astype(np.float64))
    for _ in range(n_out):
        p = rng.uniform(2.0, dims - 2.0)
        ax = rng.integers(0, 3)
        p[ax] = rng.uniform(-3.0, -0.6) if rng.integers(0, 2) else dims[ax] + rng.uniform(-0.4, 2.0)
        pts.append(p)
    for _ in range(n_edge):
        p = rng.uniform(2.0, dims - 3.0)
        ax = rng.integers(0, 3)
        p[ax] = (1.0 if rng.integers(0, 2) else dims[ax] - 2.0) + rng.uniform(-0.3, 0.3)
        pts.append(p)
    return np.ascontiguousarray(np.array(pts, dtype=np.float32))


def device_paths(h, starts, step, cd, max_len=MAX_LEN, call=None):
    """(rc of the call, k, per-path codes, rows of way-points) of the batched device walk; untouched floats stay NaN"""
    starts = np.ascontiguousarray(starts, dtype=np.float32)
    n, dim = starts.shape
    k = np.full(n, 12345, dtype=np.uint32)
    codes = np.full(n, -1, dtype=np.int32)
    out = np.full((n, max(dim * max_len, 1)), np.nan, dtype=np.float32)
    call = call or (E.epic_hip_compute_paths_3d_gpu if dim == 3 else E.epic_hip_compute_paths_2d_gpu)
    rc = call(h, n, starts.ctypes.data_as(PF), step, cd, max_len, k.ctypes.data_as(UP), codes.ctypes.data_as(PI), out.ctypes.data_as(PF))
    return rc, k, codes, out


def host_path(h, s, step, cd, max_len=MAX_LEN):
    k, raw = U(0), PF()
    rc = E.epic_hip_compute_path_3d_cpu(h, float(s[0]), float(s[1]), float(s[2]), step, cd, max_len, ct.byref(k), ct.byref(raw))
    if rc != 0:
        assert not raw
        return rc, None
    pts = np.ctypeslib.as_array(raw, shape=(3 * k.value,)).copy()
    assert E.harmonic_free_path_cpu(ct.byref(raw)) == 0
    return rc, pts


@pytest.fixture(scope="module", params=GRIDS, ids=lambda m: "x".join(map(str, m)))
def resident(request):
    """A 3-D Harmonic relaxed on the device to 1e-4 with the session's scheme and read back: host arrays == resident field.
    Shared by the tests that only read it."""
    m = request.param
    u0, l0 = synthetic_grid(list(m), SEED, DENSITY)
    h = make(m, u0, l0)
    gpu_init(h)
    relax_on_device(h)
    yield h
    gpu_fini(h)


# ---- 1. parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,cd", [(0.05, 0.5), (0.05, 0.4), (0.2, 0.5), (0.2, 0.4)])
def test_device_walks_equal_the_host_walks(resident, step, cd):
    h = resident
    starts = seeded_starts(h.shape, h.locked_array())
    rc, k, codes, out = device_paths(h, starts, step, cd)
    assert rc == 0
    ok = 0
    for i, s in enumerate(starts):
        want, pts = host_path(h, s, step, cd)
        assert codes[i] == want, (i, s, codes[i], want)
        if want != 0:
            assert k[i] == 0
            continue
        assert 3 * k[i] == pts.size, (i, s)
        assert out[i, :3 * k[i]].tobytes() == pts.tobytes(), (i, s)
        assert np.isnan(out[i, 3 * k[i]:]).all()               # nothing beyond the way-points that exist came back
        ok += 1
    print("grid %s step %g cd %g: %d of %d walks succeed, codes %s, longest %d points"
          % (h.shape, step, cd, ok, len(starts), sorted(set(codes.tolist())), int(k.max())))
    assert 2 * ok >= len(starts)                               # not vacuous: the host walker alone decides this
    assert set(codes.tolist()) >= {0, 10, 12}


# ---- 2. the extrusion identity on the device ------------------------------------------------------------------------
def test_extruded_field_reproduces_the_2d_device_walk(goldens):
    paths = np.load(os.path.join(O.ROOT, "tests", "golden", "paths.npz"))
    m, _, locked = O.load_png_reference_rule(os.path.join(O.ROOT, "tests", "golden", "maps", "basic.png"))
    u = np.asarray(goldens["maps"]["basic/converged_1e-06"], dtype=np.float32).reshape(m)
    flat = make(m, u, locked)
    solid = make([5] + list(m), np.repeat(u[None], 5, axis=0), np.repeat(np.asarray(locked).reshape(m)[None], 5, axis=0))
    gpu_init(flat)
    gpu_init(solid)
    steps = sorted({float(paths[f"basic/path{j}_start"][2]) for j in range(6)})
    walked = 0
    for step in steps:
        s2 = np.array([paths[f"basic/path{j}_start"][:2] for j in range(6) if float(paths[f"basic/path{j}_start"][2]) == step], dtype=np.float32)
        s3 = np.concatenate([s2, np.full((len(s2), 1), 2.0, dtype=np.float32)], axis=1)
        rc2, k2, c2, o2 = device_paths(flat, s2, step, 0.5, 20000)
        rc3, k3, c3, o3 = device_paths(solid, s3, step, 0.5, 20000)
        assert rc2 == 0 and rc3 == 0
        assert np.array_equal(c2, c3) and np.array_equal(k2, k3)
        for i in range(len(s2)):
            if c3[i] != 0:
                continue
            assert k3[i] < 20000
            p3 = o3[i, :3 * k3[i]].reshape(-1, 3)
            assert np.array_equal(bits(p3[:, 2]), bits(np.full(len(p3), 2.0)))
            assert np.ascontiguousarray(p3[:, :2]).tobytes() == o2[i, :2 * k2[i]].tobytes()
            walked += 1
    assert walked >= 3
    gpu_fini(flat)
    gpu_fini(solid)


# ---- 3. the maxLength bound -----------------------------------------------------------------------------------------
def test_max_length_bounds_the_walk_as_on_the_host(resident):
    h = resident
    starts = seeded_starts(h.shape, h.locked_array(), n=40, seed=8)
    natural = [host_path(h, s, 0.2, 0.5)[1] for s in starts]
    longest = max(len(p) // 3 for p in natural if p is not None)
    assert longest > 8
    seen = set()
    for max_len in (0, 1, 2, 3, 4, longest // 2):
        rc, k, codes, out = device_paths(h, starts, 0.2, 0.5, max_len)
        assert rc == 0
        for i, s in enumerate(starts):
            want, pts = host_path(h, s, 0.2, 0.5, max_len)
            assert codes[i] == want and k[i] == (0 if want else pts.size // 3), (max_len, i)
            assert want != 0 or (k[i] <= max_len and out[i, :3 * k[i]].tobytes() == pts.tobytes())
            seen.add((max_len, int(want), int(k[i]) == max_len))
    assert (3, 0, True) in seen and (4, 0, True) in seen and (longest // 2, 0, True) in seen and (2, 13, False) in seen


# ---- 4. the single-path wrapper -------------------------------------------------------------------------------------
def test_single_path_wrapper(resident, capfd):
    h = resident
    starts = seeded_starts(h.shape, h.locked_array(), n=40, seed=8)
    rc, k, codes, out = device_paths(h, starts, 0.2, 0.5)
    assert rc == 0
    tried = set()
    for i, s in enumerate(starts):
        if codes[i] in tried:
            continue
        tried.add(int(codes[i]))
        kk, raw = U(77), PF()
        got = E.epic_hip_compute_path_3d_gpu(h, float(s[0]), float(s[1]), float(s[2]), 0.2, 0.5, MAX_LEN, ct.byref(kk), ct.byref(raw))
        assert got == codes[i]
        if got != 0:
            assert not raw and kk.value == 77
            continue
        assert kk.value == k[i]
        pts = np.ctypeslib.as_array(raw, shape=(3 * kk.value,)).copy()
        assert E.harmonic_free_path_cpu(ct.byref(raw)) == 0 and not raw      # a new[] array
        assert pts.tobytes() == out[i, :3 * k[i]].tobytes()
    assert tried >= {0, 10, 12}
    junk = (F * 3)()
    busy = ct.cast(junk, PF)
    assert E.epic_hip_compute_path_3d_gpu(h, 5.0, 5.0, 3.0, 0.2, 0.5, 10, ct.byref(U(0)), ct.byref(busy)) == 2
    err = capfd.readouterr().err
    assert "Error[epic_hip_compute_path_3d_gpu]: Invalid location." in err and "Error[epic_hip_compute_path_3d_gpu]: Invalid data." in err


# ---- 5. sparse edits ------------------------------------------------------------------------------------------------
WALL_X, NEW_GOAL = 24, (30, 5, 3)


def edit_list(m, locked):
    """(v, types): a new goal, a wall across the grid at x = WALL_X, two obstacle cells freed, a face cell 'freed' (it stays locked on
    the device and is never swept on the host) and an entry outside the grid.  No cell twice."""
    L = np.asarray(locked).reshape(m)
    v = [NEW_GOAL] + [(WALL_X, y, z) for z in range(1, m[0] - 1) for y in range(1, m[1] - 1)]
    t = [GOAL] + [OBSTACLE] * (len(v) - 1)
    obst = [c for c in (np.argwhere(L[1:-1, 1:-1, 1:-1] != 0) + 1).tolist() if c[2] > WALL_X and tuple(c[::-1]) != NEW_GOAL][:2]   # (z, y, x)
    assert len(obst) == 2
    v += [tuple(c[::-1]) for c in obst] + [(0, 7, 4), (99, 1, 1), (5, 5, m[0])]
    t += [FREE, FREE, FREE, GOAL, OBSTACLE]
    assert len(set(v)) == len(v)
    return np.array(v, dtype=np.uint32), np.array(t, dtype=np.uint32)


def host_sequence(m, u0, l0, v, t):
    """harmonic_update_cpu x 40, epic_hip_set_cells_3d_cpu, x 40: the statement the device must reproduce"""
    h = make(m, u0, l0)
    for _ in range(40):
        assert E.harmonic_update_cpu(h) == 0
    assert E.epic_hip_set_cells_3d_cpu(h, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0
    for _ in range(40):
        assert E.harmonic_update_cpu(h) == 0
    return h


def test_sparse_edits_mid_relaxation_equal_the_host_sequence(capfd):
    m = GRIDS[0]
    u0, l0 = synthetic_grid(list(m), SEED, DENSITY)
    v, t = edit_list(m, l0)
    want = host_sequence(m, u0, l0, v, t)
    fields = []
    for track in (0, 1):
        h = make(m, u0, l0)
        gpu_init(h)
        assert E.epic_hip_set_math_mode(h, eh.MATH_PRECISE) == 0 and E.epic_hip_set_scheme(h, eh.SCHEME_REDBLACK) == 0
        assert E.epic_hip_set_activity_tracking(h, track) == 0
        for _ in range(40):
            assert E.harmonic_update_gpu(h, NT) == 0          # single calls: deferred iterations are pending at the edit
        assert E.epic_hip_set_cells_3d_gpu(h, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0
        assert E.epic_hip_set_cells_3d_cpu(h, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0   # as a node does: the host's lock array follows (u is read back below)
        for _ in range(40):
            assert E.harmonic_update_gpu(h, NT) == 0
        assert E.harmonic_get_potential_values_gpu(h) == 0
        assert h.currentIteration == 80
        fields.append(h.u_array().copy())
        assert np.array_equal(bits(fields[-1]), bits(want.u_array())), "tracking %d" % track
        if track == 0:
            # relax to 1e-4 and walk from behind the new wall towards the new goal
            relax_on_device(h)
            start = np.array([(34.0, 9.0, 2.0), (26.0, 8.0, 2.0), (33.0, 8.0, 2.0)], dtype=np.float32)
            rc, k, codes, out = device_paths(h, start, 0.2, 0.5, 4000)
            assert rc == 0
            reached = 0
            for i, s in enumerate(start):
                wrc, pts = host_path(h, s, 0.2, 0.5, 4000)
                assert codes[i] == wrc and (wrc != 0 or out[i, :3 * k[i]].tobytes() == pts.tobytes())
                if wrc == 0:
                    end = out[i, 3 * k[i] - 3:3 * k[i]]
                    assert (out[i, 0:3 * k[i]:3] > WALL_X + 0.5).all()          # never through the wall
                    reached += tuple(int(c + 0.5) for c in end) == NEW_GOAL
            assert reached >= 1
        gpu_fini(h)
    assert np.array_equal(bits(fields[0]), bits(fields[1]))
    assert not np.array_equal(bits(fields[0]), bits(host_sequence(m, u0, l0, v[:1], np.array([7], dtype=np.uint32)).u_array()))   # the edit mattered


# ---- 6. rejections --------------------------------------------------------------------------------------------------
def test_rejections(capfd):
    m3, m2 = GRIDS[0], (20, 37)
    u3, l3 = synthetic_grid(list(m3), SEED, DENSITY)
    u2, l2 = synthetic_grid(list(m2), SEED, DENSITY)
    solid, flat = make(m3, u3, l3), make(m2, u2, l2)
    v3 = np.array([(3, 4, 5)], dtype=np.uint32)
    v2 = np.array([(3, 4)], dtype=np.uint32)
    t = np.array([OBSTACLE], dtype=np.uint32)
    s3 = np.array([(5.0, 5.0, 5.0)], dtype=np.float32)
    s2 = np.array([(5.0, 5.0)], dtype=np.float32)

    def calls_3d(h):
        kk, raw = U(0), PF()
        return (device_paths(h, s3, 0.2, 0.5, 50, E.epic_hip_compute_paths_3d_gpu)[0],
                E.epic_hip_compute_path_3d_gpu(h, 5.0, 5.0, 5.0, 0.2, 0.5, 50, ct.byref(kk), ct.byref(raw)),
                E.epic_hip_set_cells_3d_gpu(h, 1, v3.ctypes.data_as(UP), t.ctypes.data_as(UP)))

    def calls_2d(h):
        kk, raw = U(0), PF()
        return (device_paths(h, s2, 0.2, 0.5, 50, E.epic_hip_compute_paths_2d_gpu)[0],
                E.epic_hip_compute_path_2d_gpu(h, 5.0, 5.0, 0.2, 0.5, 50, ct.byref(kk), ct.byref(raw)),
                E.harmonic_utilities_set_cells_2d_gpu(h, NT, 1, v2.ctypes.data_as(UP), t.ctypes.data_as(UP)))

    assert calls_3d(solid) == (2, 2, 2)                        # no device state
    gpu_init(solid)
    gpu_init(flat)
    assert calls_3d(flat) == (2, 2, 2)                         # the 3-D calls on a 2-D Harmonic
    assert calls_2d(solid) == (2, 2, 2)                        # the 2-D calls on a 3-D Harmonic: unchanged
    assert calls_3d(None) == (2, 2, 2)
    kk = U(0)
    assert E.epic_hip_set_cells_3d_gpu(solid, 0, v3.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 2
    assert E.epic_hip_set_cells_3d_gpu(solid, 1, None, t.ctypes.data_as(UP)) == 2
    assert E.epic_hip_compute_paths_3d_gpu(solid, 0, s3.ctypes.data_as(PF), 0.2, 0.5, 50, ct.byref(kk), None, None) == 2
    gpu_fini(solid)
    gpu_fini(flat)
    capfd.readouterr()
    # several devices in one process: plane slabs are not built for these calls, and they say where to go instead
    os.environ["EPIC_HIP_DEVICES"] = "0,0"
    try:
        assert E.epic_hip_config_reload(None) == 0
        multi = make(m3, u3, l3)
        gpu_init(multi)
        assert E.epic_hip_device_layout(multi, 0, None, None, None, None) == 2
        assert calls_3d(multi) == (2, 2, 2)
        err = capfd.readouterr().err
        assert "Error[epic_hip_compute_paths_3d_gpu]: Invalid data (not available in multi-device mode: use harmonic_get_potential_values_gpu and epic_hip_compute_path_3d_cpu)." in err
        assert "Error[epic_hip_set_cells_3d_gpu]: Invalid data (not available in multi-device mode: use epic_hip_set_cells_3d_cpu and harmonic_update_model_gpu)." in err
        # the route the message names works
        assert E.epic_hip_update_n_gpu(multi, 20, 1) in (0, 1)
        assert E.harmonic_get_potential_values_gpu(multi) == 0
        gpu_fini(multi)
    finally:
        del os.environ["EPIC_HIP_DEVICES"]
        E.epic_hip_config_reload(None)


# ---- 7. the Python class --------------------------------------------------------------------------------------------
def test_python_methods_agree_with_the_c_calls(resident):
    h = resident
    starts = seeded_starts(h.shape, h.locked_array(), n=40, seed=8)
    rc, k, codes, out = device_paths(h, starts, 0.2, 0.5)
    assert rc == 0
    for process in ("gpu", "cpu"):
        got, got_codes = h.compute_paths(starts, 0.2, 0.5, MAX_LEN, process=process)
        assert np.array_equal(got_codes, codes)
        for i in range(len(starts)):
            assert got[i].shape == (k[i], 3) and got[i].tobytes() == out[i, :3 * k[i]].tobytes()
    # set_cells, n == 3 and n == 2, on fresh state: 'both' edits the host arrays and the device state alike
    for m in (GRIDS[0], (20, 37)):
        n = len(m)
        u0, l0 = synthetic_grid(list(m), SEED, DENSITY)
        a, b = make(m, u0, l0), make(m, u0, l0)
        v = np.ascontiguousarray(np.array([(30, 5, 3), (7, 8, 4), (99, 1, 1)], dtype=np.uint32)[:, :n])
        t = np.array([GOAL, OBSTACLE, OBSTACLE], dtype=np.uint32)
        for h2 in (a, b):
            gpu_init(h2)
            assert E.epic_hip_update_n_gpu(h2, 10, 0) == 0
        a.set_cells(v, t)
        args = (len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP))
        if n == 3:
            assert E.epic_hip_set_cells_3d_cpu(b, *args) == 0 and E.epic_hip_set_cells_3d_gpu(b, *args) == 0
        else:
            assert E.harmonic_utilities_set_cells_2d_cpu(b, *args) == 0 and E.harmonic_utilities_set_cells_2d_gpu(b, NT, *args) == 0
        assert np.array_equal(a.locked_array(), b.locked_array()) and a.locked_array().reshape(m)[tuple(int(c) for c in v[0][::-1])] == 1
        for h2 in (a, b):
            assert E.epic_hip_update_n_gpu(h2, 10, 0) == 0 and E.harmonic_get_potential_values_gpu(h2) == 0
        assert np.array_equal(bits(a.u_array()), bits(b.u_array()))
        assert a.u_array().reshape(m)[tuple(int(c) for c in v[0][::-1])] == 0.0
        if n == 2:
            s2 = np.array([(5.3, 7.2), (-4.0, 3.0), (30.0, 12.0)], dtype=np.float32)
            r2, k2, c2, o2 = device_paths(a, s2, 0.2, 0.5)
            got, got_codes = a.compute_paths(s2, 0.2, 0.5, MAX_LEN)
            assert r2 == 0 and np.array_equal(got_codes, c2)
            assert all(got[i].tobytes() == o2[i, :2 * k2[i]].tobytes() for i in range(len(s2)))
        for h2 in (a, b):
            gpu_fini(h2)
