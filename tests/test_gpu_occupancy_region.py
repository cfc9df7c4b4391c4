"""epic_hip_set_occupancy_region_gpu / epic_hip_timed_occupancy_region_gpu / epic_hip_reset_free_cells_3d_gpu (include/epic_hip.h;
epic_amd/csrc/occupancy_region.hip, occupancy_driver.hip): a block of bytes applied to a rectangular region of the device-resident
state of a 2-D or 3-D field -- against the list route (harmonic_utilities_set_cells_2d_gpu / epic_hip_set_cells_3d_gpu on the
entries the callers would build for the region), the checker's state edited by the numpy rule, and the CPU variant.  Every
comparison is bitwise.  The grids, windows and boxes are those of tests/test_occupancy_region_cpu.py (occupancy_region_cases.py):
on the border and the faces, on the last row and column, across columns 127 / 128 and 255 / 256 / 257, origins and widths that take
the dword path and ones that take the byte path, strips covered in part."""
import ctypes as ct
import os

import numpy as np
import pytest

import _oracle as O
import occupancy_cases as C
import occupancy_region_cases as R
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E = eh._epic
NT = 1024
UP = C.UP
JACOBI, REDBLACK = eh.SCHEME_JACOBI, eh.SCHEME_REDBLACK
MODES = [(JACOBI, 0), (REDBLACK, 1), (JACOBI, 1), (REDBLACK, 0)]   # (epic_hip_set_scheme, epic_hip_set_activity_tracking)
GRIDS = R.GRIDS_2D + R.GRIDS_3D


def bits(a):
    return np.asarray(a, dtype=np.float32).ravel().view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make(m, u, locked, scheme=None, track=None, eps=1e-6, stagger=100, init=True):
    h = Harmonic()
    h.set_grid(list(m), u, locked)
    h.epsilon = eps
    h.numIterationsToStaggerCheck = stagger
    if not init:
        return h
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0
    assert E.harmonic_initialize_gpu(h, NT) == 0
    if scheme is not None:
        assert E.epic_hip_set_scheme(h, scheme) == 0
    if track is not None:
        assert E.epic_hip_set_activity_tracking(h, track) == 0
    return h


def fini(h):
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0


def plain(h, n):
    for _ in range(n):
        assert E.harmonic_update_gpu(h, NT) == 0


def check(h):
    assert E.harmonic_update_and_check_gpu(h, NT) in (0, 1)
    return float(h.delta)


def readback(h):
    assert E.harmonic_get_potential_values_gpu(h) == 0
    return h.u_array().ravel().copy()


def stats(h):
    active, tiles = ct.c_ulonglong(0), ct.c_ulonglong(0)
    assert E.epic_hip_activity_stats(h, ct.byref(active), ct.byref(tiles)) == 0
    return active.value, tiles.value


def lists_gpu(h, v, t):
    """the callers' lists: (x, y) pairs or (x, y, z) triples"""
    if len(t) == 0:
        return
    if h.n == 2:
        assert E.harmonic_utilities_set_cells_2d_gpu(h, NT, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0
    else:
        assert E.epic_hip_set_cells_3d_gpu(h, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0


def region_gpu(h, occ, origin, extent, thr, no_change, flags, fn=None, expect=0):
    occ = np.ascontiguousarray(occ)
    changed = ct.c_ulonglong(54321)
    o, e = (R.uints(origin), R.uints(extent)) if origin is not None else (None, None)
    assert (fn or E.epic_hip_set_occupancy_region_gpu)(h, occ.ctypes.data, o, e, thr, no_change, flags, ct.byref(changed)) == expect
    return int(changed.value)


def region_cpu_changed(m, occ, origin, extent, u, locked, thr, no_change, flags):
    h = make(m, u, locked, init=False)
    changed = ct.c_ulonglong(0)
    occ = np.ascontiguousarray(occ)
    assert E.epic_hip_set_occupancy_region_cpu(h, occ.ctypes.data, R.uints(origin), R.uints(extent), thr, no_change, flags, ct.byref(changed)) == 0
    return int(changed.value), h.u_array().ravel().copy()


def checker_run(p, k, scheme):
    """k iterations of `scheme` on Problem p from p.h.currentIteration on, the last one a check."""
    lib = O.oracle()
    if scheme == JACOBI:
        assert lib.oracle_jacobi_run(ct.byref(p.h), k) == 0
    else:
        for i in range(k):
            (lib.oracle_update_and_check if i == k - 1 else lib.oracle_update)(ct.byref(p.h))


_STATES = {}


def start_state(m):
    """(u0, locked, image), flat / shape m: computed once per grid, never modified"""
    key = tuple(m)
    if key not in _STATES:
        if len(m) == 2:
            u, l = synthetic_grid(list(m), 5, 0.08)
            for x, y in C.extra_goals(list(m), 5):
                u[y * m[1] + x] = 0.0
                l[y * m[1] + x] = 1
        else:
            u, l = R.state_3d(list(m), iterations=0)
        full = R.image_nd(list(m))
        for a in (u, l, full):
            a.setflags(write=False)
        _STATES[key] = (u, l, full)
    return _STATES[key]


def regions(m):
    return R.windows_2d(m) if len(m) == 2 else R.boxes_3d(m)


def caller_lists(m, case, full, box, u0, l0):
    if case == "node":
        return (R.node_lists_2d if len(m) == 2 else R.node_lists_3d)(m, full, u0, l0, box)   # the node's goal test reads its host arrays: goals never move
    return R.costmap_lists_nd(m, full.view(np.uint8), box)


def dense_against_lists(m, scheme, track, pending):
    """Two contexts, brought to the same point: one tick (a check and 24 plain updates), or -- pending -- 7 plain updates that are
    still only counted when the edit comes.  One gets the region through the new call, the other the same edit as lists.  Fields
    after the edit, and fields and delta after 60 more iterations ending in a check, are equal -- and equal to the checker's state
    edited by the numpy rule; `changed` is the rule's and the CPU variant's.  Every region under both callers' rules."""
    moved = sum(one_region(m, scheme, track, pending, name, origin, extent, case)
                for name, (origin, extent) in regions(m).items() for case in ("node", "costmap"))
    assert moved > 0 or min(m) == 3


def one_region(m, scheme, track, pending, name, origin, extent, case):
    u0, l0, full = start_state(m)
    kw = R.RULES[case]
    img = full if case == "node" else full.view(np.uint8)
    box = R.inside(m, origin, extent)
    v, t = caller_lists(m, case, full, box, u0, l0)
    a, b = make(m, u0, l0, scheme, track), make(m, u0, l0, scheme, track)
    p = O.Problem(m, u0, l0)
    if pending:
        for h in (a, b):
            plain(h, 7)
        checker_run(p, 7, scheme)
    else:
        for h in (a, b):
            check(h)
            plain(h, 24)
        checker_run(p, 1, scheme)
        checker_run(p, 24, scheme)
    lists_gpu(a, v, t)
    changed = region_gpu(b, R.cut(img, origin, extent), origin, extent, **kw)
    cpu_changed, cpu_u = region_cpu_changed(m, R.cut(img, origin, extent), origin, extent, p.u, p.locked, **kw)
    ru, rl, rule_changed = R.rule_nd(m, img, box, p.u, p.locked, **kw)
    p.u[:], p.locked[:] = ru, rl
    assert changed == rule_changed == cpu_changed, (name, case)
    ua, ub = readback(a), readback(b)
    assert same(ua, ub) and same(ub, p.u) and same(ub, cpu_u), (name, case)
    for h in (a, b):
        plain(h, 59)
    da, db = check(a), check(b)
    checker_run(p, 60, scheme)
    ua, ub = readback(a), readback(b)
    assert same(ua, ub) and da == db, (name, case)
    assert same(ub, p.u) and db == float(p.h.delta), (name, case)
    assert a.currentIteration == b.currentIteration == p.h.currentIteration
    fini(a)
    fini(b)
    return changed


# ---- 7. the dense route against the list route ------------------------------------------------------------------------
@pytest.mark.parametrize("m", GRIDS, ids=R.ident)
@pytest.mark.parametrize("scheme,track", MODES)
def test_region_equals_the_list_route_and_the_checker(m, scheme, track):
    dense_against_lists(m, scheme, track, pending=False)


# ---- 8. pending iterations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", GRIDS, ids=R.ident)
@pytest.mark.parametrize("scheme,track", MODES)
def test_region_acts_on_the_flushed_state(m, scheme, track):
    dense_against_lists(m, scheme, track, pending=True)


# ---- 9. the whole 2-D grid is the existing call -----------------------------------------------------------------------
@pytest.mark.parametrize("m", [[64, 1024], [37, 301]], ids=R.ident)      # the dword path and the byte path of both kernels
@pytest.mark.parametrize("scheme,track", MODES)
def test_whole_2d_grid_equals_the_2d_call(m, scheme, track):
    u0, l0, full = start_state(m)
    for kw in (C.NODE, C.COSTMAP, dict(C.NODE, flags=C.KEEP)):
        a, b, c = (make(m, u0, l0, scheme, track) for _ in range(3))
        for h in (a, b, c):
            check(h)
            plain(h, 24)
        want = ct.c_ulonglong(0)
        assert E.epic_hip_set_occupancy_2d_gpu(a, full.ctypes.data, kw["thr"], kw["no_change"], kw["flags"], ct.byref(want)) == 0
        assert region_gpu(b, full, None, None, **kw) == want.value > 0
        ms = ct.c_float(-1.0)                       # the timed variant is the same call with a kernel time
        assert region_gpu(c, full, (0, 0), m, **kw, fn=lambda *args: E.epic_hip_timed_occupancy_region_gpu(*args, ct.byref(ms))) == want.value
        assert 0.0 < ms.value < 1e3
        ua = readback(a)
        assert same(ua, readback(b)) and same(ua, readback(c))
        for h in (a, b, c):
            plain(h, 59)
        da, db, dc = check(a), check(b), check(c)
        ua = readback(a)
        assert same(ua, readback(b)) and same(ua, readback(c)) and da == db == dc
        for h in (a, b, c):
            fini(h)


# ---- 10. KEEP_FREE and a window that restates the map -----------------------------------------------------------------
@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK])
def test_keep_free_with_a_restating_window_disturbs_nothing(scheme):
    m = [64, 1024]
    u0, l0, _ = start_state(m)
    restating = C.restating_image(m, u0, l0)
    origin, extent = (8, 250), (40, 530)            # strips 0 to 3, the first and the last in part
    occ = R.cut(restating, origin, extent)
    a, b = make(m, u0, l0, scheme, 1), make(m, u0, l0, scheme, 1)
    before = []
    for h in (a, b):
        check(h)
        plain(h, 39)
        before.append(stats(h))
    assert before[0] == before[1] and 0 < before[0][0] < before[0][1], before   # some tiles sleep
    field = readback(b)
    assert region_gpu(b, occ, origin, extent, **dict(C.NODE, flags=C.KEEP)) == 0
    assert stats(b) == before[1]
    assert same(readback(b), field)
    for h in (a, b):
        plain(h, 30)
    da, db = check(a), check(b)
    assert same(readback(a), readback(b)) and da == db
    # without KEEP_FREE the same window is a cold restart of its cells: every tile is woken
    assert region_gpu(b, occ, origin, extent, **C.NODE) == 0
    active, tiles = stats(b)
    assert active == tiles
    fini(a)
    fini(b)


def test_keep_free_with_a_restating_box_disturbs_nothing_3d():
    m = [6, 7, 300]
    u0, l0, _ = start_state(m)
    restating = np.where(l0.reshape(m) != 0, 100, 0).astype(np.int8)
    restating[np.random.default_rng(13).random(restating.shape) < 0.3] = -2
    origin, extent = (0, 1, 100), (6, 5, 200)
    occ = R.cut(restating, origin, extent)
    h = make(m, u0, l0, REDBLACK, 1)
    check(h)
    plain(h, 39)
    before, field = stats(h), readback(h)
    assert region_gpu(h, occ, origin, extent, **dict(C.NODE, flags=C.KEEP)) == 0
    assert stats(h) == before and same(readback(h), field)
    assert region_gpu(h, occ, origin, extent, **C.NODE) == 0
    active, tiles = stats(h)
    assert active == tiles > 0
    fini(h)


# ---- 11. reset in 3-D -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.GRIDS_3D, ids=R.ident)
def test_reset_free_cells_3d_equals_the_list_route(m):
    u0, l0, _ = start_state(m)
    v, t = R.reset_lists_3d(m, l0)
    a, b = make(m, u0, l0), make(m, u0, l0)
    for h in (a, b):
        check(h)
        plain(h, 11)
    lists_gpu(a, v, t)
    assert E.epic_hip_reset_free_cells_3d_gpu(b) == 0
    ua, ub = readback(a), readback(b)
    inner = np.zeros(m, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    free = inner.ravel() & (l0 == 0)
    assert same(ua, ub) and same(ub[free], np.full(int(free.sum()), -1e6))
    for h in (a, b):
        plain(h, 20)
    assert same(readback(a), readback(b))
    fini(a)
    fini(b)


# ---- 12. multi-device mode ---------------------------------------------------------------------------------------------
@pytest.fixture
def env():
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))
        assert E.epic_hip_config_reload(None) == 0

    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    E.epic_hip_config_reload(None)


def test_multi_device_mode_2d_window_gives_the_single_device_field(env):
    m = [130, 515]
    u0, l0, full = start_state(m)
    out = {}
    for devices in (None, "0,0"):
        env(EPIC_HIP_DEVICES=devices)
        h = make(m, u0, l0)
        assert E.epic_hip_device_layout(h, 0, None, None, None, None) == (2 if devices else 1)
        check(h)
        plain(h, 24)
        counts, fields = [], []
        for name, (origin, extent) in R.windows_2d(m).items():
            kw = dict(C.NODE, flags=C.KEEP) if name == "odd" else C.COSTMAP if name == "last" else C.NODE
            img = full.view(np.uint8) if kw is C.COSTMAP else full
            counts.append(region_gpu(h, R.cut(img, origin, extent), origin, extent, **kw))
            plain(h, 5)
            fields.append(readback(h))
        counts.append(region_gpu(h, full, None, None, **C.NODE))
        plain(h, 19)
        d = check(h)
        out[devices] = (counts, d, fields + [readback(h)])
        fini(h)
    one, two = out[None], out["0,0"]
    assert one[:2] == two[:2] and sum(one[0]) > 0
    assert all(same(x, y) for x, y in zip(one[2], two[2]))


def test_multi_device_mode_3d_names_the_host_route(env, capfd):
    m = [12, 20, 37]
    u0, l0 = synthetic_grid(m, 20240601, 0.02)
    env(EPIC_HIP_DEVICES="0,0")
    h = make(m, u0, l0)
    assert E.epic_hip_device_layout(h, 0, None, None, None, None) == 2
    plain(h, 3)
    occ = np.full(m, 100, dtype=np.int8)
    ms = ct.c_float(0.0)
    capfd.readouterr()
    assert region_gpu(h, occ, None, None, **C.NODE, expect=2) == 54321
    assert region_gpu(h, occ[1:3, 1:3, 1:3], (1, 1, 1), (2, 2, 2), **C.NODE, expect=2,
                      fn=lambda *args: E.epic_hip_timed_occupancy_region_gpu(*args, ct.byref(ms))) == 54321
    assert E.epic_hip_reset_free_cells_3d_gpu(h) == 2
    err = capfd.readouterr().err
    route = "Invalid data (not available in multi-device mode: use %s and harmonic_update_model_gpu)."
    assert "Error[epic_hip_set_occupancy_region_gpu]: " + route % "epic_hip_set_occupancy_region_cpu" in err
    assert "Error[epic_hip_timed_occupancy_region_gpu]: " + route % "epic_hip_set_occupancy_region_cpu" in err
    assert "Error[epic_hip_reset_free_cells_3d_gpu]: " + route % "epic_hip_reset_free_cells_3d_cpu" in err
    # the route the message names works, and gives what one device gives
    plain(h, 7)
    field = readback(h)                              # the host arrays now hold what the devices hold
    assert E.epic_hip_set_occupancy_region_cpu(h, occ[1:3, 1:3, 1:3].copy().ctypes.data, R.uints((1, 1, 1)), R.uints((2, 2, 2)), 50, -2, 0, None) == 0
    assert E.harmonic_update_model_gpu(h) == 0
    plain(h, 10)
    got = readback(h)
    fini(h)
    env(EPIC_HIP_DEVICES=None)
    g = make(m, u0, l0)
    plain(g, 10)
    assert same(readback(g), field)
    assert region_gpu(g, occ[1:3, 1:3, 1:3], (1, 1, 1), (2, 2, 2), **C.NODE) == 8 - int(l0.reshape(m)[1:3, 1:3, 1:3].sum())
    plain(g, 10)
    assert same(readback(g), got)
    fini(g)


# ---- 13. errors on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [[5, 7], [4, 5, 7]], ids=R.ident)
def test_error_returns(m, capfd):
    u0, l0, _ = start_state(m)
    occ = np.full(int(np.prod(m)) + 64, 100, dtype=np.int8)             # every byte an obstacle: a call that went on would show
    changed, ms = ct.c_ulonglong(777), ct.c_float(-1.0)

    def expect(fn, *args):
        capfd.readouterr()
        assert fn(*args) == eh.EPIC_ERROR_INVALID_DATA
        assert "Error[%s]: Invalid data." % fn.__name__ in capfd.readouterr().err
        assert changed.value == 777

    rule = (50, -2, 0, ct.byref(changed))
    h = make(m, u0, l0)
    plain(h, 3)
    field = readback(h)
    for origin, extent in R.bad_regions(m):
        o = R.uints(origin) if origin is not None else None
        e = R.uints(extent) if extent is not None else None
        expect(E.epic_hip_set_occupancy_region_gpu, h, occ.ctypes.data, o, e, *rule)
        expect(E.epic_hip_timed_occupancy_region_gpu, h, occ.ctypes.data, o, e, *rule, ct.byref(ms))
    expect(E.epic_hip_set_occupancy_region_gpu, h, None, None, None, *rule)                     # null occ
    expect(E.epic_hip_timed_occupancy_region_gpu, h, occ.ctypes.data, None, None, *rule, None)  # null kernel_ms
    expect(E.epic_hip_set_occupancy_region_gpu, None, occ.ctypes.data, None, None, *rule)
    if len(m) == 2:
        expect(E.epic_hip_reset_free_cells_3d_gpu, h)                   # the 3-D reset on a 2-D field
    assert same(readback(h), field) and ms.value == -1.0
    assert E.epic_hip_set_occupancy_region_gpu(h, occ.ctypes.data, None, None, 50, -2, 0, None) == 0     # changed == NULL
    assert not same(readback(h), field)
    fini(h)
    bare = make(m, u0, l0, init=False)                                  # no device state
    expect(E.epic_hip_set_occupancy_region_gpu, bare, occ.ctypes.data, None, None, *rule)
    expect(E.epic_hip_timed_occupancy_region_gpu, bare, occ.ctypes.data, None, None, *rule, ct.byref(ms))
    expect(E.epic_hip_reset_free_cells_3d_gpu, bare)
    m4 = [3, 3, 3, 4]                                                   # n == 4: the state is resident, nothing edits it
    h4 = make(m4, np.zeros(108, dtype=np.float32), np.zeros(108, dtype=np.uint32))
    expect(E.epic_hip_set_occupancy_region_gpu, h4, occ.ctypes.data, None, None, *rule)
    expect(E.epic_hip_reset_free_cells_3d_gpu, h4)
    fini(h4)


# ---- 14. the Python class ---------------------------------------------------------------------------------------------
def test_python_both_on_a_3d_grid():
    m = [6, 7, 300]
    u0, l0, full = start_state(m)
    h = make(m, u0, l0)
    check(h)
    plain(h, 5)
    resident = readback(h)                          # the host arrays now hold what the device holds
    origin, extent = R.boxes_3d(m)["fours"]
    occ = R.cut(full, origin, extent)
    changed = h.set_occupancy(occ, process='both', origin=origin)
    assert changed == R.rule_nd(m, full, R.inside(m, origin, extent), resident, l0, **C.NODE)[2] > 0
    host_u, host_l = h.u_array().ravel().copy(), h.locked_array().ravel().copy()
    assert same(readback(h), host_u)                # the same edit on both sides
    assert h.set_occupancy(full, process='both') == R.rule_nd(m, full, np.ones(m, dtype=bool), host_u, host_l, **C.NODE)[2] > 0
    host_u, host_l = h.u_array().ravel().copy(), h.locked_array().ravel().copy()
    assert same(readback(h), host_u)
    p = O.Problem(m, host_u, host_l)                # the host's state, relaxed by the checker: the device's lock state must be the host's
    p.h.currentIteration = h.currentIteration
    plain(h, 4)
    O.run_session(p, 4)
    after = readback(h)
    assert same(after, p.u)
    h.reset_free_cells(process='both')
    host_u = h.u_array().ravel().copy()
    inner = np.zeros(m, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    free = inner.ravel() & (host_l == 0)
    assert free.any() and np.all(host_u[free] == np.float32(-1e6)) and same(readback(h), host_u)
    fini(h)
