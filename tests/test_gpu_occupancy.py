"""epic_hip_set_occupancy_2d_gpu / epic_hip_reset_free_cells_2d_gpu (include/epic_hip.h; epic_amd/csrc/occupancy_2d.hip,
occupancy_driver.hip): a map message's bytes applied to the device-resident state, against the route the reference's callers
take (their literal lists through harmonic_utilities_set_cells_2d_gpu), the checker, and the CPU variant.  Every comparison is
bitwise.  The grids put cells on columns 1 and cols - 2, on the half-word boundary 127 / 128, on the strip boundaries 255 / 256 / 257
and 511 / 512, leave padding beyond cols, and include a single interior row and cols % 4 != 0."""
import ctypes as ct
import os

import numpy as np
import pytest

import _oracle as O
import occupancy_cases as C
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E = eh._epic
NT = 1024
UP = C.UP
GRIDS = [[3, 5], [5, 257], [37, 301], [48, 300], [130, 515], [64, 1024]]
JACOBI, REDBLACK = eh.SCHEME_JACOBI, eh.SCHEME_REDBLACK
MODES = [(JACOBI, 0), (REDBLACK, 1), (JACOBI, 1), (REDBLACK, 0)]   # (epic_hip_set_scheme, epic_hip_set_activity_tracking)


def bits(a):
    return np.asarray(a, dtype=np.float32).ravel().view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def make(m, u, locked, scheme=None, track=None, eps=1e-6, stagger=100, for_execute=False):
    """for_execute: harmonic_execute_gpu brackets itself with harmonic_initialize_gpu / harmonic_uninitialize_gpu."""
    h = Harmonic()
    h.set_grid(m, u, locked)
    h.epsilon = eps
    h.numIterationsToStaggerCheck = stagger
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0
    if not for_execute:
        assert E.harmonic_initialize_gpu(h, NT) == 0
    if scheme is not None:
        assert E.epic_hip_set_scheme(h, scheme) == 0
    if track is not None:
        assert E.epic_hip_set_activity_tracking(h, track) == 0
    return h


def fini(h, for_execute=False):
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu)[1 if for_execute else 0:]:
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


def lists_gpu(h, v, t):
    if len(t):
        assert E.harmonic_utilities_set_cells_2d_gpu(h, NT, len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)) == 0


def dense_gpu(h, occ, thr, no_change, flags):
    occ = np.ascontiguousarray(occ)
    changed = ct.c_ulonglong(54321)
    assert E.epic_hip_set_occupancy_2d_gpu(h, occ.ctypes.data, thr, no_change, flags, ct.byref(changed)) == 0
    return int(changed.value)


def checker_run(p, k, scheme):
    """k iterations of `scheme` on Problem p from p.h.currentIteration on, the last one a check."""
    lib = O.oracle()
    if scheme == JACOBI:
        assert lib.oracle_jacobi_run(ct.byref(p.h), k) == 0
    else:
        for i in range(k):
            (lib.oracle_update_and_check if i == k - 1 else lib.oracle_update)(ct.byref(p.h))


def checker_edit(p, m, occ, thr, no_change, flags):
    """The header's rule (numpy) on the checker's state, in place."""
    u, l, changed = C.rule(m, occ, p.u, p.locked, thr, no_change, flags)
    p.u[:], p.locked[:] = u, l
    return changed


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


def start_state(m):
    return synthetic_with_goals(tuple(m))


_STATES = {}


def synthetic_with_goals(m):
    """(u0, locked), flat: the seeded grid with a few more goals (computed once per grid, never modified)."""
    if m not in _STATES:
        u, l = synthetic_grid(list(m), 5, 0.08)
        for x, y in C.extra_goals(list(m), 5):
            u[y * m[1] + x] = 0.0
            l[y * m[1] + x] = 1
        u.setflags(write=False)
        l.setflags(write=False)
        _STATES[m] = (u, l)
    return _STATES[m]


def list_route_against_dense(m, scheme, track, expect_path=None):
    """Two contexts, one tick (a check and 24 plain updates) each; one gets the callers' lists, the other the image.  Fields after the
    edit, and fields and delta after 60 more iterations ending in a check, are equal -- and equal to the checker's."""
    u0, l0 = start_state(m)
    occ = C.image(m)
    for case in ("node", "costmap"):
        if case == "node":
            kw, img = C.NODE, occ
            v, t = C.node_lists(m, occ, u0, l0)   # the node's goal test reads its host arrays: goals never move
        else:
            kw, img = C.COSTMAP, occ.view(np.uint8)
            v, t = C.costmap_lists(m, img)
        a, b = make(m, u0, l0, scheme, track), make(m, u0, l0, scheme, track)
        if expect_path:
            assert expect_path in eh.config_dump(b)["path"]["plain_batch"], eh.config_dump(b)["path"]["plain_batch"]
        p = O.Problem(m, u0, l0)
        for h in (a, b):
            check(h)
            plain(h, 24)
        checker_run(p, 1, scheme)
        checker_run(p, 24, scheme)
        lists_gpu(a, v, t)
        changed = dense_gpu(b, img, **kw)
        assert changed == checker_edit(p, m, img, **kw)
        ua, ub = readback(a), readback(b)
        assert same(ua, ub) and same(ub, p.u)
        for h in (a, b):
            plain(h, 59)
        da, db = check(a), check(b)
        checker_run(p, 60, scheme)
        ua, ub = readback(a), readback(b)
        assert same(ua, ub) and da == db
        assert same(ub, p.u) and db == float(p.h.delta)
        fini(a)
        fini(b)


@pytest.mark.parametrize("m", GRIDS, ids=lambda m: "%dx%d" % tuple(m))
@pytest.mark.parametrize("scheme,track", MODES)
def test_dense_route_equals_the_list_route_and_the_checker(m, scheme, track):
    list_route_against_dense(m, scheme, track)


def test_fused_pair_family_reads_the_rebuilt_fused_masks(env):
    env(EPIC_HIP_FUSE_MIN_CELLS=0, EPIC_HIP_TILE=0)
    list_route_against_dense([130, 515], REDBLACK, 0, expect_path="fused red-black pairs")


def test_lds_tile_family_reads_the_edited_masks(env):
    env(EPIC_HIP_TILE=None, EPIC_HIP_TILE_MAX_CELLS=None, EPIC_HIP_FUSE_MIN_CELLS=None)
    list_route_against_dense([130, 515], REDBLACK, 0, expect_path="LDS tiles")


@pytest.mark.parametrize("m", GRIDS, ids=lambda m: "%dx%d" % tuple(m))
@pytest.mark.parametrize("case", ["NODE", "COSTMAP"])
def test_keep_free_bits_and_count_equal_the_cpu_variant(m, case):
    kw = dict(getattr(C, case))
    kw["flags"] |= C.KEEP
    u0, l0 = start_state(m)
    occ = C.image(m)
    h = make(m, u0, l0)
    check(h)
    plain(h, 9)
    before = readback(h)            # host u = the device's field; host locked = the device's lock state (nothing edited yet)
    changed = dense_gpu(h, occ, **kw)
    got = readback(h)
    cpu = Harmonic()
    cpu.set_grid(m, before, l0)
    cchanged = ct.c_ulonglong(0)
    assert E.epic_hip_set_occupancy_2d_cpu(cpu, occ.ctypes.data, kw["thr"], kw["no_change"], kw["flags"], ct.byref(cchanged)) == 0
    assert same(got, cpu.u_array()) and changed == int(cchanged.value)
    if m != [3, 5]:
        stays_free = (l0 == 0) & (cpu.locked_array().ravel() == 0)
        assert stays_free.any() and np.any(bits(got[stays_free]) != bits(np.float32(-1e6)))
    # the lock state, seen through the next relaxation: the checker, from the CPU variant's arrays, moves the same cells the same way
    p = O.Problem(m, cpu.u_array(), cpu.locked_array())
    p.h.currentIteration = h.currentIteration
    plain(h, 3)
    O.run_session(p, 3)
    assert same(readback(h), p.u)
    fini(h)


@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK])
def test_keep_free_with_nothing_changed_disturbs_nothing(scheme):
    """The image restates the resident map, part of it as no_change: changed == 0, the work lists are what they were (tiles
    ahead of the front still sleep) and the relaxation goes on bit for bit like one that never got the call."""
    m = [64, 1024]
    u0, l0 = start_state(m)
    occ = C.restating_image(m, u0, l0)
    a, b = make(m, u0, l0, scheme, 1), make(m, u0, l0, scheme, 1)
    stats = []
    for h in (a, b):
        check(h)
        plain(h, 39)
        active, tiles = ct.c_ulonglong(0), ct.c_ulonglong(0)
        assert E.epic_hip_activity_stats(h, ct.byref(active), ct.byref(tiles)) == 0
        stats.append((active.value, tiles.value))
    assert stats[0] == stats[1] and 0 < stats[0][0] < stats[0][1], stats   # some tiles sleep
    assert dense_gpu(b, occ, **dict(C.NODE, flags=C.KEEP)) == 0
    active, tiles = ct.c_ulonglong(0), ct.c_ulonglong(0)
    assert E.epic_hip_activity_stats(b, ct.byref(active), ct.byref(tiles)) == 0
    assert (active.value, tiles.value) == stats[1]
    for h in (a, b):
        plain(h, 30)
    da, db = check(a), check(b)
    assert same(readback(a), readback(b)) and da == db
    # without KEEP_FREE the same image is a cold restart: every tile is woken
    assert dense_gpu(b, occ, **C.NODE) == 0
    assert E.epic_hip_activity_stats(b, ct.byref(active), ct.byref(tiles)) == 0
    assert active.value == tiles.value
    fini(a)
    fini(b)


@pytest.mark.parametrize("defer", [None, "0"])
def test_the_call_is_an_ordering_point(defer, env):
    """7 pending plain updates, the dense call, 13 more, a read-back: 7 checker iterations, the edit, 13 checker iterations.  The same
    right after a harmonic_update_and_check_gpu that followed whole ticks (a block may have been enqueued ahead of the caller)."""
    env(EPIC_HIP_DEFER=defer)
    m = [48, 300]
    u0, l0 = start_state(m)
    occ = C.image(m)
    h = make(m, u0, l0)
    p = O.Problem(m, u0, l0)
    plain(h, 7)
    O.run_session(p, 7)
    assert dense_gpu(h, occ, **C.NODE) == checker_edit(p, m, occ, **C.NODE)
    plain(h, 13)
    O.run_session(p, 13)
    assert same(readback(h), p.u)
    for _ in range(2):                         # whole ticks: the next check may run a block ahead
        d = check(h)
        O.run_session(p, 1)
        assert d == float(p.h.delta)
        plain(h, 16)
        O.run_session(p, 16)
    d = check(h)
    O.run_session(p, 1)
    assert d == float(p.h.delta)
    occ2 = C.image(m, seed=10)
    assert dense_gpu(h, occ2, **dict(C.NODE, flags=C.KEEP)) == checker_edit(p, m, occ2, **dict(C.NODE, flags=C.KEEP))
    plain(h, 13)
    O.run_session(p, 13)
    assert same(readback(h), p.u)
    assert h.currentIteration == 7 + 13 + 2 * 17 + 1 + 13
    fini(h)


def test_warm_start_needs_fewer_iterations_than_the_cold_restart(capsys):
    """64 x 150, 3 % obstacles, one goal at the centre, relaxed to epsilon = 1e-4 with a check every 10 iterations; then a wall of 20
    cells 20 columns beside the goal.  Iterations of the second relaxation, chosen and counted beforehand with the checker
    (oracle_complete / oracle_jacobi_complete on the rule's two results): red-black (library default) cold 1481, warm 1341; Jacobi
    (the suite's default session) cold 1481, warm 1261.  The two fields stop at different distances from the fixed point (checker:
    max |difference| 1.2e-2 red-black, 1.7e-2 Jacobi): no tolerance is put on their difference, it is printed."""
    m, eps, stagger = [64, 150], 1e-4, 10
    u0, l0 = synthetic_grid(m, 21, 0.03)
    wall_x = m[1] // 2 + 20
    occ = np.where(l0.reshape(m) != 0, 100, 0).astype(np.int8)
    occ[m[0] // 2 - 10:m[0] // 2 + 10, wall_x] = 100
    for scheme in (None, REDBLACK):            # the session's scheme and the library default
        fields, counts = {}, {}
        for label, flags in (("cold", 0), ("warm", C.KEEP)):
            h = make(m, u0, l0, scheme, eps=eps, stagger=stagger, for_execute=True)
            assert E.harmonic_execute_gpu(h, NT) == 0
            assert dense_gpu(h, occ, 50, -2, flags) == 20
            assert E.harmonic_execute_gpu(h, NT) == 0
            counts[label] = int(h.currentIteration)
            fields[label] = readback(h)
            k, raw = ct.c_uint(0), ct.POINTER(ct.c_float)()
            assert E.epic_hip_compute_path_2d_gpu(h, float(wall_x + 15), float(m[0] // 2), 0.5, 0.5, 4000, ct.byref(k), ct.byref(raw)) == 0
            assert k.value > 0
            E.harmonic_free_path_cpu(ct.byref(raw))
            fini(h, for_execute=True)
        with capsys.disabled():
            print("\nwarm start %s: cold %d iterations, warm %d, max |cold - warm| %.3e"
                  % ("session scheme" if scheme is None else "red-black", counts["cold"], counts["warm"],
                     float(np.abs(fields["cold"] - fields["warm"]).max())))
        assert counts["warm"] < counts["cold"], counts


@pytest.mark.parametrize("m", GRIDS, ids=lambda m: "%dx%d" % tuple(m))
def test_reset_free_cells_equals_the_list_route(m):
    u0, l0 = start_state(m)
    v, t = C.reset_lists(m, l0)
    a, b = make(m, u0, l0), make(m, u0, l0)
    for h in (a, b):
        check(h)
        plain(h, 11)
    lists_gpu(a, v, t)
    assert E.epic_hip_reset_free_cells_2d_gpu(b) == 0
    ua, ub = readback(a), readback(b)
    assert same(ua, ub) and same(ub[l0 == 0], np.full(int((l0 == 0).sum()), -1e6))
    for h in (a, b):
        plain(h, 20)
    assert same(readback(a), readback(b))
    fini(a)
    fini(b)


def test_multi_device_mode_gives_the_single_device_field(env):
    m = [130, 515]
    u0, l0 = start_state(m)
    occ = C.image(m)
    out = {}
    for devices in (None, "0,0"):
        env(EPIC_HIP_DEVICES=devices)
        h = make(m, u0, l0)
        nslabs = E.epic_hip_device_layout(h, 0, None, None, None, None)
        assert nslabs == (2 if devices else 1)
        check(h)
        plain(h, 24)
        c1 = dense_gpu(h, occ, **C.NODE)
        plain(h, 20)
        c2 = dense_gpu(h, C.image(m, seed=10), **dict(C.NODE, flags=C.KEEP))
        plain(h, 19)
        d = check(h)
        f40 = readback(h)
        assert E.epic_hip_reset_free_cells_2d_gpu(h) == 0
        plain(h, 5)
        out[devices] = (c1, c2, d, f40, readback(h))
        fini(h)
    one, two = out[None], out["0,0"]
    assert one[:3] == two[:3] and one[0] > 0
    assert same(one[3], two[3]) and same(one[4], two[4])


def test_error_returns(capfd):
    occ = np.zeros(105, dtype=np.int8)
    changed = ct.c_ulonglong(0)

    def expect(fn, *args):
        capfd.readouterr()
        assert fn(*args) == eh.EPIC_ERROR_INVALID_DATA
        assert "Error[%s]: Invalid data." % fn.__name__ in capfd.readouterr().err

    m3 = [3, 5, 7]
    u3, l3 = synthetic_grid(m3, 3, 0.05)
    h3 = make(m3, u3, l3)                       # a 3-D context, device state and all
    expect(E.epic_hip_set_occupancy_2d_gpu, h3, occ.ctypes.data, 50, -2, 0, ct.byref(changed))
    expect(E.epic_hip_reset_free_cells_2d_gpu, h3)
    fini(h3)
    m = [5, 21]
    u0, l0 = start_state(m)
    h = Harmonic()
    h.set_grid(m, u0, l0)                       # no device state
    expect(E.epic_hip_set_occupancy_2d_gpu, h, occ.ctypes.data, 50, -2, 0, ct.byref(changed))
    expect(E.epic_hip_reset_free_cells_2d_gpu, h)
    g = make(m, u0, l0)
    expect(E.epic_hip_set_occupancy_2d_gpu, g, None, 50, -2, 0, ct.byref(changed))   # null occ
    assert E.epic_hip_set_occupancy_2d_gpu(g, occ.ctypes.data, 50, -2, 0, None) == 0   # changed == NULL
    fini(g)


def test_python_both_keeps_host_and_device_lock_state_together():
    m = [37, 301]
    u0, l0 = start_state(m)
    occ = C.image(m)
    h = make(m, u0, l0)
    check(h)
    plain(h, 5)
    resident = readback(h)                      # the host arrays now hold what the device holds
    changed = h.set_occupancy(occ, process='both')
    assert changed == C.rule(m, occ, resident, l0, **C.NODE)[2] > 0
    host_u, host_l = h.u_array().ravel().copy(), h.locked_array().ravel().copy()
    assert same(readback(h), host_u)            # same edit on both sides
    p = O.Problem(m, host_u, host_l)            # the host's state, relaxed by the checker: the device's lock state must be the host's
    p.h.currentIteration = h.currentIteration
    plain(h, 4)
    O.run_session(p, 4)
    after = readback(h)
    assert same(after, p.u)
    moved = bits(after) != bits(host_u)
    assert moved.any() and not np.any(moved & (host_l != 0))
    h.reset_free_cells(process='both')
    host_u = h.u_array().ravel().copy()
    assert np.all(host_u[host_l == 0] == np.float32(-1e6)) and same(readback(h), host_u)
    fini(h)


def test_timed_variant_is_the_same_call_with_a_kernel_time():
    m = [37, 301]
    u0, l0 = start_state(m)
    occ = C.image(m)
    a, b = make(m, u0, l0), make(m, u0, l0)
    changed, ms = ct.c_ulonglong(0), ct.c_float(-1.0)
    assert E.epic_hip_timed_occupancy_2d_gpu(b, occ.ctypes.data, 50, -2, 0, ct.byref(changed), ct.byref(ms)) == 0
    assert dense_gpu(a, occ, **C.NODE) == int(changed.value) and 0.0 < ms.value < 1e3
    assert same(readback(a), readback(b))
    assert E.epic_hip_timed_occupancy_2d_gpu(b, occ.ctypes.data, 50, -2, 0, ct.byref(changed), None) == eh.EPIC_ERROR_INVALID_DATA
    fini(a)
    fini(b)
