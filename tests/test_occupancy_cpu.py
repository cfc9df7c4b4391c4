"""epic_hip_set_occupancy_2d_cpu / epic_hip_reset_free_cells_2d_cpu (include/epic_hip.h): a map message's bytes applied to the
host arrays, against the route the reference's callers take -- the literal lists of subOccupancyGrid / srvResetFreeCells
(src/epic_navigation_node_harmonic.cpp:383-426, :582-611) through the checker's oracle_set_cells_2d and, where it was built, the
reference's own harmonic_utilities_set_cells_2d_cpu -- and against setCellsFromCostmap's rule (epic_amd.harmonic_map.grid_from_costmap).
Every comparison is bitwise."""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
import occupancy_cases as C
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.harmonic_map import grid_from_costmap

E = eh._epic
GRIDS = [[3, 5], [5, 257], [37, 301], [48, 300], [130, 515]]


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).ravel().view(np.uint32), np.asarray(b, dtype=np.float32).ravel().view(np.uint32))


def dense_cpu(m, occ, u, locked, thr, no_change, flags, want_changed=True):
    h = Harmonic()
    h.set_grid(m, u, locked)
    changed = ct.c_ulonglong(12345)
    occ = np.ascontiguousarray(occ)
    assert E.epic_hip_set_occupancy_2d_cpu(h, occ.ctypes.data, thr, no_change, flags, ct.byref(changed) if want_changed else None) == 0
    return h.u_array().ravel().copy(), h.locked_array().ravel().copy(), int(changed.value)


@pytest.mark.parametrize("m", GRIDS)
def test_node_rule_equals_the_list_route(m):
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    v, t = C.node_lists(m, occ, u0, l0)
    assert len(t) > 0
    u, l, _ = dense_cpu(m, occ, u0, l0, **C.NODE)
    for lib in ((None, O.ref()) if O.ref() is not None else (None,)):
        ru, rl = C.apply_lists(m, u0, l0, v, t, lib)
        assert same(u, ru) and np.array_equal(l, rl)


@pytest.mark.parametrize("m", GRIDS)
def test_costmap_rule_equals_the_plugins(m):
    u0, l0 = C.previous_state(m)
    cost = C.image(m).view(np.uint8)
    u, l, _ = dense_cpu(m, cost, u0, l0, **C.COSTMAP)
    _, gu, gl = grid_from_costmap(cost)
    inner = np.s_[1:-1, 1:-1]
    assert same(u.reshape(m)[inner], gu[inner]) and np.array_equal(l.reshape(m)[inner], gl[inner])
    v, t = C.costmap_lists(m, cost)
    ru, rl = C.apply_lists(m, u0, l0, v, t)
    assert same(u, ru) and np.array_equal(l, rl)


@pytest.mark.parametrize("m", GRIDS)
@pytest.mark.parametrize("case", ["NODE", "COSTMAP"])
def test_keep_free_keeps_the_bits_of_cells_that_stay_free(m, case):
    kw = dict(getattr(C, case))
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    cold_u, cold_l, _ = dense_cpu(m, occ, u0, l0, **kw)
    kw["flags"] |= C.KEEP
    u, l, _ = dense_cpu(m, occ, u0, l0, **kw)
    stays_free = (l0 == 0) & (cold_l == 0)
    assert same(u[stays_free], u0[stays_free])
    assert same(u[~stays_free], cold_u[~stays_free]) and np.array_equal(l, cold_l)
    if m != [3, 5]:
        assert stays_free.any() and not same(u, cold_u)


@pytest.mark.parametrize("m", GRIDS)
@pytest.mark.parametrize("flags", C.ALL_FLAGS)
def test_changed_and_untouched_cells_under_every_flag_combination(m, flags):
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    for thr, no_change in ((50, -2), (250, -1), (0, 127), (100, 254)):
        u, l, changed = dense_cpu(m, occ, u0, l0, thr, no_change, flags)
        ru, rl, rchanged = C.rule(m, occ, u0, l0, thr, no_change, flags)
        assert same(u, ru) and np.array_equal(l, rl)
        assert changed == rchanged
        # the border and the no_change cells: never modified
        border = np.ones(m, dtype=bool)
        border[1:-1, 1:-1] = False
        v = (occ.view(np.uint8) if flags & C.UNSIGNED else occ).astype(np.int32)
        keep = (border | (v == no_change)).ravel()
        assert same(u[keep], u0[keep]) and np.array_equal(l[keep], l0[keep])
        # changed == NULL is accepted and changes nothing else
        nu, nl, sentinel = dense_cpu(m, occ, u0, l0, thr, no_change, flags, want_changed=False)
        assert same(nu, u) and np.array_equal(nl, l) and sentinel == 12345
    if m == [130, 515]:
        assert changed > 0


@pytest.mark.parametrize("m", GRIDS)
def test_reset_free_cells_equals_the_nodes_list(m):
    u0, l0 = C.previous_state(m)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    assert E.epic_hip_reset_free_cells_2d_cpu(h) == 0
    v, t = C.reset_lists(m, l0)
    ru, rl = C.apply_lists(m, u0, l0, v, t)
    assert same(h.u_array(), ru) and np.array_equal(h.locked_array().ravel(), rl)
    if m != [3, 5]:
        assert not same(ru, u0)


def test_error_returns(capfd):
    m = [5, 7]
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    changed = ct.c_ulonglong(0)

    def expect(fn, *args):
        capfd.readouterr()
        assert fn(*args) == eh.EPIC_ERROR_INVALID_DATA
        assert "Error[%s]: Invalid data." % fn.__name__ in capfd.readouterr().err

    h = Harmonic()
    h.set_grid(m, u0, l0)
    expect(E.epic_hip_set_occupancy_2d_cpu, h, None, 50, -2, 0, ct.byref(changed))        # null occ
    h.m = ct.POINTER(ct.c_uint)()
    expect(E.epic_hip_set_occupancy_2d_cpu, h, occ.ctypes.data, 50, -2, 0, ct.byref(changed))   # null m
    expect(E.epic_hip_reset_free_cells_2d_cpu, h)
    h3 = Harmonic()
    h3.set_grid([3, 5, 7], np.zeros(105, dtype=np.float32), np.ones(105, dtype=np.uint32))
    expect(E.epic_hip_set_occupancy_2d_cpu, h3, np.zeros(105, dtype=np.int8).ctypes.data, 50, -2, 0, ct.byref(changed))   # n = 3
    expect(E.epic_hip_reset_free_cells_2d_cpu, h3)
    expect(E.epic_hip_set_occupancy_2d_cpu, None, occ.ctypes.data, 50, -2, 0, None)
    assert same(h3.u_array(), np.zeros(105))


def test_python_method_returns_the_same_count():
    m = [37, 301]
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    for kw, py in ((C.NODE, dict()), (C.COSTMAP, dict(obstacle_threshold=250, no_change=-1, unsigned=True, over_goals=True)),
                   (dict(C.NODE, flags=C.KEEP), dict(keep_free=True))):
        u, l, changed = dense_cpu(m, occ, u0, l0, **kw)
        h = Harmonic()
        h.set_grid(m, u0, l0)
        img = occ.view(np.uint8) if py.get("unsigned") else occ
        assert h.set_occupancy(img, process='cpu', **py) == changed
        assert same(h.u_array(), u) and np.array_equal(h.locked_array().ravel(), l)
    h.reset_free_cells(process='cpu')
    assert same(h.u_array()[h.locked_array() == 0], np.full(int((l == 0).sum()), -1e6))
    with pytest.raises(ValueError):
        h.set_occupancy(occ, process='tpu')
