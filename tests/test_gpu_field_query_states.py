"""The field queries (include/epic_hip.h, "Field queries") in every state the solver leaves the resident field in -- the states
tests/test_gpu_field_states.py runs the walkers through: Jacobi with the current buffer 0 and 1, red-black, both arithmetics, work
lists off and on, single updates counted and not yet run, after LDS-tile launches and fused pairs, straight after a sparse edit and
after a region of occupancy bytes.  In each state the queries come FIRST; then the field is read back and the host twins say what
they must have been, byte for byte.  And a query leaves no trace: the work lists' counters and a relaxation that continues are what
they are without it."""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
import field_query_cases as C
from epic_amd import epic_harmonic as eh
from field_query_cases import E, bits
from test_gpu_field3d import NT, gpu_fini, gpu_init
from test_gpu_field_query import get_region, same
from test_gpu_field_states import (JACOBI, MATH_IDS, PLAN_RUNS, PLANS, PRECISE, REDBLACK, SCHEME_IDS, TOL, checker_run, plain_batch_path,
                                   set_modes)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

STATE_GRIDS = [(37, 300), (12, 20, 37)]
IDS = lambda m: "x".join(map(str, m))   # noqa: E731


def query_all(h, pts, regs, process):
    out = [C.sample_potential(h, pts, process), C.sample_gradient(h, pts, 0.5, process), C.sample_gradient(h, pts, 0.3, process)]
    for origin, extent in regs:
        out.append(C.flow_field(h, origin, extent, 0.5, process))
    return out


def queries_then_twins(h, pts, regs):
    """The device answers, then the read-back, then the twins on the field that came back; the read-backs of regions against slices"""
    got = query_all(h, pts, regs, 'gpu')
    boxes = [get_region(h, origin, extent) for origin, extent in regs]
    assert E.harmonic_get_potential_values_gpu(h) == 0
    want = query_all(h, pts, regs, 'cpu')
    for i, (a, b) in enumerate(zip(got, want)):
        assert same(a, b), i
    for (origin, extent), (rc, u, lk) in zip(regs, boxes):
        sl = C.region_slices(h.shape, origin, extent)
        assert rc == 0 and np.array_equal(bits(u), bits(h.u_array()[sl])) and np.array_equal(lk, h.locked_array()[sl])
    return got


@pytest.fixture(scope="module", params=STATE_GRIDS, ids=IDS)
def grid(request):
    m = request.param
    u0, l0, _ = C.initial(m)
    return m, u0, l0, np.ascontiguousarray(C.points(m)[::4]), C.regions(m)[1:5]


@pytest.mark.parametrize("pre", [20, 21])
@pytest.mark.parametrize("track", [0, 1])
@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
@pytest.mark.parametrize("math", [PRECISE, TOL], ids=MATH_IDS.get)
def test_queries_with_iterations_still_pending(grid, math, scheme, track, pre):
    """update_n(9) twice, then 2 or 3 single harmonic_update_gpu calls that are only counted: the query flushes them.  Under Jacobi the
    field is in buf[0] after 20 iterations and in buf[1] after 21.  The field that comes back is the checker's after all `pre`
    iterations, and the queries are the twins' on it."""
    m, u0, l0, pts, regs = grid
    p = O.Problem(m, u0, l0, epsilon=1e-4)
    checker_run(p, pre, math, scheme, False)
    h = C.make(m, u0, l0)
    gpu_init(h)
    set_modes(h, math, scheme, track)
    for _ in range(2):
        assert E.epic_hip_update_n_gpu(h, 9, 0) == 0
    for _ in range(pre - 18):
        assert E.harmonic_update_gpu(h, NT) == 0
    got = queries_then_twins(h, pts, regs)
    field, its = h.u_array().copy(), int(h.currentIteration)
    gpu_fini(h)
    assert its == pre and np.array_equal(bits(field), bits(p.u))
    assert (got[1][2] == C.OK).sum() > len(pts) // 4


@pytest.mark.parametrize("plan,k", PLAN_RUNS, ids=["%s-%d" % pk for pk in PLAN_RUNS])
@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
@pytest.mark.parametrize("math", [PRECISE, TOL], ids=MATH_IDS.get)
def test_2d_queries_after_the_solvers_own_passes(math, scheme, plan, k, monkeypatch):
    """k iterations by the LDS tiles (default plan), by the fused pairs / single sweeps (EPIC_HIP_TILE=0, EPIC_HIP_FUSE_MIN_CELLS=0) or
    as single updates left pending: each flips cur or swaps the spare buffer."""
    for var in ("EPIC_HIP_TILE", "EPIC_HIP_FUSE_MIN_CELLS"):
        monkeypatch.delenv(var, raising=False)
    for var, val in PLANS[plan].items():
        monkeypatch.setenv(var, val)
    m = (37, 300)
    u0, l0, _ = C.initial(m)
    h = C.make(m, u0, l0)
    gpu_init(h)
    assert E.epic_hip_config_reload(h) == 0
    set_modes(h, math, scheme)
    assert E.epic_hip_update_n_gpu(h, 40, 0) == 0   # a field with gradients
    path = plain_batch_path(h)
    if plan == "tiles":
        assert path.startswith("LDS tiles")
    elif plan == "fused":
        assert ("fused" in path) if (math == TOL or scheme == REDBLACK) else path.startswith("single sweeps")
    if plan == "singles":
        for _ in range(k):
            assert E.harmonic_update_gpu(h, NT) == 0
    else:
        assert E.epic_hip_update_n_gpu(h, k, 0) == 0
    got = queries_then_twins(h, np.ascontiguousarray(C.points(m)[::4]), C.regions(m)[1:5])
    its = int(h.currentIteration)
    p = O.Problem(m, u0, l0, epsilon=1e-4)
    checker_run(p, 40 + k, math, scheme, False)
    field = h.u_array().copy()
    gpu_fini(h)
    assert its == 40 + k and np.array_equal(bits(field), bits(p.u))
    assert (got[1][2] == C.OK).sum() > 100


def test_queries_straight_after_edits(grid):
    """A sparse edit and a region of occupancy bytes, each applied to the device and to the host arrays, and the queries with no
    iteration in between: the edited u and masks are all that changed."""
    m, u0, l0, pts, regs = grid
    n = len(m)
    h = C.make(m, u0, l0)
    gpu_init(h)
    assert E.epic_hip_update_n_gpu(h, 41, 0) == 0
    assert E.harmonic_get_potential_values_gpu(h) == 0
    before = query_all(h, pts, regs, 'gpu')
    # goals and obstacles at interior cells, a freed obstacle
    L = h.locked_array()
    free = (np.argwhere(L[tuple(slice(2, -2) for _ in m)] == 0) + 2)[::97][:6, ::-1]
    obst = (np.argwhere(L[tuple(slice(2, -2) for _ in m)] != 0) + 2)[:2, ::-1]
    v = np.ascontiguousarray(np.concatenate([free, obst]).astype(np.uint32))
    t = np.array([eh.EPIC_CELL_TYPE_GOAL] * 3 + [eh.EPIC_CELL_TYPE_OBSTACLE] * 3 + [eh.EPIC_CELL_TYPE_FREE] * 2, dtype=np.uint32)
    h.set_cells(v, t, process='both')
    after_cells = query_all(h, pts, regs, 'gpu')
    for i, (a, b) in enumerate(zip(after_cells, query_all(h, pts, regs, 'cpu'))):
        assert same(a, b), i
    rc, u, lk = get_region(h, None, None)
    assert rc == 0 and np.array_equal(bits(u), bits(h.u_array())) and np.array_equal(lk, h.locked_array())
    assert any(not same(a, b) for a, b in zip(before, after_cells))   # the edit mattered
    # a window of occupancy bytes: obstacles on a diagonal band, free elsewhere; cells that stay free keep their value
    origin, extent = regs[3]
    occ = np.zeros(extent, dtype=np.int8)
    idx = np.indices(extent).sum(axis=0)
    occ[idx % 5 == 0] = 100
    h.set_occupancy(occ, keep_free=True, process='both', origin=origin)
    after_occ = query_all(h, pts, regs, 'gpu')
    for i, (a, b) in enumerate(zip(after_occ, query_all(h, pts, regs, 'cpu'))):
        assert same(a, b), i
    rc, u, lk = get_region(h, None, None)
    assert rc == 0 and np.array_equal(bits(u), bits(h.u_array())) and np.array_equal(lk, h.locked_array())
    assert any(not same(a, b) for a, b in zip(after_cells, after_occ))
    gpu_fini(h)


def stats2(h):
    a, d, t = ct.c_ulonglong(0), ct.c_ulonglong(0), ct.c_ulonglong(0)
    assert E.epic_hip_activity_stats2(h, ct.byref(a), ct.byref(d), ct.byref(t)) == 0
    return a.value, d.value, t.value


@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
def test_a_query_leaves_no_trace(grid, scheme):
    """On a tracked, half-relaxed field the counters of epic_hip_activity_stats2 are the same before and after the queries, and the
    relaxation that goes on ends with the bits and the iteration count of one that was never queried."""
    m, u0, l0, pts, regs = grid
    runs = []
    for queried in (False, True):
        h = C.make(m, u0, l0)
        gpu_init(h)
        set_modes(h, PRECISE, scheme, 1)
        assert E.epic_hip_update_n_gpu(h, 30, 0) == 0
        if queried:
            before = stats2(h)
            query_all(h, pts, regs, 'gpu')
            for origin, extent in regs:
                assert get_region(h, origin, extent)[0] == 0
            v = np.zeros((1, len(m)), dtype=np.uint32)
            out = np.zeros(2, dtype=np.float32)
            assert E.epic_hip_get_cells_gpu(h, 1, v.ctypes.data, out.ctypes.data, out[1:].ctypes.data) == 0
            assert stats2(h) == before and before[2] > 0
        for _ in range(400):
            rc = E.epic_hip_update_n_gpu(h, 100, 1)
            assert rc in (0, 1)
            if rc == 1:
                break
        else:
            raise AssertionError("no convergence")
        assert E.harmonic_get_potential_values_gpu(h) == 0
        runs.append((h.u_array().copy(), int(h.currentIteration), float(h.delta)))
        gpu_fini(h)
    (ua, ia, da), (ub, ib, db) = runs
    assert ia == ib and da == db and np.array_equal(bits(ua), bits(ub))
