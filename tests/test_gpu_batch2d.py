"""Batched 2-D relaxation: several fields per launch on shared LDS tiles (epic_amd/csrc/kernels_tile2d_batch.hip, batch2d_driver.hip).

Every field of a batch call must end as its own single call would leave it, and with the library's defaults that is
harmonic_complete_cpu -- the reference's CPU solver -- bit for bit: field, iteration count, delta.  Everything at tolerance 0.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic, solve_batch
from epic_amd.synthetic import synthetic_grid
from test_gpu_tile import env, seeded

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

E = eh._epic
NT = 1024
EPS = (1e-2, 1e-3, 1e-4)
INIT = (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu)
UNINIT = (E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu, E.harmonic_uninitialize_locked_gpu)
# (obstacle densities at which no pocket of free cells is cut off from every goal: such a pocket drains by ln 4 per iteration from its
#  scrambled start down to -1e6, a million iterations of the reference's loop)
GRIDS = {"23x37": ([23, 37], 4, 0.10, None), "70x66": ([70, 66], 8, 0.10, None), "150x203": ([150, 203], 21, 0.08, None),
         "130x256wide": ([130, 256], 11, 0.05, 128)}


def field(m, u0, locked, eps, stagger=10):
    h = Harmonic()
    h.set_grid(m, u0, locked)
    h.epsilon, h.numIterationsToStaggerCheck = eps, stagger
    return h


def grid_field(grid, i):
    """Field i on a grid: its own obstacle seed, its own goals, a non-uniform start; the epsilons dealt in turn."""
    m, seed, dens, _ = GRIDS[grid]
    return field(m, *seeded(m, seed + 7 * i, dens), EPS[i % 3])


@functools.lru_cache(maxsize=None)
def cpu_result(grid, i):
    h = grid_field(grid, i)
    assert E.harmonic_complete_cpu(h) == 0
    return h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta)


def resident(h, math=eh.MATH_PRECISE, scheme=eh.SCHEME_REDBLACK):
    for fn in INIT:
        assert fn(h) == 0
    assert E.epic_hip_set_math_mode(h, math) == 0 and E.epic_hip_set_scheme(h, scheme) == 0
    return h


def execute_batch(fields, expect=0):
    codes = (ct.c_int * len(fields))()
    assert E.epic_hip_execute_batch_gpu(eh.field_array(fields), len(fields), NT, codes) == expect
    for h in fields:
        for fn in UNINIT:
            fn(h)
    return list(codes)


def same(h, want):
    u, iterations, delta = want
    assert h.currentIteration == iterations and float(h.delta) == delta
    assert np.array_equal(h.u_array().ravel(), u), int((h.u_array().ravel() != u).sum())
    assert not h.d_u and not h.d_locked and not h.d_m and not h.d_delta


# (F = 0: the plan's choice; the wide tile holds two fields at the most, so it has no F = 4 case)
@pytest.mark.parametrize("grid,B,F", [(g, B, F) for g in GRIDS for B in (1, 2, 3, 5, 9) for F in (0, 1, 2, 4) if not (GRIDS[g][3] == 128 and F == 4)])
def test_batch_equals_the_cpu_solver(grid, B, F):
    with env(EPIC_HIP_BATCH_FIELDS=F or None, EPIC_HIP_BATCH_WIDTH=GRIDS[grid][3]):
        fields = [resident(grid_field(grid, i)) for i in range(B)]
        plan = eh.batch_plan(fields)
        assert plan["batched"] == (B if B >= 2 else 0), plan
        if B >= 2:
            width = plan["tile_cols"] + 2 * plan["halo"]
            assert width == (GRIDS[grid][3] or width) and plan["fields_per_workgroup"] == (F or plan["fields_per_workgroup"])
        assert execute_batch(fields) == [0] * B
    for i, h in enumerate(fields):
        same(h, cpu_result(grid, i))


@pytest.mark.parametrize("halo,tile_rows", [(1, 0), (3, 0), (8, 48), (10, 20), (16, 32), (27, 10)])
def test_any_geometry_gives_the_same_bits(halo, tile_rows):
    """Ring depth 1, below, at and above the checking period of 10, tile heights that leave a ragged last tile row: the bits of the
    per-field loop (EPIC_HIP_BATCH=0)."""
    got = {}
    for knobs in (dict(EPIC_HIP_BATCH="0"), dict(EPIC_HIP_BATCH_HALO=halo, EPIC_HIP_BATCH_ROWS=tile_rows or None, EPIC_HIP_BATCH_WIDTH=64)):
        with env(**knobs):
            fields = [resident(grid_field("150x203", i)) for i in range(5)]
            assert eh.batch_plan(fields)["batched"] == (0 if "EPIC_HIP_BATCH" in knobs else 5)
            assert execute_batch(fields) == [0] * 5
        got[len(knobs)] = [(h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta)) for h in fields]
    for i, h in enumerate(fields):
        same(h, got[1][i])
        same(h, cpu_result("150x203", i))


def test_edges_of_the_stop_rule():
    """Converged at the first check (no free cell next to a goal) yet run to max(m); every cell locked; thousands of iterations."""
    m = [150, 203]
    u0, locked = synthetic_grid(m, 3, 0.0)
    walled = locked.reshape(m).copy()
    walled[74:77, 100:103] = 1      # the goal (the centre cell) behind obstacles: nothing next to it moves, delta is 0 from the first check on
    fields = [field(m, u0, walled, 1e-3), field(m, u0, np.ones_like(locked), 1e-3), grid_field("150x203", 6)]
    want = []
    for h in fields:
        ref = field(m, h.u_array().copy(), h.locked_array().copy(), h.epsilon)
        assert E.harmonic_complete_cpu(ref) == 0
        want.append((ref.u_array().ravel().copy(), int(ref.currentIteration), float(ref.delta)))
    assert want[0][1] >= 200 and want[0][2] == 0.0 and want[2][1] > 2000
    assert eh.batch_plan([resident(h) for h in fields])["batched"] == 3
    assert execute_batch(fields) == [0, 0, 0]
    for h, w in zip(fields, want):
        same(h, w)


def test_mixed_batch():
    """tol, Jacobi, 3-D, another shape and three default fields in one call: each as its own harmonic_complete_gpu leaves it."""
    modes = [(eh.MATH_TOL, eh.SCHEME_REDBLACK), (eh.MATH_PRECISE, eh.SCHEME_JACOBI)] + [(eh.MATH_PRECISE, eh.SCHEME_REDBLACK)] * 5

    def make():
        return [grid_field("70x66", 0), grid_field("70x66", 1), field([16, 16, 16], *synthetic_grid([16, 16, 16], 2, 0.05), 1e-3),
                grid_field("23x37", 0)] + [grid_field("70x66", i) for i in (2, 3, 4)]

    alone = make()
    for h, (math, scheme) in zip(alone, modes):
        resident(h, math, scheme)
        assert E.harmonic_execute_gpu(h, NT) == 0
        for fn in UNINIT:
            assert fn(h) == 0
    fields = [resident(h, *mode) for h, mode in zip(make(), modes)]
    assert eh.batch_plan(fields)["batched"] == 3
    assert execute_batch(fields) == [0] * 7
    for h, a in zip(fields, alone):
        same(h, (a.u_array().ravel(), int(a.currentIteration), float(a.delta)))


def test_validation(capfd):
    fields = [resident(grid_field("23x37", i)) for i in range(3)]
    arr = eh.field_array(fields)
    assert E.epic_hip_execute_batch_gpu(None, 3, NT, None) == eh.EPIC_ERROR_INVALID_DATA
    assert E.epic_hip_execute_batch_gpu(arr, 0, NT, None) == eh.EPIC_ERROR_INVALID_DATA
    assert E.epic_hip_execute_batch_gpu(eh.field_array([fields[0], fields[1], fields[0]]), 3, NT, None) == eh.EPIC_ERROR_INVALID_DATA
    assert E.epic_hip_execute_batch_gpu(arr, 3, 1000, None) == eh.EPIC_ERROR_INVALID_CUDA_PARAM
    err = capfd.readouterr().err
    assert err.count("Error[epic_hip_execute_batch_gpu]: Invalid data") == 3 and "divisible by 32" in err
    assert all(h.currentIteration == 0 for h in fields)   # nothing ran
    fields[1].epsilon = 0.0
    assert execute_batch(fields, expect=eh.EPIC_ERROR_INVALID_DATA) == [0, eh.EPIC_ERROR_INVALID_DATA, 0]
    same(fields[0], cpu_result("23x37", 0))
    same(fields[2], cpu_result("23x37", 2))
    assert execute_batch([resident(grid_field("23x37", 0)), None], expect=eh.EPIC_ERROR_INVALID_DATA) == [0, eh.EPIC_ERROR_INVALID_DATA]


def test_solve_batch():
    fields = [grid_field("70x66", i) for i in range(3)]
    with env(EPIC_HIP_SCHEME=None, EPIC_HIP_MATH=None):
        wall, cpu = solve_batch(fields, epsilon=[EPS[i % 3] for i in range(3)])
        assert wall > 0.0
        for i, h in enumerate(fields):
            same(h, cpu_result("70x66", i))
        fields[1].numIterationsToStaggerCheck = 0
        with pytest.raises(RuntimeError, match="field 1 of the batch failed with code 2"):
            solve_batch(fields, epsilon=1e-2)
    assert not fields[1].d_u and not fields[1].d_m
