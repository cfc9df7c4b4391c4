"""Small 3-D grids: several iterations per launch on LDS bricks (epic_amd/csrc/kernels_brick3d.hip).

The bricks' arithmetic is the per-iteration kernels', so everything here is held at tolerance 0: against the checker (oracle/) and
against the per-iteration kernels (EPIC_HIP_BRICK=0).  The tests force the path on every grid with EPIC_HIP_BRICK_MAX_CELLS.
"""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from test_gpu_tile import MODES, env, seeded

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

E = eh._epic
NT = 1024
UP = ct.POINTER(ct.c_uint)
ON = dict(EPIC_HIP_BRICK=None, EPIC_HIP_BRICK_MAX_CELLS=1 << 40)
OFF = dict(EPIC_HIP_BRICK="0")


def gpu_open(m, u0, locked, math, scheme, eps=1e-6, stagger=100):
    h = Harmonic()
    h.set_grid(m, u0, locked)
    h.epsilon, h.numIterationsToStaggerCheck = eps, stagger
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0
    assert E.harmonic_initialize_gpu(h, NT) == 0
    assert E.epic_hip_set_math_mode(h, math) == 0 and E.epic_hip_set_scheme(h, scheme) == 0
    return h


def gpu_close(h):
    assert E.harmonic_get_potential_values_gpu(h) == 0
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0
    return h.u_array().ravel().copy(), float(h.delta), int(h.currentIteration)


def run_gpu(m, u0, locked, k, math, scheme, bricks):
    """k iterations as ONE batch (epic_hip_update_n_gpu: k - 1 plain ones and a check): field, delta, iterations per brick launch."""
    h = gpu_open(m, u0, locked, math, scheme)
    halo = E.epic_hip_brick_iterations(h)
    assert (halo > 0) == bricks, (halo, eh.config_dump(h)["path"])
    assert E.epic_hip_update_n_gpu(h, k, 1) in (0, 1) and h.currentIteration == k
    u, delta, _ = gpu_close(h)
    return u, delta, halo


def checker(m, u0, locked, k, math, scheme):
    p = O.Problem(m, u0, locked)
    if math == eh.MATH_TOL:
        assert O.oracle().oracle_tol_run(ct.byref(p.h), k, 1 if scheme == eh.SCHEME_REDBLACK else 0) == 0
    elif scheme == eh.SCHEME_JACOBI:
        assert O.oracle().oracle_jacobi_run(ct.byref(p.h), k) == 0
    else:
        for i in range(k):
            (O.oracle().oracle_update_and_check if i == k - 1 else O.oracle().oracle_update)(ct.byref(p.h))
    return p.u, float(p.h.delta)


# one free cell; two brick columns along x2 with a degenerate x0; one brick without any ghosts; x2 at the lane width and one past it;
# several bricks along x0 and x1 with remainders; ghosts on x1 and x2 only
GRIDS = [([3, 3, 3], 6, 0.0), ([4, 5, 70], 2, 0.0), ([20, 19, 18], 3, 0.08), ([9, 40, 64], 4, 0.05), ([9, 40, 65], 4, 0.05),
         ([34, 33, 30], 5, 0.08), ([7, 70, 66], 7, 0.05)]


@pytest.mark.parametrize("shells", [None, 3])   # the planner's depth (2 on these grids), and an odd one: launches start at either parity
@pytest.mark.parametrize("math,scheme", MODES)
@pytest.mark.parametrize("m,seed,dens", GRIDS)
def test_bricks_against_the_checker(m, seed, dens, math, scheme, shells):
    u0, locked = seeded(m, seed, dens)
    with env(EPIC_HIP_BRICK_HALO=shells, **ON):
        _, _, halo = run_gpu(m, u0, locked, 2, math, scheme, True)
        assert shells is None or halo == shells
        # k - 1 plain iterations and a check: no brick launch at all, a short launch (H >= 3), a full one, a launch boundary, several launches
        for k in (2, halo, halo + 1, halo + 2, 2 * halo + 3):
            got, gdelta, _ = run_gpu(m, u0, locked, k, math, scheme, True)
            want, wdelta = checker(m, u0, locked, k, math, scheme)
            assert np.array_equal(got, want), (m, k, halo, int(np.flatnonzero(got != want)[0]), int((got != want).sum()))
            assert gdelta == wdelta


@pytest.mark.parametrize("math,scheme", MODES)
def test_any_shell_depth_and_brick_shape_gives_the_same_bits(math, scheme):
    m = [26, 37, 70]
    u0, locked = seeded(m, 21, 0.08)
    with env(**OFF):
        want, wdelta, _ = run_gpu(m, u0, locked, 23, math, scheme, False)
    ran = 0
    for halo in (1, 2, 3, 5):
        for dims in ("7x12", "11x16"):
            for graph in (None, "1"):
                with env(EPIC_HIP_BRICK_HALO=halo, EPIC_HIP_BRICK_DIMS=dims, EPIC_HIP_NO_GRAPH=graph, **ON):
                    h = gpu_open(m, u0, locked, math, scheme)
                    fits = E.epic_hip_brick_iterations(h) == halo   # 0: the instantiation cannot hold this brick, or no cell is left to own
                    gpu_close(h)
                    if not fits:
                        continue
                    got, gdelta, _ = run_gpu(m, u0, locked, 23, math, scheme, True)
                assert np.array_equal(got, want), (halo, dims, graph, int((got != want).sum()))
                assert gdelta == wdelta
                ran += 1
    assert ran >= 6   # tol Jacobi holds 88 rows: the small brick up to three shells, with and without the graph


@pytest.mark.parametrize("math,scheme", MODES)
@pytest.mark.parametrize("m,seed", [([24, 24, 24], 9), ([20, 30, 70], 10)])
def test_complete_through_bricks(m, seed, math, scheme):
    u0, locked = seeded(m, seed, 0.05)

    def complete(bricks, **kv):
        with env(EPIC_HIP_JACOBI_CHECKS=None, EPIC_HIP_MATH="tol" if math == eh.MATH_TOL else None,
                 EPIC_HIP_SCHEME="redblack" if scheme == eh.SCHEME_REDBLACK else "jacobi", **kv):
            h = gpu_open(m, u0, locked, math, scheme)
            assert (E.epic_hip_brick_iterations(h) > 0) == bricks
            gpu_close(h)
            h = Harmonic()   # the one-shot call makes its own context from the environment
            h.set_grid(m, u0, locked)
            h.epsilon, h.numIterationsToStaggerCheck = 1e-3, 10
            assert E.harmonic_complete_gpu(h, NT) == 0
            return h.u_array().ravel().copy(), float(h.delta), int(h.currentIteration)

    got = complete(True, **ON)
    if math == eh.MATH_TOL:
        want = complete(False, **OFF)
    else:
        p = O.Problem(m, u0, locked, 1e-3, 10)
        assert (O.oracle().oracle_complete if scheme == eh.SCHEME_REDBLACK else O.oracle().oracle_jacobi_complete)(ct.byref(p.h)) == 0
        want = (p.u, float(p.h.delta), int(p.h.currentIteration))
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (got[1:], want[1:])


@pytest.mark.parametrize("math,scheme", MODES)
def test_the_nodes_tick_with_edits_and_reads_between_rounds(math, scheme):
    m = [24, 24, 24]
    u0, locked = seeded(m, 9, 0.05)
    cells = np.array([[5, 6, 7], [12, 3, 20], [20, 20, 2]], dtype=np.uint32)   # (x, y, z) triples
    types = np.array([eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_CELL_TYPE_GOAL, eh.EPIC_CELL_TYPE_FREE], dtype=np.uint32)
    origin, extent = np.array([2, 3, 1], dtype=np.uint32), np.array([20, 18, 22], dtype=np.uint32)

    def tick(bricks, **kv):
        seen = []
        with env(**kv):
            h = gpu_open(m, u0, locked, math, scheme)
            assert (E.epic_hip_brick_iterations(h) > 0) == bricks
            for rnd in range(3):
                assert E.harmonic_update_and_check_gpu(h, NT) in (0, 1)
                seen.append(float(h.delta))
                for _ in range(9):
                    assert E.harmonic_update_gpu(h, NT) == 0
                assert E.epic_hip_set_cells_3d_gpu(h, 1, cells[rnd:].ctypes.data_as(UP), types[rnd:].ctypes.data_as(UP)) == 0
                box = np.zeros(int(extent.prod()), dtype=np.float32)
                assert E.epic_hip_get_region_gpu(h, origin.ctypes.data_as(UP), extent.ctypes.data_as(UP), 0, box.ctypes.data, None) == 0
                seen.append(box)
            seen.append(gpu_close(h)[0])
        return seen

    for g, w in zip(tick(True, **ON), tick(False, **OFF)):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("why", ["multi-device", "tracking", "2-D", "above the limit"])
def test_where_the_path_is_not_taken(why):
    m = [40, 44] if why == "2-D" else [12, 14, 40]
    u0, locked = seeded(m, 3, 0.05)
    kv = dict(ON)
    if why == "multi-device":
        kv["EPIC_HIP_DEVICES"] = "0,0"
    if why == "tracking":
        kv["EPIC_HIP_TRACK"] = "1"
    if why == "above the limit":
        kv["EPIC_HIP_BRICK_MAX_CELLS"] = 12 * 14 * 40 - 1
    with env(**kv):
        got, gdelta, _ = run_gpu(m, u0, locked, 13, eh.MATH_PRECISE, eh.SCHEME_REDBLACK, False)
    with env(**dict(kv, EPIC_HIP_BRICK="0")):
        want, wdelta, _ = run_gpu(m, u0, locked, 13, eh.MATH_PRECISE, eh.SCHEME_REDBLACK, False)
    assert np.array_equal(got, want) and gdelta == wdelta
