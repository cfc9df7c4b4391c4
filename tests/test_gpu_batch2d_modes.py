"""Batched 2-D relaxation in the modes beside the default: tol (red-black, Jacobi), precise Jacobi, fast (kernels_tile2d_batch_modes.hip).

Every field of a batch call ends as its own harmonic_execute_gpu leaves it -- host u, currentIteration, delta, return code and
epic_hip_finish_iteration -- at tolerance 0, through every exit a field can take out of its group (converged, the tol mode's finishing
phase, the Jacobi hand-over).  By default these groups start at four fields and the fast arithmetic is off (profiles/batch_2d_modes.txt):
EPIC_HIP_BATCH=1 is the study knob that takes every mode from two fields.
"""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
from epic_amd import epic_harmonic as eh
from test_gpu_batch2d import NT, UNINIT, execute_batch, field, resident
from test_gpu_tile import env, seeded

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

E = eh._epic
MODES = {"tol-redblack": (eh.MATH_TOL, eh.SCHEME_REDBLACK), "tol-jacobi": (eh.MATH_TOL, eh.SCHEME_JACOBI),
         "precise-jacobi": (eh.MATH_PRECISE, eh.SCHEME_JACOBI), "fast-redblack": (eh.MATH_FAST, eh.SCHEME_REDBLACK)}
# shape: (m, fields, checking period) -- smaller than a tile; column seams at 64 and 128; row seams; seams both ways with odd remainders
SHAPES = {"20x23": ([20, 23], 2, 7), "70x150": ([70, 150], 3, 100), "150x70": ([150, 70], 5, 7), "131x259": ([131, 259], 3, 100)}
EPS = (1e-2, 1e-4, 1e-6)


def make(m, B, stagger, eps=EPS):
    """B fields on one seeded grid (2 % obstacles: no closed pocket of free cells), a further goal of its own for each."""
    out = []
    for i in range(B):
        u0, locked = seeded(m, 5, 0.02)
        free = np.flatnonzero(locked == 0)
        g = free[(i + 1) * free.size // (B + 2)]
        u0[g], locked[g] = 0.0, 1
        out.append(field(m, u0, locked, eps[i % len(eps)], stagger))
    return out


def run(fields, mode, batch, plan=None):
    """The fields through one batch call (batch) or each through its own harmonic_execute_gpu: what the caller can see of each afterwards."""
    for h in fields:
        resident(h, *mode)
    if batch:
        got = eh.batch_plan(fields)
        assert got["batched"] == (len(fields) if plan is None else plan), got
        codes = (ct.c_int * len(fields))()
        assert E.epic_hip_execute_batch_gpu(eh.field_array(fields), len(fields), NT, codes) == 0
    else:
        codes = [E.harmonic_execute_gpu(h, NT) for h in fields]
    seen = [(h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta), int(rc), int(E.epic_hip_finish_iteration(h)))
            for h, rc in zip(fields, codes)]
    for h in fields:
        for fn in UNINIT:
            assert fn(h) == 0
    return seen


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[1:] == w[1:], (i, g[1:], w[1:])
        assert np.array_equal(g[0], w[0]), (i, int((g[0] != w[0]).sum()))


def both(mode, m, B, stagger, eps=EPS, **knobs):
    with env(**dict(knobs, EPIC_HIP_BATCH="0")):   # (the product knobs among them hold for both routes)
        alone = run(make(m, B, stagger, eps), mode, False)
    with env(EPIC_HIP_BATCH="1", **knobs):
        same(run(make(m, B, stagger, eps), mode, True), alone)
    return alone


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_the_single_call(mode, shape):
    """Fields of epsilon 1e-2, 1e-4, 1e-6 in one group: they leave at different checks and the plan is made again."""
    alone = both(MODES[mode], *SHAPES[shape])
    assert len({a[1] for a in alone}) > 1   # (not all at the same check)


FORCED = [("EPIC_HIP_BATCH_FIELDS", 1), ("EPIC_HIP_BATCH_FIELDS", 2), ("EPIC_HIP_BATCH_FIELDS", 4), ("EPIC_HIP_BATCH_HALO", 3), ("EPIC_HIP_BATCH_WIDTH", 128)]


@pytest.mark.parametrize("mode,knob,value", [(mo, k, v) for mo in MODES for k, v in FORCED if (mo, v) != ("tol-jacobi", 128)])
def test_forced_plans_give_the_same_bits(mode, knob, value):
    """Fields per workgroup 1, 2, 4 (a mode whose LDS holds fewer takes its largest), a ring shallower than the checking period, the wide
    tile (tol Jacobi has none) on the grid with two column seams; three fields, so the last workgroup has an empty slot."""
    both(MODES[mode], *SHAPES["70x150"], **{knob: value})


def test_tol_exits():
    """One field hands over to the finishing phase at the first check (epsilon 10: iteration 0 moves the scrambled start by less than 100, and
    the check keeps its verdict), one later (iteration 801 by the checker), and fields of epsilon <= 1e-5 under EPIC_HIP_TOL_FINISH=0 never do."""
    m, B, stagger = SHAPES["70x150"]
    alone = both(MODES["tol-redblack"], m, 2, stagger, (10.0, 1e-3))
    assert alone[0][4] == 1 < alone[1][4]
    alone = both(MODES["tol-redblack"], m, 2, stagger, (1e-6, 1e-5), EPIC_HIP_TOL_FINISH="0")
    assert [a[4] for a in alone] == [0, 0]
    both(MODES["tol-jacobi"], m, 3, stagger, (1e-1, 1e-3, 1e-6), EPIC_HIP_TOL_FINISH_FACTOR="30")


def test_jacobi_hand_over():
    """Precise Jacobi to epsilon 1e-6 stagnates on this grid (|u| > 8: the two chains end an ulp apart): the single call hands over to the
    reference's half-sweeps, found with the checker's loop on the CPU -- both fields at the check of iteration 2 900, ending after 3 001 -- and
    the batch's fields do so at the same check.  The checker states the loop: its field, iteration count and delta."""
    m, B, stagger = SHAPES["70x150"]
    alone = both(MODES["precise-jacobi"], m, 2, stagger, (1e-6, 1e-6))
    for p, a in zip(make(m, 2, stagger, (1e-6, 1e-6)), alone):
        q = O.Problem(m, p.u_array(), p.locked_array(), 1e-6, stagger)
        assert O.oracle().oracle_jacobi_complete(ct.byref(q.h)) == 0
        assert a[1:3] == (q.h.currentIteration, q.h.delta) and np.array_equal(a[0], q.u)


def test_reference_checks_equal_the_cpu_solver():
    """EPIC_HIP_JACOBI_CHECKS=reference, precise: harmonic_complete_cpu bit for bit, iteration count included."""
    m, B, stagger = SHAPES["150x70"]
    with env(EPIC_HIP_BATCH="1", EPIC_HIP_JACOBI_CHECKS="reference"):
        got = run(make(m, B, stagger), MODES["precise-jacobi"], True)
    for h, g in zip(make(m, B, stagger), got):
        assert E.harmonic_complete_cpu(h) == 0
        assert g[1:4] == (h.currentIteration, float(h.delta), 0) and np.array_equal(g[0], h.u_array().ravel())


@pytest.mark.parametrize("mode", ["tol-redblack", "tol-jacobi", "precise-jacobi"])
def test_batch_equals_the_cpu_statement_of_the_mode(mode):
    """oracle/tol_checker.c for tol, the Jacobi checker for precise Jacobi (the fast arithmetic has no CPU statement)."""
    m, B, stagger = SHAPES["131x259"]
    with env(EPIC_HIP_BATCH="1"):
        got = run(make(m, B, stagger), MODES[mode], True)
    for h, g in zip(make(m, B, stagger), got):
        q = O.Problem(m, h.u_array(), h.locked_array(), h.epsilon, stagger)
        lib = O.oracle()
        assert (lib.oracle_jacobi_complete(ct.byref(q.h)) if mode == "precise-jacobi" else lib.oracle_tol_complete(ct.byref(q.h), int(MODES[mode][1]))) == 0
        assert g[1:3] == (q.h.currentIteration, q.h.delta) and np.array_equal(g[0], q.u)


def test_plan_counts_groups_of_one_mode():
    m = SHAPES["70x150"][0]
    tol, jac = MODES["tol-redblack"], MODES["precise-jacobi"]

    def planned(modes):
        fields = [resident(h, *mode) for h, mode in zip(make(m, len(modes), 100), modes)]
        n = eh.batch_plan(fields)["batched"]
        assert execute_batch(fields) == [0] * len(fields)
        return n

    with env(EPIC_HIP_BATCH="1"):
        assert planned([tol] * 3) == 3 and planned([jac] * 2) == 2
        assert planned([tol]) == 0 and planned([tol, jac]) == 0         # a lone field of its mode
        assert planned([tol, jac, tol, jac, tol]) == 5                    # two groups in one call
    with env(EPIC_HIP_BATCH="0"):
        assert planned([tol] * 3) == 0
