"""One application of the cell update, u' = ln((1 / 2n) sum e^(u_i)), against the EXACT value -- the checker's two arithmetics.  No GPU.

Every other test of an arithmetic here compares two implementations of one rounding sequence.  An error they share (a wrong hi / lo
split of log2 e, a polynomial coefficient one ulp off, a wrong ln 6) passes all of them, and a relaxation amplifies a systematic
error of the update by the square of the domain's radius (epic_amd/csrc/cell_update.h).  tests/update_accuracy_cases.py builds
fields in which every sample has a neighbourhood of its own, in regimes chosen for where the arithmetic can go wrong, and states the
exact value in 80-bit longdouble; errors are counted in f32 spacings at max(|t|, |u'|), t = u' + ln 2n.

What is asserted, per regime, 2-D and 3-D:
  * PINS: the statistics of oracle_jacobi_run (the reference's rounding sequence) and oracle_tol_run (the tol arithmetic) are the
    ones recorded in tests/golden/update_accuracy.json (tests/golden/generate_update_accuracy.py), to 1e-12: the arithmetic is
    deterministic.  A change of either arithmetic shows here first, with the regime it moved.
  * CONDITIONS that do not depend on the pins -- what a CHANGED tol arithmetic has to meet to be acceptable, in seconds:
      - max |err| of tol <= max |err| of the reference arithmetic + max_excess_margin.  The margin exists because tol's terms carry
        the split's error (< 1 ulp, tests/test_tol_checker.py) where the reference's carry expf's 0.502; its value is the largest
        excess measured on the checker over all regimes (1.125 units, one dominant neighbour with the others within 2e-6 of it),
        rounded up to the next half unit: 1.5.
      - |mean (tol - reference)| < 0.1 units: the project's own number -- a bias of 0.1 ulp (v_exp_f32) is what moved the converged
        basic.png by 2e-5, out of the 1e-5 bar (cell_update.h).  Largest measured: 0.039 (3-D, lesser neighbours 15-18 below).
      - |mean err| of tol - |mean err| of the reference <= the recorded excess of the regime + 5 standard errors of the paired mean.
      - a cell whose neighbours are all at the seed keeps the seed's bits; a front cell (one reached neighbour) is within one unit
        of mx - ln 2n.
  * where the reference's own CPU build is present (oracle/_ref): harmonic_update_cpu, one call per colour, leaves the bits of
    oracle_jacobi_run at the samples -- the "reference" column is the reference's, on inputs it was never compared on.

Sensitivity (measured on scratch copies of oracle/tol_checker.c, not committed): the last coefficient of the split's polynomial one
f32 ulp up (0x1.62e43p-1f -> 0x1.62e432p-1f) and the TOL_LL correction of log2 e dropped each fail the pins AND the third condition;
the figures are in DESIGN.md section 2.
"""
import ctypes as ct
import importlib.util
import os

import numpy as np
import pytest

import _oracle as O
import update_accuracy_cases as C

if not C.longdouble_is_80_bit():
    pytest.skip("numpy.longdouble has fewer than 64 significand bits here: no exact values", allow_module_level=True)

IDS = ["%dd-%s" % c for c in C.CASES]


@pytest.fixture(scope="module")
def golden():
    return C.golden()


@pytest.mark.parametrize("dim,name", C.CASES, ids=IDS)
def test_checker_update_against_exact(dim, name, golden):
    c = C.case(dim, name)
    pins = golden["regimes"]["%dd/%s" % (dim, name)]
    assert c.sha256 == pins["sha256"], "the regime's input field is not the one the golden was generated from"
    ref, tol = c.checker("ref"), c.checker("tol")
    rec = c.measure(ref, tol)
    print("\n" + C.HEADER)
    print(C.table_row(c.name, "ref", rec["ref"]))
    print(C.table_row("", "tol", rec["tol"], rec["paired"]))
    bad = C.failed_conditions(c, ref, tol, rec, pins, golden["max_excess_margin"])
    assert not bad, "conditions: " + "; ".join(bad)
    bad = C.pin_mismatches(rec, pins)
    assert not bad, "pins: " + "; ".join(bad)


def test_margin_is_the_largest_excess_rounded_up_to_a_half_unit(golden):
    worst = max(r["max_excess"] for r in golden["regimes"].values())
    assert golden["max_excess_margin"] == C.half_unit_up(worst) and worst == golden["max_excess_largest"]["value"]
    assert sorted(golden["regimes"]) == sorted("%dd/%s" % c for c in C.CASES)


def test_generator_reproduces_the_golden_byte_for_byte(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("generate_update_accuracy",
                                                  os.path.join(O.ROOT, "tests", "golden", "generate_update_accuracy.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = os.path.join(tmp_path, "update_accuracy.json")
    gen.main(out)
    capsys.readouterr()
    assert open(out, "rb").read() == open(C.GOLDEN, "rb").read()


@pytest.mark.parametrize("dim", [2, 3])
def test_exact_values_against_mpmath(dim):
    """The longdouble statement against 100-bit arithmetic, 2000 samples per regime, to 1e-17 relative (to max(|t|, |u'|), the
    magnitude the unit is taken at): 1e-10 of a unit."""
    pytest.importorskip("mpmath")
    for name in C.NAMES:
        c = C.case(dim, name)
        worst = C.mp_cross_check(c.nb, c.exact)
        assert worst <= 1e-17, (name, worst)


@pytest.mark.parametrize("dim,name", C.CASES, ids=IDS)
def test_reference_build_leaves_the_checkers_bits(dim, name):
    ref = O.ref()
    if ref is None:
        pytest.skip("oracle/_ref/libepic_ref.so absent: the reference's own CPU build exists only where its sources do")
    c = C.case(dim, name)
    want = c.checker("ref")
    got = np.empty_like(want)
    seen = np.zeros(want.size, dtype=bool)
    for parity in (0, 1):     # one call per colour, each on the regime's field: a sample's neighbours are of the other colour
        p = O.Problem(c.m, c.u0, c.locked)
        p.h.currentIteration = parity
        assert ref.harmonic_update_cpu(ct.byref(p.h)) == 0
        sel = C.updated_by(dim, parity)
        got[sel] = p.u[c.idx][sel]
        assert np.array_equal(p.u[c.idx][~sel], c.u0[c.idx][~sel]), "the other colour's samples are untouched"
        seen |= sel
    assert seen.all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
