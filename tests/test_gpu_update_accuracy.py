"""One application of the cell update on the device against the EXACT value: `precise`, `tol` and `fast`, 2-D and 3-D, Jacobi and
red-black, on the designed neighbourhoods of tests/update_accuracy_cases.py (CPU side and the reasons for every bound:
tests/test_update_accuracy_cpu.py).

  * precise and tol: the device's samples are the checker's bits (oracle_jacobi_run / oracle_tol_run) on these fields -- values at
    -9e5, terms in f32's denormals, four equal neighbours, lone reached neighbours: inputs no other test feeds the kernels.  The
    device's output then goes through the same statistics against the exact value and must meet the conditions and the pins of
    tests/golden/update_accuracy.json.  Both follow from bit-identity; they are asserted on their own so that a failure says which
    one broke.
  * red-black: a half-sweep of either colour leaves the checker's bits at the samples of that colour (their neighbours are of the
    other colour, so these are the Jacobi sweep's bits) and every other cell of the field bit-unchanged.
  * fast (v_exp_f32 / v_log_f32) has no CPU twin.  Its max |err| and mean err per regime were measured ONCE on an MI355X and are
    written down below (FAST_MEASURED): the constants come from the code under test, by necessity -- there is nothing else to hold
    it to.  Asserted: max <= measured x 1.5 rounded up to a half unit, |mean - measured| <= 0.05 units.

2-D runs through the raw operators on torch-owned memory (epic_hip_sweep_2d, epic_hip_sweep_rb_2d), 3-D through a context
(epic_hip_set_math_mode, epic_hip_set_scheme, one harmonic_update_gpu, a read-back).  Every test sets the scheme and the arithmetic
it needs, so the file means the same under both EPIC_TEST_SCHEME sessions.  Each test prints its table (pytest -s).
"""
import numpy as np
import pytest

import update_accuracy_cases as C
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

if not C.longdouble_is_80_bit():
    pytest.skip("numpy.longdouble has fewer than 64 significand bits here: no exact values", allow_module_level=True)

E = eh._epic
NT = 1024

# fast: (max |err|, mean err) in units against exact, per regime; one Jacobi sweep.  Measured 2026-10-21 on an MI355X (gfx950) at commit
# 36c651b + this file.  `vs precise`: paired with the device's precise output on the same samples.
FAST_MEASURED = {
    "2d/spread_0.3_0.3": (4.0395, -0.3287),      # rms 0.6977; vs precise: 28.1 % differ, max|d| 4.00, mean d -0.2942
    "2d/spread_0.5_0.001": (3.6668, -0.3229),      # rms 0.9602; vs precise: 22.3 % differ, max|d| 4.00, mean d -0.2699
    "2d/spread_5_0.001": (0.8219, +0.0795),      # rms 0.3081; vs precise: 5.3 % differ, max|d| 1.00, mean d -0.0303
    "2d/spread_5_2": (1.3139, +0.0972),      # rms 0.3522; vs precise: 6.9 % differ, max|d| 2.00, mean d -0.0388
    "2d/spread_40_0.0001": (0.7512, -0.2503),      # rms 0.3954; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/spread_40_10": (1.0710, -0.0938),      # rms 0.3968; vs precise: 0.2 % differ, max|d| 1.00, mean d -0.0003
    "2d/spread_700_0.001": (0.5000, +0.1233),      # rms 0.3054; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/spread_700_50": (0.5481, +0.0372),      # rms 0.1861; vs precise: 0.0 % differ, max|d| 1.00, mean d -0.0000
    "2d/spread_90000_0.01": (0.7493, +0.3678),      # rms 0.4634; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/spread_90000_30": (0.9457, +0.4296),      # rms 0.4665; vs precise: 0.0 % differ, max|d| 1.00, mean d +0.0000
    "2d/spread_900000_1000": (0.6745, +0.1803),      # rms 0.1826; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/dominant_0_2em06": (2.5000, +0.1152),      # rms 0.4140; vs precise: 0.6 % differ, max|d| 2.00, mean d +0.0047
    "2d/dominant_15_18": (1.7542, -0.0540),      # rms 0.3406; vs precise: 0.1 % differ, max|d| 1.00, mean d +0.0014
    "2d/dominant_80_88": (0.4993, +0.0807),      # rms 0.3331; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/dominant_87_104": (0.4993, +0.0811),      # rms 0.3336; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/dominant_103_110": (0.4993, +0.0804),      # rms 0.3331; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/equal": (1.0000, +0.0732),      # rms 0.2714; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/front": (0.4980, +0.1452),      # rms 0.3392; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/seed_only": (0.0000, +0.0000),      # rms 0.0000; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "2d/goal": (3.9201, -0.2543),      # rms 0.8101; vs precise: 39.5 % differ, max|d| 5.00, mean d -0.2470
    "3d/spread_0.3_0.3": (3.1102, -0.5617),      # rms 0.8848; vs precise: 56.0 % differ, max|d| 3.00, mean d -0.5918
    "3d/spread_0.5_0.001": (2.9652, -0.6699),      # rms 0.9468; vs precise: 51.6 % differ, max|d| 4.00, mean d -0.6215
    "3d/spread_5_0.001": (0.9223, -0.0803),      # rms 0.3255; vs precise: 15.5 % differ, max|d| 1.00, mean d -0.1523
    "3d/spread_5_2": (1.4003, +0.0562),      # rms 0.3380; vs precise: 8.3 % differ, max|d| 2.00, mean d -0.0529
    "3d/spread_40_0.0001": (0.5010, -0.0616),      # rms 0.2964; vs precise: 6.3 % differ, max|d| 1.00, mean d -0.0633
    "3d/spread_40_10": (0.7758, +0.0877),      # rms 0.3259; vs precise: 0.3 % differ, max|d| 1.00, mean d -0.0012
    "3d/spread_700_0.001": (0.6666, +0.2487),      # rms 0.3783; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/spread_700_50": (0.6880, +0.1764),      # rms 0.2751; vs precise: 0.0 % differ, max|d| 1.00, mean d +0.0000
    "3d/spread_90000_0.01": (0.8328, +0.3964),      # rms 0.4972; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/spread_90000_30": (0.8452, +0.3280),      # rms 0.3907; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/spread_900000_1000": (0.8303, -0.3325),      # rms 0.3344; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/dominant_0_2em06": (4.5000, -0.0853),      # rms 0.3680; vs precise: 8.8 % differ, max|d| 3.00, mean d -0.0913
    "3d/dominant_15_18": (1.9839, -0.1430),      # rms 0.2802; vs precise: 0.0 % differ, max|d| 1.00, mean d +0.0002
    "3d/dominant_80_88": (0.4949, +0.0253),      # rms 0.1411; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/dominant_87_104": (0.4949, +0.0261),      # rms 0.1428; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/dominant_103_110": (0.4949, +0.0260),      # rms 0.1428; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/equal": (2.0000, -0.0210),      # rms 0.1590; vs precise: 18.9 % differ, max|d| 2.00, mean d -0.1921
    "3d/front": (0.4972, +0.1958),      # rms 0.3185; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/seed_only": (0.0000, +0.0000),      # rms 0.0000; vs precise: 0.0 % differ, max|d| 0.00, mean d +0.0000
    "3d/goal": (3.9691, -0.4358),      # rms 0.8549; vs precise: 38.8 % differ, max|d| 5.00, mean d -0.2694
}


@pytest.fixture(scope="module")
def golden():
    return C.golden()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 2-D: raw operators on torch-owned memory ---------------------------------------------------------------------------------
class Raw2d:
    """The block layout's mask, packed once; one field buffer and one output buffer, reused by every regime."""

    def __init__(self):
        import torch

        self.torch = torch
        m, locked, self.idx, _ = C.layout(2)
        self.rows, self.cols = m
        self.pitch = E.epic_hip_pitch_for_cols(self.cols)
        assert self.pitch >= self.cols and self.pitch % 256 == 0
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream
        d_locked = torch.from_numpy(locked.astype(np.int32)).to(self.dev)
        self.maskw = torch.zeros(E.epic_hip_mask_words_2d(self.rows, self.pitch), dtype=torch.int32, device=self.dev)
        assert E.epic_hip_pack_mask_2d(d_locked.data_ptr(), self.rows, self.cols, self.pitch, 0, 0, self.maskw.data_ptr(),
                                       self.stream) == 0
        self.a = torch.full((self.rows, self.pitch), float(C.SEED_VALUE), dtype=torch.float32, device=self.dev)
        self.b = torch.empty_like(self.a)
        rr = torch.arange(self.rows, device=self.dev)[:, None]
        cc = torch.arange(self.pitch, device=self.dev)[None, :]
        self.odd = ((rr + cc) & 1) == 1
        torch.cuda.synchronize()

    def load(self, c):
        self.a[:, :self.cols] = self.torch.from_numpy(c.u0.reshape(self.rows, self.cols)).to(self.dev)

    def samples(self, t):
        return t[:, :self.cols].cpu().numpy().ravel()[self.idx]

    def jacobi(self, math):
        self.b.copy_(self.a)
        assert E.epic_hip_sweep_2d(self.a.data_ptr(), self.b.data_ptr(), self.maskw.data_ptr(), self.rows, self.pitch, 0, self.rows,
                                   0, math, None, self.stream) == 0
        self.torch.cuda.synchronize()
        return self.samples(self.b)

    def redblack(self, math, parity):
        """One in-place half-sweep of a copy of the field: (the samples, no cell of the other colour changed its bits)."""
        torch = self.torch
        self.b.copy_(self.a)
        assert E.epic_hip_sweep_rb_2d(self.b.data_ptr(), self.maskw.data_ptr(), self.rows, self.pitch, 0, self.rows, 0, math, parity,
                                      None, self.stream) == 0
        torch.cuda.synchronize()
        changed = self.b.view(torch.int32) != self.a.view(torch.int32)
        other = ~self.odd if parity == 0 else self.odd       # iteration parity p recomputes (row + column + p) odd
        return self.samples(self.b), not bool((changed & other).any().item()), bool(changed.any().item())


@pytest.fixture(scope="module")
def raw2d():
    return Raw2d()


def check_against_checker_and_exact(c, outputs, golden, what):
    """outputs: {'ref': samples of the precise run, 'tol': samples of the tol run}."""
    for which in ("ref", "tol"):
        want = c.checker(which)
        differ = np.flatnonzero(bits(outputs[which]) != bits(want))
        assert differ.size == 0, "%s %s: %d samples are not the checker's bits, first %d: device %r checker %r neighbours %r" % (
            what, which, differ.size, differ[0], outputs[which][differ[0]], want[differ[0]], c.nb[differ[0]])
    pins = golden["regimes"]["%dd/%s" % (c.dim, c.name)]
    rec = c.measure(outputs["ref"], outputs["tol"])
    print("\n%s\n%s" % (what, C.HEADER))
    print(C.table_row(c.name, "precise", rec["ref"]))
    print(C.table_row("", "tol", rec["tol"], rec["paired"]))
    bad = C.failed_conditions(c, outputs["ref"], outputs["tol"], rec, pins, golden["max_excess_margin"])
    assert not bad, what + " conditions: " + "; ".join(bad)
    bad = C.pin_mismatches(rec, pins)
    assert not bad, what + " pins: " + "; ".join(bad)


def merge_colours(dim, halves):
    """halves[parity] = samples after the half-sweep of that parity -> every sample from the half-sweep that recomputed it."""
    out = np.empty_like(halves[0])
    for parity in (0, 1):
        sel = C.updated_by(dim, parity)
        out[sel] = halves[parity][sel]
    return out


def check_untouched(c, halves):
    for parity in (0, 1):
        keep = ~C.updated_by(c.dim, parity)
        assert np.array_equal(bits(halves[parity][keep]), bits(c.u0[c.idx][keep])), "samples of the other colour moved"


@pytest.mark.parametrize("name", C.NAMES)
def test_2d_raw_operators_precise_and_tol(name, raw2d, golden):
    c = C.case(2, name)
    raw2d.load(c)
    jac, rb = {}, {}
    for which, math in (("ref", eh.MATH_PRECISE), ("tol", eh.MATH_TOL)):
        jac[which] = raw2d.jacobi(math)
        halves = []
        for parity in (0, 1):
            got, others_kept, any_change = raw2d.redblack(math, parity)
            assert others_kept, "%s parity %d: a cell outside the updated colour changed its bits" % (which, parity)
            assert any_change or name == "seed_only"
            halves.append(got)
        check_untouched(c, halves)
        rb[which] = merge_colours(2, halves)
    check_against_checker_and_exact(c, jac, golden, "2-D epic_hip_sweep_2d")
    check_against_checker_and_exact(c, rb, golden, "2-D epic_hip_sweep_rb_2d, both parities")


def check_fast(c, got, key):
    s = c.stats(got)
    print("\n" + C.HEADER)
    print(C.table_row("%dd/%s" % (c.dim, c.name), "fast", s, c.paired(got, c.checker("ref"))))
    assert key in FAST_MEASURED, "no measured constants for " + key
    mx, mean = FAST_MEASURED[key]
    assert s["max_abs_err"] <= C.half_unit_up(1.5 * mx), (key, s["max_abs_err"], mx)
    assert abs(s["mean_err"] - mean) <= 0.05, (key, s["mean_err"], mean)
    if c.name == "seed_only":
        assert np.array_equal(bits(got), bits(np.full(got.size, C.SEED_VALUE))), "seed-only cells left the seed's bits"


@pytest.mark.parametrize("name", C.NAMES)
def test_2d_raw_operator_fast(name, raw2d):
    c = C.case(2, name)
    raw2d.load(c)
    check_fast(c, raw2d.jacobi(eh.MATH_FAST), "2d/" + name)


# ---- 3-D: through a context -----------------------------------------------------------------------------------------------------
def context_update_3d(c, math, scheme, parity):
    """One harmonic_update_gpu on the regime's field: (the samples, the whole field)."""
    h = Harmonic()
    h.set_grid(c.m, c.u0, c.locked)
    h.epsilon = 1e-6
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0
    try:
        assert E.epic_hip_set_math_mode(h, math) == 0
        assert E.epic_hip_set_scheme(h, eh.SCHEME_JACOBI if scheme == "jacobi" else eh.SCHEME_REDBLACK) == 0
        if parity is not None:
            h.currentIteration = parity      # the colour of a red-black iteration is its number's parity
        assert E.harmonic_update_gpu(h, NT) == 0
        assert E.harmonic_get_potential_values_gpu(h) == 0
    finally:
        for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
                   E.harmonic_uninitialize_locked_gpu):
            assert fn(h) == 0, fn.__name__
    field = h.u_array().ravel().copy()
    return field[c.idx], field


def redblack_3d(c, math):
    """Both colours, each a half-sweep of the regime's field; every cell of the other colour keeps its bits."""
    m = c.m
    colour = (np.indices(m).sum(axis=0) & 1).ravel()
    halves = []
    for parity in (0, 1):
        got, field = context_update_3d(c, math, "redblack", parity)
        changed = bits(field) != bits(c.u0)
        other = ((colour + parity) & 1) == 1            # iteration parity p recomputes (x0 + x1 + x2 + p) even
        assert not (changed & other).any(), "parity %d: a cell outside the updated colour changed its bits" % parity
        assert not (changed & (c.locked != 0)).any()
        halves.append(got)
    check_untouched(c, halves)
    return merge_colours(3, halves)


@pytest.mark.parametrize("name", C.NAMES)
def test_3d_context_precise_and_tol(name, golden):
    c = C.case(3, name)
    jac, rb = {}, {}
    for which, math in (("ref", eh.MATH_PRECISE), ("tol", eh.MATH_TOL)):
        jac[which] = context_update_3d(c, math, "jacobi", None)[0]
        rb[which] = redblack_3d(c, math)
    check_against_checker_and_exact(c, jac, golden, "3-D context, Jacobi")
    check_against_checker_and_exact(c, rb, golden, "3-D context, red-black, both colours")


@pytest.mark.parametrize("name", C.NAMES)
def test_3d_context_fast(name):
    c = C.case(3, name)
    jac = context_update_3d(c, eh.MATH_FAST, "jacobi", None)[0]
    rb = redblack_3d(c, eh.MATH_FAST)
    assert np.array_equal(bits(jac), bits(rb)), "fast: the red-black half-sweeps and the Jacobi sweep disagree at the samples"
    check_fast(c, jac, "3d/" + name)
