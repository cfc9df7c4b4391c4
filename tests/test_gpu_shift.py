"""epic_hip_shift_field_gpu (include/epic_hip.h; epic_amd/csrc/field_shift.hip, field_shift_driver.hip) against its host twin, bit for bit, in
every state the solver leaves: the resident values and lock bits straight after the call (epic_hip_get_region_gpu), and the field, delta and
currentIteration after 7 more iterations and a check against a FRESH context uploaded from the twin's arrays with the same currentIteration.
(37, 300) crosses a 256-column strip (pitch 512); (34, 9, 260) does so in 3-D and keeps two columns under a shift of 256."""
import ctypes as ct

import numpy as np
import pytest

from epic_amd import epic_harmonic as eh
from test_gpu_field3d import NT, gpu_fini, gpu_init
from test_shift_cpu import BAD, FREE, OBSTACLE, E, bits, call, make, seeded_field, shifts_for

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

PRECISE, TOL, JACOBI, REDBLACK = eh.MATH_PRECISE, eh.MATH_TOL, eh.SCHEME_JACOBI, eh.SCHEME_REDBLACK
STATES = {   # (math, scheme, tracking, iterations before the shift, asked for one harmonic_update_gpu at a time)
    "fresh": (PRECISE, JACOBI, 0, 0, False),
    "jacobi-odd": (PRECISE, JACOBI, 0, 3, False),      # the field is in buf[1]
    "jacobi-even": (PRECISE, JACOBI, 0, 4, False),
    "redblack": (PRECISE, REDBLACK, 0, 3, False),
    "tol": (TOL, JACOBI, 0, 3, False),
    "tracked": (PRECISE, JACOBI, 1, 5, False),
    "pending": (PRECISE, REDBLACK, 0, 3, True),        # the calls only count: the shift has to flush them first
}


def resident(m, u, locked, state, iteration=0, advance=False):
    """A context holding (u, locked) at `iteration` in the state's modes; advance: the state's iterations are run (or counted)"""
    math, scheme, track, pre, single = STATES[state]
    h = make(m, u, locked)
    gpu_init(h)
    assert E.epic_hip_set_math_mode(h, math) == 0 and E.epic_hip_set_scheme(h, scheme) == 0 and E.epic_hip_set_activity_tracking(h, track) == 0
    h.currentIteration = iteration
    for _ in range(pre if advance and single else 0):
        assert E.harmonic_update_gpu(h, NT) == 0
    assert not (advance and pre and not single) or E.epic_hip_update_n_gpu(h, pre, 0) == 0
    return h


def region(h):   # values and lock bits (0 / 1) of the whole grid as the device holds them
    u, locked = np.zeros(int(np.prod(h.shape)), dtype=np.float32), np.zeros(int(np.prod(h.shape)), dtype=np.uint32)
    assert E.epic_hip_get_region_gpu(h, None, None, 0, u.ctypes.data, locked.ctypes.data) == 0
    return bits(u), locked


def seven_and_a_check(h):
    assert E.epic_hip_update_n_gpu(h, 8, 1) in (0, 1) and E.harmonic_get_potential_values_gpu(h) == 0
    got = bits(h.u_array()).copy(), float(h.delta), int(h.currentIteration)
    gpu_fini(h)
    return got


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("m", [(37, 300), (5, 5), (6, 7, 70), (34, 9, 260)], ids=lambda m: "x".join(map(str, m)))
def test_shift_gpu_equals_the_twin_and_a_fresh_context(m, state):
    u0, l0 = seeded_field(m)
    before = resident(m, u0, l0, state, advance=True)   # the state's field, once: what every shift below starts from
    assert E.harmonic_get_potential_values_gpu(before) == 0
    u_pre, it_pre = before.u_array().ravel().copy(), int(before.currentIteration)
    gpu_fini(before)
    moved = 0
    for i, shift in enumerate(shifts_for(m)):
        for fill in ((FREE, OBSTACLE) if state == "fresh" else (FREE,) if i % 2 else (OBSTACLE,)):
            twin = make(m, u_pre, l0)
            want_kept = call(E.epic_hip_shift_field_cpu, twin, shift, fill)[1]
            want_u, want_l = twin.u_array().ravel().copy(), twin.locked_array().ravel().copy()
            h, ms = resident(m, u0, l0, state, advance=True), ct.c_float(-1.0)
            assert call(E.epic_hip_shift_field_gpu, h, shift, fill, ct.byref(ms)) == (0, want_kept), (shift, fill)
            assert (ms.value > 0.0) == any(shift) and h.currentIteration == it_pre, (shift, ms.value)
            got_u, got_l = region(h)
            assert np.array_equal(got_u, bits(want_u)) and np.array_equal(got_l, (want_l != 0).astype(np.uint32)), (shift, fill)
            got, want = seven_and_a_check(h), seven_and_a_check(resident(m, want_u, want_l, state, it_pre))
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (shift, fill, got[1:], want[1:])
            moved += int((got[0] != bits(want_u)).sum())
    assert moved > 0                                    # the iterations after the shift did something


def test_a_zero_shift_leaves_the_work_lists_alone():
    h = resident((37, 300), *seeded_field((37, 300)), "tracked")
    assert E.epic_hip_update_n_gpu(h, 6, 1) in (0, 1)
    seen = []
    for _ in range(2):
        a, d, t = ct.c_ulonglong(0), ct.c_ulonglong(0), ct.c_ulonglong(0)
        assert E.epic_hip_activity_stats2(h, ct.byref(a), ct.byref(d), ct.byref(t)) == 0
        seen.append((a.value, d.value, t.value, region(h)[0].tobytes(), region(h)[1].tobytes()))
        assert call(E.epic_hip_shift_field_gpu, h, (0, 0), FREE, None) == (0, 35 * 298)
    print("tiles due %d of %d" % seen[0][1:3])
    assert seen[0] == seen[1]
    gpu_fini(h)


def test_invalid_calls_and_the_multi_device_mode_change_nothing(capfd, monkeypatch):
    m = (12, 7, 70)                                     # twelve planes: two slabs in the multi-device mode
    u0, l0 = seeded_field(m)
    h = make(m, u0, l0)
    assert call(E.epic_hip_shift_field_gpu, h, (1, 1, 1), FREE, None) == (BAD, 777)   # no device state
    gpu_init(h)
    was = region(h)
    for who, shift, fill in [(None, (1, 1, 1), FREE), (h, None, FREE), (h, (1, 1, 1), eh.EPIC_CELL_TYPE_GOAL), (h, (1, 1, 1), 3)]:
        assert call(E.epic_hip_shift_field_gpu, who, shift, fill, None) == (BAD, 777)
    assert all(np.array_equal(a, b) for a, b in zip(region(h), was))
    gpu_fini(h)
    capfd.readouterr()
    monkeypatch.setenv("EPIC_HIP_DEVICES", "0,0")
    try:
        assert E.epic_hip_config_reload(None) == 0
        multi, ms = make(m, u0, l0), ct.c_float(-1.0)
        gpu_init(multi)
        assert E.epic_hip_device_layout(multi, 0, None, None, None, None) == 2
        assert call(E.epic_hip_shift_field_gpu, multi, (1, 1, 1), FREE, ct.byref(ms)) == (BAD, 777) and ms.value == 0.0
        assert "epic_hip_shift_field_cpu and harmonic_update_model_gpu" in capfd.readouterr().err
        assert E.harmonic_get_potential_values_gpu(multi) == 0 and np.array_equal(bits(multi.u_array()), bits(u0))
        gpu_fini(multi)
    finally:
        monkeypatch.delenv("EPIC_HIP_DEVICES")
        E.epic_hip_config_reload(None)
