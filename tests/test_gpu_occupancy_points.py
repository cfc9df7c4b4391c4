"""epic_hip_set_occupancy_points_gpu (include/epic_hip.h; epic_amd/csrc/occupancy_points.hip, occupancy_driver.hip) against its CPU twin, bit
for bit: the resident state read back (epic_hip_get_region_gpu), *changed, and the field a solve reaches from either.  Widths across the
64-cell words of the bit planes, windows off the word grid, 0 / 1 / 65 / 5000 points, the points of occupancy_points_cases.cloud."""
import ctypes as ct

import numpy as np
import pytest

import occupancy_points_cases as P
from epic_amd import epic_harmonic as eh
from test_gpu_occupancy_region import fini, make   # a context on the device and its release

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E, I = eh._epic, P.I


def device(geom, points, sensor, r2, rule=None, state=None, solve=False, init=True, **kw):
    """(u, locked, changed) as the device holds them after the _gpu call, kernel_ms, and the solved field"""
    m = P.box(geom)[0]
    h, ms, cells = make(m, *(state or I.state(m)), eps=1e-2, init=init), ct.c_float(-1.0), int(np.prod(m))
    changed = P.points_cpu(h, geom, points, sensor, r2=r2, **(rule or {}), fn=E.epic_hip_set_occupancy_points_gpu, tail=(ct.byref(ms),), **kw)
    u, locked, field = np.empty(cells, dtype=np.float32), np.empty(cells, dtype=np.uint32), None
    if init:
        assert E.epic_hip_get_region_gpu(h, None, None, 0, u.ctypes.data, locked.ctypes.data) == 0
        if solve:   # harmonic_execute_gpu initialises and releases the solver's state itself, around the device arrays that stay
            assert E.harmonic_uninitialize_gpu(h) == 0 and E.harmonic_execute_gpu(h, 1024) == 0 and E.harmonic_initialize_gpu(h, 1024) == 0
            field = h.u_array().ravel().copy()
        fini(h)
    return (u, locked, changed), ms.value, field


@pytest.mark.parametrize("sensor", P.SENSORS)
@pytest.mark.parametrize("geom", P.GEOMS)
def test_points_gpu_equals_the_twin(geom, sensor):
    points, s = P.cloud(geom, 65, sensor)
    for r2, rule in P.RULES:
        got, ms, _ = device(geom, points, s, r2, rule)
        assert I.same(got, P.twin(geom, points, s, r2, rule)) and ms > 0.0, (r2, rule)


@pytest.mark.parametrize("sensor", ["none", "corner"])
@pytest.mark.parametrize("count", [0, 1, 65, 5000])
@pytest.mark.parametrize("geom", ["2d-129", "3d-129"])
def test_point_counts_and_the_solve_afterwards(geom, count, sensor):
    points, s = P.cloud(geom, count, sensor)
    want = P.twin(geom, points, s, 1, P.C.NODE)
    got, _, field = device(geom, points, s, 1, P.C.NODE, solve=count < 5000)
    assert I.same(got, want) and (count > 0 or want[2] == 0)
    if count == 5000:   # three rows of obstacles wall the goal in: that solve takes its whole iteration budget, 16 s
        return
    solved = device(geom, None, None, 0, P.C.NODE, state=want[:2], solve=True, count=0)[2]   # the twin's arrays on the device, no points
    assert np.array_equal(field.view(np.uint32), solved.view(np.uint32))


@pytest.mark.parametrize("bad", list(P.bad_calls("2d-65")) + ["no-device-state"])
@pytest.mark.parametrize("geom", ["2d-65", "3d-65"])
def test_invalid_arguments_touch_nothing(geom, bad, capfd):
    args = P.bad_calls(geom).get(bad) or dict(P.bad_calls(geom)["radius"], r2=1)
    got, ms, _ = device(geom, **args, init=bad != "no-device-state", expect=eh.EPIC_ERROR_INVALID_DATA)
    assert "Error[epic_hip_set_occupancy_points_gpu]: Invalid data." in capfd.readouterr().err and got[2] == 777 and ms == -1.0
    assert bad == "no-device-state" or I.same(got, I.state(P.box(geom)[0]) + (777,))


def test_python_set_points():
    m, o, e, _ = P.box("3d-65")
    points, s = P.cloud("3d-65", 65, "corner")
    h, u, locked = make(m, *I.state(m)), np.empty(int(np.prod(m)), dtype=np.float32), np.empty(int(np.prod(m)), dtype=np.uint32)
    changed = h.set_points(points, sensor=s, origin=o, extent=e, inflate_sq=1)
    assert E.epic_hip_get_region_gpu(h, None, None, 0, u.ctypes.data, locked.ctypes.data) == 0
    fini(h)
    assert I.same((u, locked, changed), P.twin("3d-65", points, s, 1, P.C.NODE))
