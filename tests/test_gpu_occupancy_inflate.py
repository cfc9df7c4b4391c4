"""epic_hip_set_occupancy_inflated_gpu (include/epic_hip.h; epic_amd/csrc/occupancy_inflate.hip, occupancy_driver.hip): the resident
state read back (epic_hip_get_region_gpu) and *changed against the reference of occupancy_inflate_cases.py -- B' by brute force
through the existing epic_hip_set_occupancy_region_cpu --, bit for bit."""
import ctypes as ct

import numpy as np
import pytest

import occupancy_inflate_cases as I
from epic_amd import epic_harmonic as eh
from test_gpu_occupancy_region import env, fini, make   # noqa: F401  (a context on the device, its release, EPIC_HIP_DEVICES for one test)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

E = eh._epic


def resident(h, changed=0):
    u, locked = np.empty(int(np.prod(h.shape)), dtype=np.float32), np.empty(int(np.prod(h.shape)), dtype=np.uint32)
    assert E.epic_hip_get_region_gpu(h, None, None, 0, u.ctypes.data, locked.ctypes.data) == 0
    return u, locked, changed


def inflated_gpu(h, b, origin, extent, thr, no_change, flags, r2, expect=0):
    changed, ms = ct.c_ulonglong(777), ct.c_float(-1.0)
    o, e = (I.R.uints(origin), I.R.uints(extent)) if origin is not None else (None, None)
    assert E.epic_hip_set_occupancy_inflated_gpu(h, np.ascontiguousarray(b).ctypes.data, o, e, thr, no_change, flags, r2, ct.byref(changed), ct.byref(ms)) == expect
    return resident(h, int(changed.value)), ms.value


@pytest.mark.parametrize("r2", I.RADII)
@pytest.mark.parametrize("pattern", ["marks", "sprinkle"])
@pytest.mark.parametrize("geom", I.GEOMS)
def test_inflated_gpu_equals_the_region_call_on_the_brute_force_block(geom, pattern, r2):
    m, _, _, where = I.region(geom)
    for flavour, (rule, _, _) in I.FLAVOURS.items():
        h = make(m, *I.state(m))
        got, ms = inflated_gpu(h, I.block(geom, pattern, flavour), *where, **rule, r2=r2)
        fini(h)
        assert I.same(got, I.expected(geom, pattern, flavour, r2)) and (ms > 0.0) == (r2 > 0), flavour   # ms: the inflation kernels'; none ran at radius 0


def test_a_radius_past_the_limit_touches_nothing(capfd):
    m, _, _, where = I.region("2d-tiny")
    h = make(m, *I.state(m))
    got, ms = inflated_gpu(h, I.block("2d-tiny", "marks", "node"), *where, **I.C.NODE, r2=257, expect=eh.EPIC_ERROR_INVALID_DATA)
    fini(h)
    assert "Error[epic_hip_set_occupancy_inflated_gpu]: Invalid data." in capfd.readouterr().err and I.same(got, I.state(m) + (777,)) and ms == -1.0


@pytest.mark.parametrize("geom", ["2d-window", "3d-window"])
def test_pending_iterations_are_flushed_first(geom):
    m, _, _, where = I.region(geom)
    b, rule, out = I.block(geom, "sprinkle", "keep"), I.FLAVOURS["keep"][0], []
    for flush in (False, True):
        h = make(m, *I.state(m))
        for _ in range(7):
            assert E.harmonic_update_gpu(h, 1024) == 0
        assert not flush or E.harmonic_get_potential_values_gpu(h) == 0
        out.append(inflated_gpu(h, b, *where, **rule, r2=5)[0])
        fini(h)
    assert I.same(out[0], out[1]) and out[0][2] > 0


def test_two_slabs_2d_equal_one_device_and_3d_names_the_host_route(env, capfd):
    env(EPIC_HIP_DEVICES="0,0")
    for geom in ("2d-window", "3d-window"):
        m, _, _, where = I.region(geom)
        h = make(m, *I.state(m))
        assert E.epic_hip_device_layout(h, 0, None, None, None, None) == 2
        got, ms = inflated_gpu(h, I.block(geom, "sprinkle", "node"), *where, **I.C.NODE, r2=9, expect=0 if geom == "2d-window" else eh.EPIC_ERROR_INVALID_DATA)
        fini(h)
        if geom == "2d-window":
            assert I.same(got, I.expected(geom, "sprinkle", "node", 9)) and ms == 0.0
    assert "inflated_gpu]: Invalid data (not available in multi-device mode: use epic_hip_set_occupancy_inflated_cpu and harmonic_update_model_gpu)." in capfd.readouterr().err
    assert I.same(got, I.state(m) + (777,))


@pytest.mark.parametrize("geom", ["2d-window", "3d-grid"])
def test_python_set_occupancy_inflate_sq(geom):
    m, origin, _, where = I.region(geom)
    h = make(m, *I.state(m))
    changed = h.set_occupancy(I.block(geom, "marks", "node").view(np.int8), process='both', origin=where[0] and origin, inflate_sq=5)
    for got in (resident(h, changed), (h.u_array().ravel(), h.locked_array().ravel(), changed)):
        assert I.same(got, I.expected(geom, "marks", "node", 5)) and changed > 0
    fini(h)
