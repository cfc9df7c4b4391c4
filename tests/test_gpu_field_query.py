"""Queries of the device-resident field (include/epic_hip.h, "Field queries"; epic_amd/csrc/field_query.hip, field_query_driver.hip):
epic_hip_sample_potential_gpu, epic_hip_sample_gradient_gpu and epic_hip_flow_field_gpu against their host twins
(epic_amd/csrc/field_query_cpu.cpp), epic_hip_get_cells_gpu and epic_hip_get_region_gpu against slices of the host arrays -- byte for
byte, values and statuses.  The grids, points and regions are those of tests/test_field_query_cpu.py (tests/field_query_cases.py);
the field is relaxed on the device to 1e-4 and read back, so the host arrays are the resident field."""
import ctypes as ct
import os

import numpy as np
import pytest

import field_query_cases as C
from epic_amd import epic_harmonic as eh
from field_query_cases import E, OK, bits
from test_gpu_field3d import NT, gpu_fini, gpu_init, relax_on_device

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

INVALID_DATA, INVALID_LOCATION_RC = 2, 10
DEVICE_OUT = eh.EPIC_HIP_QUERY_DEVICE_OUT
SENTINEL = np.float32(-7.5)
IDS = lambda m: "x".join(map(str, m))   # noqa: E731


@pytest.fixture(scope="module", params=list(C.GRIDS), ids=IDS)
def resident(request):
    m = request.param
    u0, l0, _ = C.initial(m)
    h = C.make(m, u0, l0)
    gpu_init(h)
    relax_on_device(h)
    yield h
    gpu_fini(h)


def same(a, b):
    """(rc, values, statuses) of two calls agree byte for byte"""
    return a[0] == b[0] == 0 and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def all_points(m):
    return np.ascontiguousarray(np.concatenate([C.points(m), C.edge_points(m)]))


# ---- point samples ---------------------------------------------------------------------------------------------------
def test_samples_equal_the_twins(resident):
    h = resident
    pts = all_points(h.shape)
    want = C.sample_potential(h, pts, 'cpu')
    got = C.sample_potential(h, pts, 'gpu')
    assert same(got, want), np.flatnonzero((bits(got[1]) != bits(want[1])) | (got[2] != want[2]))[:8]
    counts = {"potential": np.bincount(want[2], minlength=4).tolist()}
    for cd in C.CDS + (1.5,):
        want = C.sample_gradient(h, pts, cd, 'cpu')
        got = C.sample_gradient(h, pts, cd, 'gpu')
        bad = np.flatnonzero((bits(got[1]).reshape(len(pts), -1) != bits(want[1]).reshape(len(pts), -1)).any(axis=1) | (got[2] != want[2]))
        assert same(got, want), (cd, bad[:8], pts[bad[:8]])
        counts[cd] = np.bincount(want[2], minlength=4).tolist()
        assert (want[2][-len(C.edge_points(h.shape)):] != OK).all()
    print("grid %s statuses [OK, location, gradient, flat]: %s" % (h.shape, counts))
    assert counts[0.5][OK] >= 0.4 * len(C.points(h.shape))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_batch_sizes(resident, n):
    h = resident
    base = all_points(h.shape)
    pts = np.ascontiguousarray(np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n])
    assert same(C.sample_potential(h, pts, 'gpu'), C.sample_potential(h, pts, 'cpu'))
    assert same(C.sample_gradient(h, pts, 0.3, 'gpu'), C.sample_gradient(h, pts, 0.3, 'cpu'))


def test_status_may_be_null_and_a_count_of_zero_touches_nothing(resident):
    h = resident
    pts = all_points(h.shape)[:300]
    for status in (True, False):
        assert same(C.sample_potential(h, pts, 'gpu', status), C.sample_potential(h, pts, 'cpu', status))
        assert same(C.sample_gradient(h, pts, 0.5, 'gpu', status), C.sample_gradient(h, pts, 0.5, 'cpu', status))
    rc, v, st = C.sample_potential(h, pts, 'gpu', status=False)
    assert (st == 99).all()
    out = np.full(8, SENTINEL)
    assert E.epic_hip_sample_potential_gpu(h, 0, pts.ctypes.data, out.ctypes.data, None) == 0
    assert E.epic_hip_sample_gradient_gpu(h, 0, pts.ctypes.data, 0.5, out.ctypes.data, None) == 0
    assert E.epic_hip_get_cells_gpu(h, 0, pts.ctypes.data, out.ctypes.data, out.ctypes.data) == 0
    assert (out == SENTINEL).all()


# ---- flow fields and read-backs of regions ----------------------------------------------------------------------------
def test_flow_field_equals_the_twin_on_every_region(resident):
    h = resident
    for cd in (0.5, 0.3):
        for origin, extent in C.regions(h.shape):
            want = C.flow_field(h, origin, extent, cd, 'cpu')
            got = C.flow_field(h, origin, extent, cd, 'gpu')
            assert same(got, want), (cd, origin, extent, np.argwhere(got[2] != want[2])[:8])
            bare = C.flow_field(h, origin, extent, cd, 'gpu', status=False)
            assert bare[0] == 0 and np.array_equal(bits(bare[1]), bits(want[1])) and (bare[2] == 99).all()
    st = C.flow_field(h, None, None, 0.5, 'gpu')[2]
    print("grid %s flow field statuses: %s" % (h.shape, np.bincount(st.ravel(), minlength=4).tolist()))
    assert len(np.unique(st)) == 4


def get_region(h, origin, extent, want_u=True, want_locked=True):
    m = h.shape
    o, e, keep = C.region_args(origin, extent)
    shape = tuple(extent) if extent is not None else m
    u = np.full(shape, SENTINEL, dtype=np.float32)
    lk = np.full(shape, 77, dtype=np.uint32)
    rc = E.epic_hip_get_region_gpu(h, o, e, 0, u.ctypes.data if want_u else None, lk.ctypes.data if want_locked else None)
    return rc, u, lk


def test_get_region_and_get_cells_equal_the_host_arrays(resident):
    h = resident
    m = h.shape
    U, L = h.u_array(), h.locked_array()
    for origin, extent in C.regions(m):
        sl = C.region_slices(m, origin, extent)
        rc, u, lk = get_region(h, origin, extent)
        assert rc == 0 and np.array_equal(bits(u), bits(U[sl])) and np.array_equal(lk, L[sl]), (origin, extent)
        rc, u, lk = get_region(h, origin, extent, want_locked=False)
        assert rc == 0 and np.array_equal(bits(u), bits(U[sl])) and (lk == 77).all()
        rc, u, lk = get_region(h, origin, extent, want_u=False)
        assert rc == 0 and np.array_equal(lk, L[sl]) and (u == SENTINEL).all()
        assert get_region(h, origin, extent, False, False)[0] == INVALID_DATA
    rng = np.random.default_rng(3)
    for k in (1, 65, 3000):
        v = np.ascontiguousarray(np.stack([rng.integers(0, d, k) for d in m[::-1]], axis=1).astype(np.uint32))
        u = np.full(k, SENTINEL, dtype=np.float32)
        lk = np.full(k, 77, dtype=np.uint32)
        assert E.epic_hip_get_cells_gpu(h, k, v.ctypes.data, u.ctypes.data, lk.ctypes.data) == 0
        idx = tuple(v[:, ::-1].T.astype(np.int64))
        assert np.array_equal(bits(u), bits(U[idx])) and np.array_equal(lk, L[idx])
        for ax in range(len(m)):   # one entry outside the grid: the code, and nothing is touched
            bad = v.copy()
            bad[k // 2, ax] = m[::-1][ax]
            u[:], lk[:] = SENTINEL, 77
            assert E.epic_hip_get_cells_gpu(h, k, bad.ctypes.data, u.ctypes.data, lk.ctypes.data) == INVALID_LOCATION_RC
            assert (u == SENTINEL).all() and (lk == 77).all()
    pu, pl = h.get_cells(v[:10])
    assert np.array_equal(bits(pu), bits(U[idx][:10])) and np.array_equal(pl, L[idx][:10])


# ---- device output -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_floats,pad_bytes", [(2, 4), (1, 1)], ids=["aligned", "unaligned"])
def test_device_output_equals_host_output_and_writes_nothing_else(resident, pad_floats, pad_bytes):
    """The kernels write into torch tensors pre-filled with a sentinel, at an offset inside a larger allocation: the region's
    elements equal the host-output call's, every other element keeps the sentinel.  Aligned: the outputs start on 8 / 4 bytes (one
    dwordx2 per cell, packed status dwords where the width allows); unaligned: they do not."""
    import torch

    h = resident
    m, n = h.shape, len(h.shape)
    dev = torch.device("cuda", 0)
    for origin, extent in C.regions(m):
        shape = tuple(extent) if extent is not None else m
        cells = int(np.prod(shape))
        o, e, keep = C.region_args(origin, extent)
        want = C.flow_field(h, origin, extent, 0.3, 'gpu')
        g = torch.full((cells * n + 2 * pad_floats + 6,), float(SENTINEL), dtype=torch.float32, device=dev)
        s = torch.full((cells + 2 * pad_bytes + 6,), 99, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rc = E.epic_hip_flow_field_gpu(h, o, e, 0.3, DEVICE_OUT, g.data_ptr() + 4 * pad_floats, s.data_ptr() + pad_bytes)
        assert rc == 0
        gh, sh = g.cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(bits(gh[pad_floats:pad_floats + cells * n]), bits(want[1])), (origin, extent)
        assert np.array_equal(sh[pad_bytes:pad_bytes + cells], want[2].ravel()), (origin, extent)
        assert (gh[:pad_floats] == SENTINEL).all() and (gh[pad_floats + cells * n:] == SENTINEL).all()
        assert (sh[:pad_bytes] == 99).all() and (sh[pad_bytes + cells:] == 99).all()
        # the read-back of the region, both outputs and one at a time
        sl = C.region_slices(m, origin, extent)
        u = torch.full((cells + 2 * pad_floats,), float(SENTINEL), dtype=torch.float32, device=dev)
        lk = torch.full((cells + 2 * pad_floats,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert E.epic_hip_get_region_gpu(h, o, e, DEVICE_OUT, u.data_ptr() + 4 * pad_floats, lk.data_ptr() + 4 * pad_floats) == 0
        uh, lh = u.cpu().numpy(), lk.cpu().numpy()
        assert np.array_equal(bits(uh[pad_floats:pad_floats + cells]), bits(h.u_array()[sl]))
        assert np.array_equal(lh[pad_floats:pad_floats + cells].astype(np.uint32), h.locked_array()[sl].ravel())
        assert (uh[:pad_floats] == SENTINEL).all() and (uh[pad_floats + cells:] == SENTINEL).all()
        assert (lh[:pad_floats] == 77).all() and (lh[pad_floats + cells:] == 77).all()
        lk.fill_(77)
        torch.cuda.synchronize()
        assert E.epic_hip_get_region_gpu(h, o, e, DEVICE_OUT, None, lk.data_ptr() + 4 * pad_floats) == 0
        assert np.array_equal(lk.cpu().numpy(), lh)
    big = np.zeros(int(np.prod(m)) * n, dtype=np.float32)
    assert E.epic_hip_flow_field_gpu(h, None, None, 0.5, 2, big.ctypes.data, None) == INVALID_DATA   # an unknown flag


def test_python_surface(resident):
    import torch

    h = resident
    m, n = h.shape, len(h.shape)
    pts = C.points(m)[:100]
    g, st = h.gradient_at(pts, 0.5)
    assert g.shape == (100, n) and g.dtype == np.float32 and st.shape == (100,) and st.dtype == np.uint8
    assert same((0, g, st), C.sample_gradient(h, pts, 0.5, 'cpu'))
    v, st = h.potential_at(pts)
    assert v.shape == (100,) and same((0, v, st), C.sample_potential(h, pts, 'cpu'))
    origin, extent = C.regions(m)[4]
    for o, e, shape in ((None, None, tuple(m)), (origin, extent, tuple(extent))):
        g, st = h.flow_field(0.5, o, e)
        assert g.shape == shape + (n,) and st.shape == shape and same((0, g, st), C.flow_field(h, o, e, 0.5, 'cpu'))
        u, lk = h.get_region(o, e)
        sl = C.region_slices(m, o, e)
        assert u.shape == shape and lk.shape == shape and lk.dtype == np.uint32
        assert np.array_equal(bits(u), bits(h.u_array()[sl])) and np.array_equal(lk, h.locked_array()[sl])
        dev = torch.device("cuda", 0)
        tg = torch.zeros(shape + (n,), dtype=torch.float32, device=dev)
        ts = torch.zeros(shape, dtype=torch.uint8, device=dev)
        rg, rs = h.flow_field(0.5, o, e, out=(tg, ts))
        assert rg is tg and rs is ts and same((0, tg.cpu().numpy(), ts.cpu().numpy()), (0, g, st))
        tu = torch.zeros(shape, dtype=torch.float32, device=dev)
        tl = torch.zeros(shape, dtype=torch.int32, device=dev)
        h.get_region(o, e, out=(tu, tl))
        assert np.array_equal(bits(tu.cpu().numpy()), bits(u)) and np.array_equal(tl.cpu().numpy().astype(np.uint32), lk)
        with pytest.raises(ValueError):
            h.flow_field(0.5, o, e, out=(torch.zeros(shape, dtype=torch.float32, device=dev), None))


# ---- what is refused ----------------------------------------------------------------------------------------------------
def test_invalid_calls(resident, capfd):
    h = resident
    m, n = h.shape, len(h.shape)
    pts = C.points(m)[:4]
    out = np.full(4 * n, SENTINEL)
    st = np.full(4, 99, dtype=np.uint8)
    args = (pts.ctypes.data, out.ctypes.data, st.ctypes.data)
    assert E.epic_hip_sample_potential_gpu(None, 4, *args) == INVALID_DATA
    assert E.epic_hip_sample_potential_gpu(h, 4, None, out.ctypes.data, None) == INVALID_DATA
    assert E.epic_hip_sample_potential_gpu(h, 4, pts.ctypes.data, None, None) == INVALID_DATA
    assert E.epic_hip_sample_gradient_gpu(h, 4, pts.ctypes.data, 0.5, None, None) == INVALID_DATA
    assert E.epic_hip_flow_field_gpu(h, None, None, 0.5, 0, None, None) == INVALID_DATA
    assert E.epic_hip_get_cells_gpu(h, 4, None, out.ctypes.data, out.ctypes.data) == INVALID_DATA
    assert E.epic_hip_get_cells_gpu(h, 4, pts.ctypes.data, None, out.ctypes.data) == INVALID_DATA
    big = np.zeros(int(np.prod(m)) * n, dtype=np.float32)
    for origin, extent in (((0,) * n, None), ((0,) * n, (0,) * n), ((1,) * n, tuple(m)), (tuple(m), (1,) * n)):
        o = np.array(origin, dtype=np.uint32)
        e = np.array(extent, dtype=np.uint32) if extent is not None else None
        eptr = e.ctypes.data_as(C.UP) if e is not None else None
        assert E.epic_hip_flow_field_gpu(h, o.ctypes.data_as(C.UP), eptr, 0.5, 0, big.ctypes.data, None) == INVALID_DATA
        assert E.epic_hip_get_region_gpu(h, o.ctypes.data_as(C.UP), eptr, 0, big.ctypes.data, None) == INVALID_DATA
    # a context that is not initialised: what epic_hip_compute_paths_2d_gpu returns in that state
    u0, l0, _ = C.initial(m)
    cold = C.make(m, u0, l0)
    assert E.epic_hip_sample_potential_gpu(cold, 4, *args) == INVALID_DATA
    assert E.epic_hip_flow_field_gpu(cold, None, None, 0.5, 0, big.ctypes.data, None) == INVALID_DATA
    assert E.epic_hip_get_region_gpu(cold, None, None, 0, big.ctypes.data, None) == INVALID_DATA
    assert (out == SENTINEL).all() and (st == 99).all()
    capfd.readouterr()


# ---- several devices ------------------------------------------------------------------------------------------------
@pytest.fixture
def env():
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))
        assert E.epic_hip_config_reload(None) == 0

    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    E.epic_hip_config_reload(None)


@pytest.mark.parametrize("m", list(C.GRIDS), ids=IDS)
def test_multi_device_mode_equals_one_device(m, env, capfd):
    """EPIC_HIP_DEVICES=0,0 and 0,0,0 -- rows of a 2-D grid, planes of a 3-D one, in slabs on one GPU: all five calls answer from a
    snapshot of the slabs and equal the single-device answers byte for byte."""
    u0, l0, _ = C.initial(m)
    pts = all_points(m)[::7]
    regs = C.regions(m)[1:5]
    rng = np.random.default_rng(4)
    v = np.ascontiguousarray(np.stack([rng.integers(0, d, 200) for d in m[::-1]], axis=1).astype(np.uint32))

    def answers(devices):
        env(EPIC_HIP_DEVICES=devices)
        h = C.make(m, u0, l0)
        gpu_init(h)
        slabs = len(devices.split(",")) if devices else 1
        assert E.epic_hip_device_layout(h, 0, None, None, None, None) == (slabs if m[0] // slabs >= 4 else 1)
        assert E.epic_hip_update_n_gpu(h, 60, 0) == 0
        for _ in range(3):
            assert E.harmonic_update_gpu(h, NT) == 0   # left pending: the query flushes them
        out = [C.sample_potential(h, pts, 'gpu'), C.sample_gradient(h, pts, 0.3, 'gpu')]
        for origin, extent in regs:
            out.append(C.flow_field(h, origin, extent, 0.5, 'gpu'))
            out.append(get_region(h, origin, extent))
        u, lk = np.zeros(len(v), dtype=np.float32), np.zeros(len(v), dtype=np.uint32)
        out.append((E.epic_hip_get_cells_gpu(h, len(v), v.ctypes.data, u.ctypes.data, lk.ctypes.data), u, lk))
        if slabs > 1 and E.epic_hip_device_layout(h, 0, None, None, None, None) > 1:
            big = np.zeros(int(np.prod(m)) * len(m), dtype=np.float32)
            assert E.epic_hip_flow_field_gpu(h, None, None, 0.5, DEVICE_OUT, big.ctypes.data, None) == INVALID_DATA
            assert E.epic_hip_get_region_gpu(h, None, None, DEVICE_OUT, big.ctypes.data, None) == INVALID_DATA
        assert E.harmonic_get_potential_values_gpu(h) == 0 and h.currentIteration == 63
        twin = C.sample_gradient(h, pts, 0.3, 'cpu')
        gpu_fini(h)
        return out, twin

    one, twin = answers(None)
    assert same(one[1], twin)
    for devices in ("0,0", "0,0,0"):
        many, _ = answers(devices)
        for i, (a, b) in enumerate(zip(many, one)):
            assert same(a, b), (devices, i)
    capfd.readouterr()
