"""The host twins of the field queries (include/epic_hip.h, "Field queries"; epic_amd/csrc/field_query_cpu.cpp) against the host
functions they restate -- harmonic_compute_potential_2d_cpu / _gradient_2d_cpu (and the compiled reference's, where it is built),
epic_hip_compute_potential_3d_cpu / _gradient_3d_cpu -- in return class and in bits, and against one another: flow field against
point samples, regions against the whole grid, a z-constant 3-D field against the 2-D field it extrudes.  Host code only."""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
import field_query_cases as C
from field_query_cases import E, FLAT, INVALID_GRADIENT, INVALID_LOCATION, OK, bits

F = ct.c_float
INVALID_DATA = 2


@pytest.fixture(scope="module", params=list(C.GRIDS), ids=lambda m: "x".join(map(str, m)))
def case(request):
    """(m, Harmonic, points, twin potential results, {cd: twin gradient results}): computed once per grid"""
    m = request.param
    h = C.host_field(m)
    pts = C.points(m)
    pot = C.sample_potential(h, pts, 'cpu')
    grads = {cd: C.sample_gradient(h, pts, cd, 'cpu') for cd in C.CDS}
    return m, h, pts, pot, grads


def host_functions(h, lib=None):
    """(potential(p) -> (rc, value), gradient(p, cd) -> (rc, components)) of the single-point host functions for h's dimension"""
    n = int(h.n)
    lib = lib or E
    if n == 2:
        fp, fg = lib.harmonic_compute_potential_2d_cpu, lib.harmonic_compute_gradient_2d_cpu
    else:
        fp, fg = lib.epic_hip_compute_potential_3d_cpu, lib.epic_hip_compute_gradient_3d_cpu
    if lib is not E:
        fp.argtypes = (ct.c_void_p,) + (F,) * n + (ct.POINTER(F),)
        fg.argtypes = (ct.c_void_p,) + (F,) * (n + 1) + (ct.POINTER(F),) * n
        fp.restype = fg.restype = ct.c_int
    ref = ct.cast(ct.pointer(h), ct.c_void_p) if lib is not E else h

    def potential(p):
        v = F(-7.5)
        return fp(ref, *[float(c) for c in p], ct.byref(v)), np.float32(v.value)

    def gradient(p, cd):
        g = [F(-7.5) for _ in range(n)]
        return fg(ref, *[float(c) for c in p], cd, *[ct.byref(c) for c in g]), np.array([c.value for c in g], dtype=np.float32)

    return potential, gradient


def check_anchor(h, pts, pot, grads, lib=None):
    potential, gradient = host_functions(h, lib)
    rc, v, st = pot
    assert rc == 0
    for i, p in enumerate(pts):
        hrc, hv = potential(p)
        if hrc == 0:
            assert st[i] == OK and bits(v[i])[0] == bits(hv)[0], (i, p)
        else:
            assert hrc == 10 and st[i] == INVALID_LOCATION and bits(v[i])[0] == 0, (i, p)
    for cd, (rc, g, st) in grads.items():
        assert rc == 0
        for i, p in enumerate(pts):
            hrc, hg = gradient(p, cd)
            if hrc != 0:
                assert hrc == 12 and st[i] == INVALID_GRADIENT and not bits(g[i]).any(), (cd, i, p)
            elif np.isfinite(hg).all():
                assert st[i] == OK and np.array_equal(bits(g[i]), bits(hg)), (cd, i, p, g[i], hg)
            else:   # the host function divided by a norm that is not a positive finite number
                assert st[i] == FLAT and not bits(g[i]).any(), (cd, i, p)


def test_the_comparison_is_not_empty(case):
    m, h, pts, (rc, v, st), grads = case
    dims = np.array(m[::-1], dtype=np.float32)
    assert len(pts) >= 2000 and (pts >= 1.5).all() and (pts <= dims - 2.5).all()
    seen = np.zeros(4, dtype=np.int64)
    seen += np.bincount(st, minlength=4)[:4]
    assert (st == OK).mean() >= 0.4
    for cd, (grc, g, gst) in grads.items():
        assert (gst == OK).mean() >= 0.4, (cd, np.bincount(gst))
        assert min(np.bincount(gst, minlength=4)[[OK, INVALID_GRADIENT, FLAT]]) >= 5, (cd, np.bincount(gst))
        seen += np.bincount(gst, minlength=4)[:4]
    assert seen.min() >= 5, seen
    assert set(np.unique(st)) <= {OK, INVALID_LOCATION}
    free = h.u_array()[h.locked_array() == 0]
    outside = free[free > -1e5]   # the pocket sits at -1e6; the scrambled cells are still rough after a few dozen iterations
    assert len(np.unique(outside)) >= 0.99 * len(outside)


def test_twins_equal_the_host_functions(case, capfd):
    m, h, pts, pot, grads = case
    check_anchor(h, pts, pot, grads)
    ref = O.ref()   # the reference's own 2-D functions, where its sources were there to be compiled
    if len(m) == 2 and ref is not None:
        check_anchor(h, pts, pot, grads, ref)
    capfd.readouterr()   # (the single-point functions report every failing point on stderr)


def test_flow_field_is_the_gradient_at_the_cells_own_points(case):
    m, h, *_ = case
    n = len(m)
    idx = np.indices(m).reshape(n, -1).T[:, ::-1].astype(np.float32)   # every cell as (x, y[, z]), row-major in m
    L, U = h.locked_array().ravel(), h.u_array().ravel()
    unusable = (L == 1) & (U < 0)
    for cd in C.CDS:
        rc, g, st = C.flow_field(h, None, None, cd, 'cpu')
        grc, gg, gst = C.sample_gradient(h, idx, cd, 'cpu')
        assert rc == 0 and grc == 0
        g, st = g.reshape(-1, n), st.ravel()
        assert (st[unusable] == INVALID_LOCATION).all() and not bits(g[unusable]).any()
        assert not (st[~unusable] == INVALID_LOCATION).any()
        assert np.array_equal(st[~unusable], gst[~unusable]) and np.array_equal(bits(g[~unusable]), bits(gg[~unusable]))
        goal = tuple(d // 2 for d in m)
        assert st.reshape(m)[goal] != INVALID_LOCATION
        prc, pv, pst = C.sample_potential(h, idx, 'cpu')   # the cell's own point is where the potential is the cell's value
        assert np.array_equal(bits(pv[~unusable]), bits(U[~unusable])) and (pst[~unusable] == OK).all()
        assert (pst[unusable] == INVALID_LOCATION).all()


def test_a_region_is_a_slice_of_the_grid(case):
    m, h, *_ = case
    for cd in (0.5, 0.3):
        rc, whole, wst = C.flow_field(h, None, None, cd, 'cpu')
        assert rc == 0
        for origin, extent in C.regions(m):
            rc, g, st = C.flow_field(h, origin, extent, cd, 'cpu')
            sl = C.region_slices(m, origin, extent)
            assert rc == 0 and np.array_equal(bits(g), bits(whole[sl])) and np.array_equal(st, wst[sl]), (origin, extent)
            rc, g2, _ = C.flow_field(h, origin, extent, cd, 'cpu', status=False)
            assert rc == 0 and np.array_equal(bits(g2), bits(g))


def test_extrusion_reproduces_the_2d_flow_field():
    m2 = (20, 70)
    h2 = C.host_field(m2)
    planes = 5
    u3 = np.repeat(h2.u_array()[None], planes, axis=0).copy()
    l3 = np.repeat(h2.locked_array()[None], planes, axis=0).copy()
    h3 = C.make((planes,) + m2, u3, l3)
    rc2, g2, st2 = C.flow_field(h2, None, None, 0.5, 'cpu')
    assert rc2 == 0 and (st2 == OK).mean() > 0.4
    for z in (1, 2, 3):
        rc3, g3, st3 = C.flow_field(h3, (z, 0, 0), (1,) + m2, 0.5, 'cpu')
        assert rc3 == 0 and np.array_equal(st3[0], st2)
        assert np.array_equal(bits(g3[0, ..., :2]), bits(g2)) and not bits(g3[0, ..., 2]).any()


def test_edge_coordinates_are_never_ok(case):
    m, h, *_ = case
    pts = C.edge_points(m)
    rc, v, st = C.sample_potential(h, pts, 'cpu')
    assert rc == 0 and (st == INVALID_LOCATION).all() and not bits(v).any()
    for cd in C.CDS + (1.5,):
        rc, g, st = C.sample_gradient(h, pts, cd, 'cpu')
        assert rc == 0 and np.isin(st, (INVALID_LOCATION, INVALID_GRADIENT)).all() and not bits(g).any(), (cd, st)
    # a NaN cdPrecision makes every sample a NaN point
    rc, g, st = C.sample_gradient(h, C.points(m)[:64], float('nan'), 'cpu')
    assert rc == 0 and (st == INVALID_GRADIENT).all() and not bits(g).any()


def test_invalid_calls(case, capfd):
    m, h, pts, *_ = case
    n = len(m)
    one = np.zeros(4, dtype=np.float32)
    st = np.zeros(4, dtype=np.uint8)
    p = pts[:1].copy()
    assert E.epic_hip_sample_potential_cpu(None, 1, p.ctypes.data, one.ctypes.data, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_sample_potential_cpu(h, 1, None, one.ctypes.data, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_sample_potential_cpu(h, 1, p.ctypes.data, None, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_sample_gradient_cpu(h, 1, None, 0.5, one.ctypes.data, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_sample_gradient_cpu(h, 1, p.ctypes.data, 0.5, None, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_flow_field_cpu(h, None, None, 0.5, 0, None, None) == INVALID_DATA
    big = np.zeros(int(np.prod(m)) * n, dtype=np.float32)
    assert E.epic_hip_flow_field_cpu(h, None, None, 0.5, eh_flag(), big.ctypes.data, None) == INVALID_DATA   # device output: _gpu only
    # a count of 0 is a success that touches nothing
    one[:] = 3.0
    assert E.epic_hip_sample_potential_cpu(h, 0, p.ctypes.data, one.ctypes.data, st.ctypes.data) == 0
    assert E.epic_hip_sample_gradient_cpu(h, 0, p.ctypes.data, 0.5, one.ctypes.data, st.ctypes.data) == 0
    assert (one == 3.0).all() and not st.any()
    # regions: one pointer null, an empty extent, an extent past the grid, an origin past the grid
    good_o, good_e = (0,) * n, (1,) * n
    for origin, extent in ((good_o, None), (None, good_e), (good_o, (0,) + good_e[1:]), (good_o, tuple(m[:-1]) + (m[-1] + 1,)),
                           (tuple(m), good_e), ((m[0] - 1,) + good_o[1:], (2,) + good_e[1:]), (good_o, (0xffffffff,) * n)):
        o = np.array(origin, dtype=np.uint32) if origin is not None else None
        e = np.array(extent, dtype=np.uint32) if extent is not None else None
        rc = E.epic_hip_flow_field_cpu(h, o.ctypes.data_as(C.UP) if o is not None else None, e.ctypes.data_as(C.UP) if e is not None else None,
                                       0.5, 0, big.ctypes.data, None)
        assert rc == INVALID_DATA, (origin, extent)
    # n = 4
    m4 = (3, 3, 3, 3)
    h4 = C.make(m4, np.zeros(81, dtype=np.float32), np.ones(81, dtype=np.uint32))
    p4 = np.ones(4, dtype=np.float32)
    assert E.epic_hip_sample_potential_cpu(h4, 1, p4.ctypes.data, one.ctypes.data, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_sample_gradient_cpu(h4, 1, p4.ctypes.data, 0.5, big.ctypes.data, st.ctypes.data) == INVALID_DATA
    assert E.epic_hip_flow_field_cpu(h4, None, None, 0.5, 0, big.ctypes.data, None) == INVALID_DATA
    capfd.readouterr()


def eh_flag():
    from epic_amd import epic_harmonic as eh

    return eh.EPIC_HIP_QUERY_DEVICE_OUT


def test_python_surface_on_the_host(case):
    m, h, pts, pot, grads = case
    n = len(m)
    v, st = h.potential_at(pts[:50], process='cpu')
    assert v.shape == (50,) and st.shape == (50,) and np.array_equal(bits(v), bits(pot[1][:50]))
    g, st = h.gradient_at(pts[:50], 0.5, process='cpu')
    assert g.shape == (50, n) and np.array_equal(bits(g), bits(grads[0.5][1][:50]))
    g, st = h.flow_field(process='cpu')
    assert g.shape == tuple(m) + (n,) and st.shape == tuple(m) and g.dtype == np.float32 and st.dtype == np.uint8
    origin, extent = C.regions(m)[-1]
    g2, st2 = h.flow_field(0.5, origin, extent, process='cpu')
    sl = C.region_slices(m, origin, extent)
    assert g2.shape == tuple(extent) + (n,) and np.array_equal(bits(g2), bits(g[sl])) and np.array_equal(st2, st[sl])
