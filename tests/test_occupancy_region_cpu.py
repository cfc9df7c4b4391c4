"""epic_hip_set_occupancy_region_cpu / epic_hip_reset_free_cells_3d_cpu (include/epic_hip.h; epic_amd/csrc/occupancy_cpu.cpp): a
block of bytes applied to a rectangular region of the host arrays of a 2-D or 3-D grid -- against epic_hip_set_occupancy_2d_cpu
(whole 2-D grids; windows through a full image that says no_change outside; 3-D grids plane by plane), against the list route
(epic_hip_set_cells_3d_cpu on the triples the node would build) and against the numpy statement of the rule masked to the region.
Every comparison is bitwise.  The windows and boxes sit where an index error would: on the border and the faces, on the last row
and column, across columns 127 / 128 and 255 / 256 / 257, with three different extents."""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

import occupancy_cases as C
import occupancy_region_cases as R
from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic

E = eh._epic
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).ravel().view(np.uint32), np.asarray(b, dtype=np.float32).ravel().view(np.uint32))


def region_cpu(m, occ, origin, extent, u, locked, thr, no_change, flags):
    """(u, locked, changed) of epic_hip_set_occupancy_region_cpu; origin = extent = None: the whole grid."""
    h = Harmonic()
    h.set_grid(m, u, locked)
    changed = ct.c_ulonglong(12345)
    occ = np.ascontiguousarray(occ)
    o, e = (R.uints(origin), R.uints(extent)) if origin is not None else (None, None)
    assert E.epic_hip_set_occupancy_region_cpu(h, occ.ctypes.data, o, e, thr, no_change, flags, ct.byref(changed)) == 0
    return h.u_array().ravel().copy(), h.locked_array().ravel().copy(), int(changed.value)


def dense_2d_cpu(m, occ, u, locked, thr, no_change, flags):
    h = Harmonic()
    h.set_grid(m, u, locked)
    changed = ct.c_ulonglong(12345)
    occ = np.ascontiguousarray(occ)
    assert E.epic_hip_set_occupancy_2d_cpu(h, occ.ctypes.data, thr, no_change, flags, ct.byref(changed)) == 0
    return h.u_array().ravel().copy(), h.locked_array().ravel().copy(), int(changed.value)


# ---- 1. the whole 2-D grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.GRIDS_2D, ids=R.ident)
def test_whole_2d_grid_equals_the_2d_call(m):
    u0, l0 = C.previous_state(m)
    occ = C.image(m)
    for kw in (C.NODE, C.COSTMAP):
        for flags in C.ALL_FLAGS:
            want = dense_2d_cpu(m, occ, u0, l0, kw["thr"], kw["no_change"], flags)
            got = region_cpu(m, occ, None, None, u0, l0, kw["thr"], kw["no_change"], flags)
            assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
            # ... and the same with the grid spelled out, and the n-axis numpy rule is occupancy_cases.rule on two axes
            spelled = region_cpu(m, occ, (0, 0), m, u0, l0, kw["thr"], kw["no_change"], flags)
            assert same(spelled[0], want[0]) and np.array_equal(spelled[1], want[1]) and spelled[2] == want[2]
            ru, rl, rc = R.rule_nd(m, occ, np.ones(m, dtype=bool), u0, l0, kw["thr"], kw["no_change"], flags)
            cu, cl, cc = C.rule(m, occ, u0, l0, kw["thr"], kw["no_change"], flags)
            assert same(ru, cu) and np.array_equal(rl, cl) and rc == cc == want[2]
    if m != [3, 5]:
        assert want[2] > 0


# ---- 2. 2-D windows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.GRIDS_2D, ids=R.ident)
def test_2d_windows(m):
    u0, l0 = C.previous_state(m)
    full = C.image(m)
    windows = R.windows_2d(m)
    if m == [130, 515]:
        assert sorted(windows) == ["anchored", "cell", "crossing", "fours", "last", "odd"]
        assert windows["odd"][0][1] % 2 == 1 and windows["odd"][1][1] % 4 != 0
        assert windows["fours"][0][1] % 4 == 0 and windows["fours"][1][1] % 4 == 0
    moved = 0
    for name, (origin, extent) in windows.items():
        occ = R.cut(full, origin, extent)
        box = R.inside(m, origin, extent)
        for flags in (0, C.KEEP):
            # the node's rule: a full image that says no_change outside the window, through the 2-D call
            kw = dict(C.NODE, flags=flags)
            padded = np.where(box, full, np.int8(kw["no_change"])).astype(np.int8)
            want = dense_2d_cpu(m, padded, u0, l0, **kw)
            got = region_cpu(m, occ, origin, extent, u0, l0, **kw)
            assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], name
            # the costmap rule (no_change out of range): the numpy rule masked to the window
            kw = dict(C.COSTMAP, flags=C.COSTMAP["flags"] | flags)
            want = R.rule_nd(m, full, box, u0, l0, **kw)
            got = region_cpu(m, occ.view(np.uint8), origin, extent, u0, l0, **kw)
            assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], name
            assert same(got[0][~box.ravel()], u0[~box.ravel()]) and np.array_equal(got[1][~box.ravel()], l0[~box.ravel()])
            moved += got[2]
    assert moved > 0 or m == [3, 5]


# ---- 3. 3-D -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.GRIDS_3D, ids=R.ident)
def test_whole_3d_grid_equals_the_2d_call_plane_by_plane(m):
    u0, l0 = R.state_3d(m)
    occ = R.image_nd(m)
    plane = [m[1], m[2]]
    for kw in (C.NODE, C.COSTMAP, dict(C.NODE, flags=C.KEEP)):
        got_u, got_l, got_changed = region_cpu(m, occ, None, None, u0, l0, **kw)
        total = 0
        for z in range(m[0]):
            pu, pl = u0.reshape(m)[z], l0.reshape(m)[z]
            if 0 < z < m[0] - 1:
                pu, pl, changed = dense_2d_cpu(plane, occ[z], pu, pl, **kw)
                total += changed
            assert same(got_u.reshape(m)[z], pu) and np.array_equal(got_l.reshape(m)[z].ravel(), np.asarray(pl).ravel()), z
        assert got_changed == total
        assert got_changed > 0 or m == [3, 3, 5]


@pytest.mark.parametrize("m", R.GRIDS_3D, ids=R.ident)
def test_whole_3d_grid_equals_the_list_route(m):
    u0, l0 = R.state_3d(m)
    occ = R.image_nd(m)
    v, t = R.node_lists_3d(m, occ, u0, l0)
    assert len(t) > 0
    h = Harmonic()
    h.set_grid(m, u0, l0)
    assert E.epic_hip_set_cells_3d_cpu(h, len(t), v.ctypes.data_as(C.UP), t.ctypes.data_as(C.UP)) == 0
    got_u, got_l, _ = region_cpu(m, occ, None, None, u0, l0, **C.NODE)
    assert same(got_u, h.u_array()) and np.array_equal(got_l, h.locked_array().ravel())


@pytest.mark.parametrize("m", R.GRIDS_3D, ids=R.ident)
def test_3d_boxes_equal_the_numpy_rule_masked_to_the_box(m):
    u0, l0 = R.state_3d(m)
    full = R.image_nd(m)
    boxes = R.boxes_3d(m)
    assert {"voxel", "face_x0_lo", "face_x0_hi", "face_x1_lo", "face_x1_hi", "face_x2_lo", "face_x2_hi", "planes", "extents"} <= set(boxes)
    assert len(set(boxes["extents"][1])) == 3 and boxes["planes"][1][0] == m[0]
    if m[2] > 256:
        o, e = boxes["crossing"]
        assert o[2] <= 255 and o[2] + e[2] > 256
    moved = 0
    for name, (origin, extent) in boxes.items():
        occ = R.cut(full, origin, extent)
        box = R.inside(m, origin, extent)
        for kw in (C.NODE, C.COSTMAP, dict(C.NODE, flags=C.KEEP)):
            want = R.rule_nd(m, full, box, u0, l0, **kw)
            got = region_cpu(m, occ, origin, extent, u0, l0, **kw)
            assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (name, kw)
            moved += got[2]
    assert moved > 0


# ---- 4. errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [[5, 7], [4, 5, 7]], ids=R.ident)
def test_error_returns_leave_the_arrays_untouched(m, capfd):
    u0, l0 = (C.previous_state(m) if len(m) == 2 else R.state_3d(m))
    occ = np.full(int(np.prod(m)) + 64, 100, dtype=np.int8)            # every byte an obstacle: a call that went on would show
    h = Harmonic()
    h.set_grid(m, u0, l0)
    changed = ct.c_ulonglong(777)

    def expect(fn, *args):
        capfd.readouterr()
        assert fn(*args) == eh.EPIC_ERROR_INVALID_DATA
        assert "Error[%s]: Invalid data." % fn.__name__ in capfd.readouterr().err
        assert same(h._keep["u"], u0) and np.array_equal(h._keep["locked"], l0) and changed.value == 777

    for origin, extent in R.bad_regions(m):
        o = R.uints(origin) if origin is not None else None
        e = R.uints(extent) if extent is not None else None
        expect(E.epic_hip_set_occupancy_region_cpu, h, occ.ctypes.data, o, e, 50, -2, 0, ct.byref(changed))
    expect(E.epic_hip_set_occupancy_region_cpu, h, None, None, None, 50, -2, 0, ct.byref(changed))          # null occ
    expect(E.epic_hip_set_occupancy_region_cpu, None, occ.ctypes.data, None, None, 50, -2, 0, ct.byref(changed))
    if len(m) == 2:
        expect(E.epic_hip_reset_free_cells_3d_cpu, h)                   # the 3-D reset on a 2-D grid
    h4 = Harmonic()
    h4.set_grid([3, 3, 3, 4], np.zeros(108, dtype=np.float32), np.zeros(108, dtype=np.uint32))
    expect(E.epic_hip_set_occupancy_region_cpu, h4, occ.ctypes.data, None, None, 50, -2, 0, ct.byref(changed))   # n == 4
    expect(E.epic_hip_reset_free_cells_3d_cpu, h4)
    assert same(h4.u_array(), np.zeros(108)) and not h4.locked_array().any()
    h.m = ct.POINTER(ct.c_uint)()
    expect(E.epic_hip_set_occupancy_region_cpu, h, occ.ctypes.data, None, None, 50, -2, 0, ct.byref(changed))    # null m
    h.m = h._keep["m"].ctypes.data_as(ct.POINTER(ct.c_uint))
    assert E.epic_hip_set_occupancy_region_cpu(h, occ.ctypes.data, None, None, 50, -2, 0, None) == 0          # changed == NULL
    assert not same(h.u_array(), u0)


# ---- 5. reset ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.GRIDS_3D, ids=R.ident)
def test_reset_free_cells_3d(m):
    u0, l0 = R.state_3d(m)
    l0 = l0.copy()
    l0.reshape(m)[0, 1, 1] = 0                                          # an unlocked face cell: not an interior cell, left alone
    h = Harmonic()
    h.set_grid(m, u0, l0)
    assert E.epic_hip_reset_free_cells_3d_cpu(h) == 0
    want = u0.copy().reshape(m)
    inner = (slice(1, -1),) * 3
    want[inner][l0.reshape(m)[inner] == 0] = np.float32(-1e6)
    assert same(h.u_array(), want) and np.array_equal(h.locked_array().ravel(), l0)
    if m != [3, 3, 5]:
        assert not same(want, u0)
    v, t = R.reset_lists_3d(m, l0)                                      # ... which is the list route
    g = Harmonic()
    g.set_grid(m, u0, l0)
    if len(t):
        assert E.epic_hip_set_cells_3d_cpu(g, len(t), v.ctypes.data_as(C.UP), t.ctypes.data_as(C.UP)) == 0
    assert same(g.u_array(), want)


# ---- the Python method on the host arrays -------------------------------------------------------------------------------
def test_python_method_takes_a_3d_grid_and_a_window():
    m = [6, 7, 300]
    u0, l0 = R.state_3d(m)
    full = R.image_nd(m)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    want = region_cpu(m, full, None, None, u0, l0, **C.NODE)
    assert h.set_occupancy(full, process='cpu') == want[2]
    assert same(h.u_array(), want[0]) and np.array_equal(h.locked_array().ravel(), want[1])
    origin, extent = R.boxes_3d(m)["extents"]
    h.set_grid(m, u0, l0)
    want = region_cpu(m, R.cut(full, origin, extent), origin, extent, u0, l0, **dict(C.NODE, flags=C.KEEP))
    assert h.set_occupancy(R.cut(full, origin, extent), keep_free=True, process='cpu', origin=origin) == want[2]
    assert same(h.u_array(), want[0]) and np.array_equal(h.locked_array().ravel(), want[1])
    h.reset_free_cells(process='cpu')
    assert np.all(h.u_array()[1:-1, 1:-1, 1:-1][h.locked_array()[1:-1, 1:-1, 1:-1] == 0] == np.float32(-1e6))
    m2 = [37, 301]
    u2, l2 = C.previous_state(m2)
    img = C.image(m2)
    origin, extent = R.windows_2d(m2)["crossing"]
    g = Harmonic()
    g.set_grid(m2, u2, l2)
    want = region_cpu(m2, R.cut(img, origin, extent), origin, extent, u2, l2, **C.NODE)
    assert g.set_occupancy(R.cut(img, origin, extent), process='cpu', origin=origin) == want[2]
    assert same(g.u_array(), want[0]) and np.array_equal(g.locked_array().ravel(), want[1])
    with pytest.raises(ValueError):
        g.set_occupancy(R.cut(img, origin, extent), process='cpu', origin=(m2[0] - 1, 0))   # not inside the grid
    with pytest.raises(ValueError):
        g.set_occupancy(R.cut(img, origin, extent).ravel(), process='cpu', origin=origin)   # a window needs its shape


# ---- 6. the host walk under AddressSanitizer and UBSan ------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_region_walk_is_clean_under_asan_and_ubsan(tmp_path):
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if (subprocess.run(["g++", *sanitize, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0):
        pytest.skip("this g++ has no sanitizer runtime that runs here")
    exe = str(tmp_path / "occupancy_region_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *sanitize, "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "occupancy_region_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "occupancy region host code: ok" in run.stdout
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed"):
        assert bad not in run.stderr, run.stderr[-2000:]
