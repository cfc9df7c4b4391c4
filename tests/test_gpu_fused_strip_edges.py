"""The strip geometry of the fused 2-D passes (epic_amd/csrc/kernels.h: fused_2d_strips / fused_2d_col / fused_2d_owns): lane L of
strip S holds columns 248 S + 4 L .. + 3, lanes 0 and 63 are halo lanes towards a neighbouring strip only -- strip 0 owns its lane 0,
and lane 63 owns its quad where that is the last of the row, so that a pitch of 256 k with k = 1 (mod 31) takes one strip fewer
(256: 1, 8192: 33, 16128: 65).

Every comparison is bit for bit -- field and, where the call has one, delta -- against the checker (oracle/tol_checker.c for the tol
arithmetic, the reference's half-sweeps for the precise red-black pairs): no tolerance, nothing left out.  The grids are the smallest
at which each edge case exists; the goals sit where the first two or three iterations already cross the edge lanes and the seams."""
import ctypes as ct

import numpy as np
import pytest

import _oracle as O
import test_gpu_tol as T
from epic_amd import epic_harmonic as eh
from epic_amd.synthetic import synthetic_grid

E = eh._epic
NT = 1024
STRIDE, LANE_COLS = 248, 4

TOL_JACOBI, TOL_REDBLACK, PRECISE_REDBLACK = "tol_jacobi", "tol_redblack", "precise_redblack"
PATHS = {TOL_JACOBI: (eh.MATH_TOL, eh.SCHEME_JACOBI), TOL_REDBLACK: (eh.MATH_TOL, eh.SCHEME_REDBLACK),
         PRECISE_REDBLACK: (eh.MATH_PRECISE, eh.SCHEME_REDBLACK)}
ITERATIONS = (2, 3, 8, 41)       # even, odd, and (41) twenty pairs and the check
HEIGHTS = (0, 5, 7, 24)          # rows per task: the library's choice, around the six-row trip, the whole grid

# rows x cols, seed, obstacle density
GRIDS = [([24, 256], 41, 0.05),      # one strip, all 64 lanes owned
         ([24, 250], 42, 0.30),
         ([24, 300], 43, 0.10),      # three strips, a short last one
         ([24, 512], 44, 0.20),
         ([24, 8192], 45, 0.05),     # 33 strips, lane 63 of the last one owns
         ([13, 8190], 46, 0.15),     # ... with the border at column 8189, next to locked padding
         ([24, 8448], 47, 0.10),     # the neighbour that is not lucky: 35 strips, two quads in the last
         ([24, 16128], 48, 0.05)]    # the second width at which lane 63 owns
GRID_IDS = ["%dx%d" % tuple(g[0]) for g in GRIDS]


def strips_rule(pitch):
    """The fewest strips that cover a row when strip 0 owns 252 columns, the others 248 and lane 63 the row's last quad."""
    if (pitch - 2 * LANE_COLS) % STRIDE == 0:
        return (pitch - 2 * LANE_COLS) // STRIDE
    return -(-(pitch - LANE_COLS) // STRIDE)


def edge_field(m, seed, dens):
    """synthetic_grid plus goals in columns 1, 2, cols - 2, on either side of the seams at 252 and 500 and of the last seam of the
    row, and free cells in columns 1 and cols - 2 of several rows."""
    rows, cols = m
    u0, locked = synthetic_grid(m, seed, dens)
    u, lk = u0.reshape(rows, cols), locked.reshape(rows, cols)
    for r in range(2, rows - 1, 3):
        for c in (1, cols - 2):
            u[r, c], lk[r, c] = -1e6, 0
    pitch = (cols + 255) // 256 * 256
    last_seam = STRIDE * (strips_rule(pitch) - 1) + LANE_COLS     # first column the last strip's lane 1 holds
    goals = [1, 2, cols - 2, 251, 252, 499, 500] + [last_seam + d for d in (-2, -1, 0, 1)]
    goals = sorted({c for c in goals if 1 <= c <= cols - 2})
    for i, c in enumerate(goals):
        r = 1 + (5 * i) % (rows - 2)
        u[r, c], lk[r, c] = 0.0, 1
    return u0, locked


_fields, _wanted = {}, {}


def field_of(m, seed, dens):
    key = (tuple(m), seed)
    if key not in _fields:
        _fields[key] = edge_field(m, seed, dens)
    return _fields[key]


def checker(m, seed, dens, k, path):
    """Field and delta after k iterations, the last one a check: computed once per grid, arithmetic and count, never written to."""
    key = (tuple(m), seed, k, path)
    if key not in _wanted:
        u0, locked = field_of(m, seed, dens)
        math, scheme = PATHS[path]
        if math == eh.MATH_TOL:
            u, d = T.checker_iterations(m, u0, locked, k, scheme)
        else:
            p = O.Problem(m, u0, locked)
            lib = O.oracle()
            for i in range(k):
                (lib.oracle_update_and_check if i == k - 1 else lib.oracle_update)(ct.byref(p.h))
            u, d = p.u, float(p.h.delta)
        u = u.copy()
        u.setflags(write=False)
        _wanted[key] = (u, d)
    return _wanted[key]


def gpu_run(m, u0, locked, k, path, track, rows, expect):
    math, scheme = PATHS[path]
    h = T.make(m, u0, locked)
    T.gpu_init(h)
    assert E.epic_hip_set_math_mode(h, math) == 0 and E.epic_hip_set_scheme(h, scheme) == 0
    assert E.epic_hip_set_activity_tracking(h, track) == 0
    if rows:
        assert E.epic_hip_set_rows_per_task(h, rows) == 0
    plain = eh.config_dump(h)["path"]["plain_batch"]
    assert expect in plain, plain
    assert E.epic_hip_update_n_gpu(h, k, 1) in (0, 1)
    assert h.currentIteration == k
    assert E.harmonic_get_potential_values_gpu(h) == 0
    T.gpu_fini(h)
    return h.u_array().ravel().copy(), float(h.delta)


def fused_env(monkeypatch, rows):
    monkeypatch.setenv("EPIC_HIP_FUSE_MIN_CELLS", "0")
    monkeypatch.setenv("EPIC_HIP_TILE", "0")          # (the precise red-black pairs: the LDS tiles would take a grid this small)
    for name in ("EPIC_HIP_FUSED_ROWS", "EPIC_HIP_TRACK_PAIR_ROWS"):
        if rows:
            monkeypatch.setenv(name, str(rows))
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("m,seed,dens", GRIDS, ids=GRID_IDS)
def test_fused_pairs_with_owned_edge_lanes_equal_the_checker_bit_for_bit(m, seed, dens, path, monkeypatch):
    """Tracking off: the plain instantiations (jacobi_fused2d_kernel, rb_tol_fused2d_kernel, rb_fused2d_kernel).  Tracking on: the
    list-driven ones, the check riding the second level of the last pass (TRACK / CHECK)."""
    u0, locked = field_of(m, seed, dens)
    for rows in HEIGHTS:
        fused_env(monkeypatch, rows)
        for track, expect in ((0, "fused"), (1, "tracked pairs")):
            for k in ITERATIONS:
                want, wdelta = checker(m, seed, dens, k, path)
                got, gdelta = gpu_run(m, u0, locked, k, path, track, rows, expect)
                bad = np.flatnonzero(got != want)
                print("%s %s: %d iterations, %d rows per task, tracking %d: %d cells differ, delta %r against %r"
                      % (m, path, k, rows, track, bad.size, gdelta, wdelta))
                assert bad.size == 0, f"{m} {path}, {k} iterations, {rows} rows per task, tracking {track}: first at column {bad[0] % m[1]}"
                assert gdelta == wdelta


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("m,seed,dens", [GRIDS[3], GRIDS[4]], ids=[GRID_IDS[3], GRID_IDS[4]])
def test_funnel_instantiation_equals_the_checker_bit_for_bit(m, seed, dens):
    """epic_hip_sweeps_2d with a null d_maskf: the pass cuts its masks from the standard layout itself (a funnel shift of two words
    per row, from quad 62 S on)."""
    import torch

    rows, cols = m
    u0, locked = field_of(m, seed, dens)
    pitch = E.epic_hip_pitch_for_cols(cols)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d_locked = torch.from_numpy(locked.astype(np.int32)).to(dev)
    maskw = torch.zeros(E.epic_hip_mask_words_2d(rows, pitch), dtype=torch.int32, device=dev)
    assert E.epic_hip_pack_mask_2d(d_locked.data_ptr(), rows, cols, pitch, 0, 0, maskw.data_ptr(), s) == 0
    for rpp in HEIGHTS:
        for k in ITERATIONS:
            a = torch.full((rows, pitch), -1e6, dtype=torch.float32, device=dev)
            a[:, :cols] = torch.from_numpy(u0.reshape(rows, cols)).to(dev)
            b = a.clone()
            flips = ct.c_int(-1)
            assert E.epic_hip_sweeps_2d(a.data_ptr(), b.data_ptr(), maskw.data_ptr(), None, rows, pitch, k, 10, rpp, eh.MATH_TOL,
                                        ct.byref(flips), s) == 0
            torch.cuda.synchronize()
            got = (b if flips.value else a)[:, :cols].cpu().numpy().ravel()
            want, _ = checker(m, seed, dens, k, TOL_JACOBI)       # (the raw operator has no delta)
            assert np.array_equal(got, want), f"{m}, {k} sweeps, {rpp} rows per pair"


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("path", list(PATHS))
def test_tracked_pairs_on_two_slabs_equal_the_checker_bit_for_bit(path, monkeypatch):
    """Two in-library slabs on the one GPU: the wake ranges after a halo exchange are counted in strips of the fused tiling
    (driver_multi.hip: multi_run_pairs)."""
    m, seed, dens = [48, 8192], 49, 0.05
    monkeypatch.setenv("EPIC_HIP_DEVICES", "0,0")
    monkeypatch.setenv("EPIC_HIP_HALO", "8")
    u0, locked = field_of(m, seed, dens)
    for rows in (0, 5):
        fused_env(monkeypatch, rows)
        for k in ITERATIONS:
            want, wdelta = checker(m, seed, dens, k, path)
            got, gdelta = gpu_run(m, u0, locked, k, path, 1, rows, "slabs: tracked pairs")
            assert np.array_equal(got, want), f"{path}, {k} iterations, {rows} rows per task"
            assert gdelta == wdelta


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("pitch", [256, 512, 8192])
def test_fused_mask_layout(pitch):
    """epic_hip_fuse_masks_2d against the layout as kernels.h states it: per row and strip four 64-bit words, bit L of word j = the
    lock of column 248 S + 4 L + j.  Only the bits of cells inside the row are compared."""
    import torch

    rows, cols = 5, pitch
    rng = np.random.default_rng(pitch)
    locked = (rng.random((rows, cols)) < 0.4).astype(np.uint32)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d_locked = torch.from_numpy(locked.astype(np.int32)).to(dev)
    maskw = torch.zeros(E.epic_hip_mask_words_2d(rows, pitch), dtype=torch.int32, device=dev)
    words = int(E.epic_hip_mask_words_fused_2d(rows, pitch))
    nstrips = strips_rule(pitch)
    assert words == rows * nstrips * 8
    maskf = torch.zeros(words, dtype=torch.int32, device=dev)
    assert E.epic_hip_pack_mask_2d(d_locked.data_ptr(), rows, cols, pitch, 0, 0, maskw.data_ptr(), s) == 0
    assert E.epic_hip_fuse_masks_2d(maskw.data_ptr(), rows, pitch, maskf.data_ptr(), s) == 0
    torch.cuda.synchronize()
    got = maskf.cpu().numpy().view(np.uint64).reshape(rows, nstrips, 4)
    want = locked != 0                                  # what pack_mask_2d makes of it: the border is forced locked
    want[0, :] = want[-1, :] = True
    want[:, 0] = want[:, -1] = True
    seen = np.zeros(cols, dtype=bool)
    for strip in range(nstrips):
        for lane in range(64):
            for j in range(4):
                c = STRIDE * strip + LANE_COLS * lane + j
                if c >= cols:
                    continue
                seen[c] = True
                bits = ((got[:, strip, j] >> np.uint64(lane)) & np.uint64(1)).astype(bool)
                assert np.array_equal(bits, want[:, c]), (strip, lane, j)
    assert seen.all()


def test_strip_counts():
    """Host side (no device needed): epic_hip_mask_words_fused_2d is 8 words per row and strip."""
    for pitch in range(256, 65536 + 1, 4):
        n, rem = divmod(int(E.epic_hip_mask_words_fused_2d(3, pitch)), 3 * 8)
        assert rem == 0 and n == strips_rule(pitch), pitch
        assert n <= -(-pitch // STRIDE), pitch
        # the rule covers the row: 252 columns from strip 0, 248 from the others, four more where lane 63 holds the last quad
        assert STRIDE * n + LANE_COLS >= pitch or STRIDE * n + 2 * LANE_COLS == pitch, pitch
        assert n == 1 or STRIDE * (n - 1) + LANE_COLS < pitch, pitch     # and no strip is left without a column of its own
    counts = {p: int(E.epic_hip_mask_words_fused_2d(1, p)) // 8 for p in (256, 512, 4096, 8192, 8448, 16128, 32768)}
    assert counts == {256: 1, 512: 3, 4096: 17, 8192: 33, 8448: 35, 16128: 65, 32768: 133}
