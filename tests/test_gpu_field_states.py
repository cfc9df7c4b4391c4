"""The consumers and the sparse edit of the resident field in every state the solver leaves it in (include/epic_hip.h, "3-D fields";
epic_amd/csrc/field3d_driver.hip, field_3d.hip, path_2d.hip, driver_ext.hip): epic_hip_compute_paths_3d_gpu, epic_hip_set_cells_3d_gpu and
epic_hip_compute_paths_2d_gpu address the field as buf[cur] plus the lane masks, which is right only if cur, the deferred iterations, the
work lists and the captured graphs are in the state the call assumes.  tests/test_gpu_field3d.py walks and edits buf[0] after a read-back
only; here the same calls run on buf[1], between captured batches, under both arithmetics, with and without work lists, with iterations
still counted and not yet run, and straight after an edit.

Every comparison is bit for bit.  Fields are compared with the checker (oracle/), walks with the host walker on the read-back field
(epic_hip_compute_path_3d_cpu, harmonic_compute_path_2d_cpu).  Every test sets the scheme and the arithmetic it needs, so the file means
the same under both EPIC_TEST_SCHEME sessions."""
import ctypes as ct
import hashlib
import json
import os

import numpy as np
import pytest

import _oracle as O
from epic_amd import epic_harmonic as eh
from epic_amd.synthetic import synthetic_grid
from test_gpu_field3d import (DENSITY, FREE, GOAL, GRIDS, MAX_LEN, NT, OBSTACLE, SEED, WALL_X, E, PF, U, UP, bits, device_paths, edit_list,
                              gpu_fini, gpu_init, host_path, make, relax_on_device, seeded_starts)
from test_path3d_cpu import FACE_GOAL, WILD_X, WILD_X_CODES

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

PRECISE, TOL = eh.MATH_PRECISE, eh.MATH_TOL
JACOBI, REDBLACK = eh.SCHEME_JACOBI, eh.SCHEME_REDBLACK
SCHEME_IDS = {JACOBI: "jacobi", REDBLACK: "redblack"}
MATH_IDS = {PRECISE: "precise", TOL: "tol"}


def set_modes(h, math, scheme, track=None):
    assert E.epic_hip_set_math_mode(h, math) == 0 and E.epic_hip_set_scheme(h, scheme) == 0
    if track is not None:
        assert E.epic_hip_set_activity_tracking(h, track) == 0


def plain_batch_path(h):
    buf = ct.create_string_buffer(1 << 16)
    assert E.epic_hip_config_dump(h, buf, len(buf)) > 0
    return json.loads(buf.value.decode())["path"]["plain_batch"]


def set_cells_args(v, t):
    return len(t), v.ctypes.data_as(UP), t.ctypes.data_as(UP)


def walk_and_compare(h, starts, step, cd, max_len=MAX_LEN, read_back=True, memo=None):
    """The batched device walk FIRST, then (read_back) the field comes to the host arrays, then every row against the host walk of its
    start: the code, k, the bytes, NaN beyond 3 * k (a failed path leaves its whole row untouched).  Returns [(code, bytes)] per start.
    memo: host walks per distinct start, for batches that repeat starts."""
    rc, k, codes, out = device_paths(h, starts, step, cd, max_len)
    assert rc == 0
    if read_back:
        assert E.harmonic_get_potential_values_gpu(h) == 0
    memo = {} if memo is None else memo
    got = []
    for i, s in enumerate(starts):
        key = s.tobytes()
        if key not in memo:
            memo[key] = host_path(h, s, step, cd, max_len)
        want, pts = memo[key]
        assert codes[i] == want, (i, s, codes[i], want)
        if want != 0:
            assert k[i] == 0 and np.isnan(out[i]).all(), (i, s)
            got.append((int(want), b""))
            continue
        assert 3 * k[i] == pts.size, (i, s)
        assert out[i, :3 * k[i]].tobytes() == pts.tobytes(), (i, s)
        assert np.isnan(out[i, 3 * k[i]:]).all(), (i, s)
        got.append((0, pts.tobytes()))
    return got


# ---- 1. the sparse edit between captured batches, against the checker, in every context -----------------------------
# (7, 40, 300): 7 planes = a plane group of 4 and one of 3, and an odd plane for the two-planes-per-wave kernel; 40 rows = a 32-row chunk, a
# second chunk of 8 and ragged tails; 300 columns = two 256-column strips.
EDIT_GRID = (7, 40, 300)
NEAR_GOAL = [(149, 20, 3), (151, 20, 4), (150, 19, 3), (150, 22, 3)]      # next to the synthetic goal (150, 20, 3): relaxed at the edit
QUIET_GOAL = (280, 35, 5)


def state_edits(m, locked):
    """(v, types), no cell twice: see the list in the test's docstring"""
    L = np.asarray(locked).reshape(m)
    nz, ny, nx = m
    # goals: interior, on an x == 0 face cell, and QUIET_GOAL beyond the wall, in a tile (second strip, second chunk) that the front of the
    # synthetic goal has not reached by the edit: no work list names it, only the edit's force_all has it swept
    v, t = [(100, 10, 2), (0, 20, 3), QUIET_GOAL], [GOAL, GOAL, GOAL]
    wall = [(x, y, z) for x in (255, 256) for z in range(1, nz - 1) for y in range(1, ny - 1) if y not in (31, 32)]
    v += wall
    t += [OBSTACLE] * len(wall)
    freed = [tuple(c[::-1]) for c in (np.argwhere(L[1:-1, 1:-1, 1:-1] != 0) + 1).tolist() if c[2] > 257][:3]   # obstacles beyond the wall
    assert len(freed) == 3
    v += freed
    t += [FREE] * len(freed)
    seam = []                                                                         # FREE on free cells at the plane-group seam
    for z in (3, 4):
        for x in (31, 32, 63, 64):
            y = next(y for y in range(1, ny - 1) if L[z, y, x] == 0)
            seam.append((x, y, z))
    near = [c for c in NEAR_GOAL if L[c[2], c[1], c[0]] == 0]                         # ... and on cells the front has reached
    assert len(near) >= 2
    v += seam + near
    t += [FREE] * (len(seam) + len(near))
    v += [(nx - 1, 5, 2), (10, 0, 2), (10, ny - 1, 2), (10, 5, 0), (10, 5, nz - 1)]   # FREE on the other five faces
    t += [FREE] * 5
    v += [(nx, 1, 1), (1, ny, 1), (1, 1, nz), (0xFFFFFFFF, 2, 2)]                     # outside the grid, once per axis
    t += [OBSTACLE, GOAL, FREE, OBSTACLE]
    v += [(50, 5, 2), (51, 5, 2)]                                                     # invalid types
    t += [3, 0xFFFFFFFF]
    assert len(set(v)) == len(v)
    return np.array(v, dtype=np.uint32), np.array(t, dtype=np.uint32), near


def numpy_edit(m, u, locked, v, t):
    """The rule, stated independently: GOAL -> 0 and locked, OBSTACLE -> -1e6 and locked, FREE -> -1e6 and unlocked; entries outside the
    grid and types above 2 are skipped."""
    u3, l3 = u.reshape(m), locked.reshape(m)
    for (x, y, z), ty in zip(v.tolist(), t.tolist()):
        if x >= m[2] or y >= m[1] or z >= m[0] or ty > 2:
            continue
        u3[z, y, x] = 0.0 if ty == GOAL else -1e6
        l3[z, y, x] = 0 if ty == FREE else 1


def checker_run(p, k, math, scheme, check_last):
    """k iterations on Problem p as the table says: tol -> oracle_tol_run, precise Jacobi -> oracle_jacobi_run (both leave the delta of
    their last iteration), precise red-black -> oracle_update, the last one oracle_update_and_check where a check is asked for."""
    lib = O.oracle()
    if math == TOL:
        assert lib.oracle_tol_run(ct.byref(p.h), k, scheme) == 0
    elif scheme == JACOBI:
        assert lib.oracle_jacobi_run(ct.byref(p.h), k) == 0
    else:
        for i in range(k):
            (lib.oracle_update_and_check if check_last and i == k - 1 else lib.oracle_update)(ct.byref(p.h))


@pytest.fixture(scope="module")
def edit_case():
    u0, l0 = synthetic_grid(list(EDIT_GRID), SEED, DENSITY)
    v, t, near = state_edits(EDIT_GRID, l0)
    return u0, l0, v, t, near


@pytest.mark.parametrize("pre", [20, 21])
@pytest.mark.parametrize("track", [0, 1])
@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
@pytest.mark.parametrize("math", [PRECISE, TOL], ids=MATH_IDS.get)
def test_edit_between_captured_batches_equals_the_checker(edit_case, math, scheme, track, pre):
    """update_n(9) twice (the second may replay what the first captured), 2 or 3 single updates, the edit, update_n(9) twice, one check,
    read-back -- against the same sequence on the checker, the edit applied to its arrays by numpy_edit.  Under Jacobi the edit lands in
    buf[0] after 20 iterations and in buf[1] after 21.  The list: goals at an interior cell, on an x == 0 face cell and in a tile that is
    quiet at the edit (with work lists, only the edit's force_all gets its neighbours swept); a wall on columns
    255 and 256 (the strip seam) with a gap at rows 31 and 32 (the chunk seam); obstacles freed beyond it; FREE on free cells at columns
    31, 32, 63, 64 of planes 3 and 4 (the plane-group seam) and on relaxed cells next to the goal; FREE on a cell of each other face
    (locked on the device, never swept by the checker); entries outside the grid; invalid types."""
    m = EDIT_GRID
    u0, l0, v, t, near = edit_case
    after = 19
    # the checker
    p = O.Problem(m, u0, l0, epsilon=1e-4)
    checker_run(p, pre, math, scheme, False)
    for x, y, z in near:
        assert p.field()[z, y, x] != np.float32(-1e6)                   # FREE there resets a relaxed value: not a no-op
    qx, qy, qz = QUIET_GOAL
    assert (p.field()[:, 32:, 256:] == np.float32(-1e6)).all() and qy >= 32 and qx >= 256   # nothing has moved in that goal's tile yet
    twin = make(m, p.u.copy(), p.locked.copy())                         # the host statement of the edit on a copy of the same state
    assert E.epic_hip_set_cells_3d_cpu(twin, *set_cells_args(v, t)) == 0
    numpy_edit(m, p.u, p.locked, v, t)
    assert np.array_equal(bits(twin.u_array()), bits(p.u)) and np.array_equal(twin.locked_array().ravel(), p.locked)
    checker_run(p, after, math, scheme, True)
    plain = O.Problem(m, u0, l0, epsilon=1e-4)                          # the same run without the edit
    checker_run(plain, pre, math, scheme, False)
    checker_run(plain, after, math, scheme, True)
    # the device
    h = make(m, u0, l0)
    gpu_init(h)
    set_modes(h, math, scheme, track)
    path = plain_batch_path(h)
    for _ in range(2):
        assert E.epic_hip_update_n_gpu(h, 9, 0) == 0
    for _ in range(pre - 18):
        assert E.harmonic_update_gpu(h, NT) == 0
    assert h.currentIteration == pre
    assert E.epic_hip_set_cells_3d_gpu(h, *set_cells_args(v, t)) == 0
    for _ in range(2):
        assert E.epic_hip_update_n_gpu(h, 9, 0) == 0
    assert E.harmonic_update_and_check_gpu(h, NT) in (0, 1)
    assert E.harmonic_get_potential_values_gpu(h) == 0
    got, delta, its = h.u_array().copy(), float(h.delta), int(h.currentIteration)
    gpu_fini(h)
    differ = int((bits(got) != bits(plain.u)).sum())
    print("%s %s track %d, %d + %d iterations (%s): %d cells differ from the run without the edit, delta %.9g"
          % (MATH_IDS[math], SCHEME_IDS[scheme], track, pre, after, path, differ, delta))
    wrong = np.flatnonzero(bits(got) != bits(p.u))
    assert wrong.size == 0, (wrong.size, [np.unravel_index(i, m) for i in wrong[:8]])
    assert delta == float(p.h.delta)
    assert its == p.h.currentIteration == pre + after
    assert differ > 0                                                   # the edit mattered


# ---- 2. walks at both buffer parities, with an iteration counted but not read back, and straight after an edit -----
WALL_STARTS = np.array([(WALL_X, y, z) for z in (2, 5, 8) for y in (3, 9, 15)], dtype=np.float32)


@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
@pytest.mark.parametrize("m", GRIDS, ids=lambda m: "x".join(map(str, m)))
def test_walks_at_both_buffer_parities_and_straight_after_an_edit(m, scheme):
    """relax_on_device runs whole blocks of 100 and reads back, so cur is 0; one more harmonic_update_gpu puts a Jacobi field into buf[1]
    and leaves an iteration the host arrays have not seen.  The walk comes first, then the read-back, then the host walks.  On
    (12, 20, 37) the edit of test_gpu_field3d.py follows on both sides (without its face cell, which the device keeps locked and the
    host unlocks -- documented, and not what this is about), and the same starts plus nine on the new wall are walked with no iteration
    in between: the edited u and masks are all that changed."""
    step, cd = 0.2, 0.5
    u0, l0 = synthetic_grid(list(m), SEED, DENSITY)
    h = make(m, u0, l0)
    gpu_init(h)
    set_modes(h, PRECISE, scheme)
    relax_on_device(h)
    before_update = h.u_array().copy()
    assert E.harmonic_update_gpu(h, NT) == 0
    starts = seeded_starts(h.shape, h.locked_array())
    first = walk_and_compare(h, starts, step, cd)
    moved = int((bits(before_update) != bits(h.u_array())).sum())
    ok = sum(code == 0 for code, _ in first)
    print("grid %s %s: iteration %d moved %d cells, %d of %d walks succeed" % (m, SCHEME_IDS[scheme], h.currentIteration, moved, ok, len(starts)))
    assert 2 * ok >= len(starts)
    # the walks read another field than the one read back before: on (12, 20, 37) the checker moves some 2000 cells in iteration 401 of either
    # scheme; (6, 9, 300) has come to rest in f32 by iteration 800 and nothing moves there
    assert h.currentIteration % 2 == 1 and (moved > 0 or m != GRIDS[0])
    if m != GRIDS[0]:
        gpu_fini(h)
        return
    v, t = edit_list(m, l0)
    keep = ~(v == np.array([0, 7, 4], dtype=np.uint32)).all(axis=1)
    assert keep.sum() == len(t) - 1
    v, t = np.ascontiguousarray(v[keep]), np.ascontiguousarray(t[keep])
    assert E.epic_hip_set_cells_3d_gpu(h, *set_cells_args(v, t)) == 0
    assert E.epic_hip_set_cells_3d_cpu(h, *set_cells_args(v, t)) == 0
    want = h.u_array().copy()
    assert E.harmonic_get_potential_values_gpu(h) == 0
    assert np.array_equal(bits(h.u_array()), bits(want))                # the resident field is the host-edited one
    second = walk_and_compare(h, np.concatenate([starts, WALL_STARTS]), step, cd, read_back=False)
    gpu_fini(h)
    ok = sum(code == 0 for code, _ in second[:len(starts)])
    changed = sum(a != b for a, b in zip(first, second))
    print("grid %s %s: %d of %d walks succeed straight after the edit, %d differ from before it, wall starts %s"
          % (m, SCHEME_IDS[scheme], ok, len(starts), changed, [code for code, _ in second[len(starts):]]))
    assert 2 * ok >= len(starts)
    assert changed >= 10
    assert all(code == 10 for code, _ in second[len(starts):])


# ---- 3. and 4. share one resident field ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resident():
    """(12, 20, 37) relaxed on the device to 1e-4 (precise, red-black), then FACE_GOAL -- an x == 0 face cell -- made a goal on the device
    and on the host arrays: host arrays == resident field.  Only read afterwards."""
    m = GRIDS[0]
    u0, l0 = synthetic_grid(list(m), SEED, DENSITY)
    h = make(m, u0, l0)
    gpu_init(h)
    set_modes(h, PRECISE, REDBLACK)
    relax_on_device(h)
    v, t = np.array([FACE_GOAL], dtype=np.uint32), np.array([GOAL], dtype=np.uint32)
    assert E.epic_hip_set_cells_3d_gpu(h, *set_cells_args(v, t)) == 0
    assert E.epic_hip_set_cells_3d_cpu(h, *set_cells_args(v, t)) == 0
    want = h.u_array().copy()
    assert E.harmonic_get_potential_values_gpu(h) == 0
    assert np.array_equal(bits(h.u_array()), bits(want)) and want[FACE_GOAL[2], FACE_GOAL[1], FACE_GOAL[0]] == 0.0
    yield h
    gpu_fini(h)


BATCH_STEP, BATCH_CD, BATCH_LEN = 0.2, 0.5, 40


@pytest.fixture(scope="module")
def batch_memo():
    return {}


@pytest.mark.parametrize("n", [1, 8, 9, 63, 64, 65, 4097, 8200])
def test_batch_sizes_around_the_copy_routes_and_past_the_pack_grid(resident, batch_memo, n):
    """Up to 8 paths come back in a copy each, 9 and more through pack_paths_3d_kernel, whose launch is capped at 4096 blocks: 4097 and
    8200 paths make its grid-stride loop stride.  Every row against the host walk of its start."""
    h = resident
    base = seeded_starts(h.shape, h.locked_array())
    starts = np.ascontiguousarray(np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n])
    got = walk_and_compare(h, starts, BATCH_STEP, BATCH_CD, BATCH_LEN, read_back=False, memo=batch_memo)
    ok = sum(code == 0 for code, _ in got)
    print("batch of %d: %d walks succeed" % (n, ok))
    assert ok >= 1 and (n < 64 or 2 * ok >= n)


def test_packed_batch_in_which_nothing_walks_and_one_whose_ends_fail(resident, batch_memo):
    h = resident
    L, u = h.locked_array(), h.u_array()
    obst = (np.argwhere((L[1:-1, 1:-1, 1:-1] != 0) & (u[1:-1, 1:-1, 1:-1] < 0)) + 1)[:9, ::-1]
    assert len(obst) == 9
    starts = np.ascontiguousarray(obst, dtype=np.float32)
    rc, k, codes, out = device_paths(h, starts, BATCH_STEP, BATCH_CD, BATCH_LEN)
    assert rc == 0 and (codes == 10).all() and (k == 0).all() and np.isnan(out).all()      # total == 0: no copy-back, rows untouched
    got = walk_and_compare(h, starts, BATCH_STEP, BATCH_CD, BATCH_LEN, read_back=False)
    assert [code for code, _ in got] == [10] * 9
    good = [s for s in seeded_starts(h.shape, h.locked_array()) if host_path(h, s, BATCH_STEP, BATCH_CD, BATCH_LEN)[0] == 0][:10]
    assert len(good) == 10
    ends = np.ascontiguousarray(np.array([starts[0]] + good + [(-2.0, 5.0, 5.0)], dtype=np.float32))
    got = walk_and_compare(h, ends, BATCH_STEP, BATCH_CD, BATCH_LEN, read_back=False)
    assert [code for code, _ in got] == [10] + [0] * 10 + [10]


# ---- 4. start points and parameters nobody sends on purpose ----------------------------------------------------------
def test_start_points_far_outside_the_index_range(resident):
    """to_index is (unsigned)(long long)v on both sides; for NaN, +-inf and |v| >= 2^63 the host result is what x86-64's conversion
    leaves (a low word of 0, i.e. column 0 -- here the goal FACE_GOAL, so the walk is a valid start that goes nowhere: 13), and the
    device must say the same.  tests/test_path3d_cpu.py pins the host's codes."""
    h = resident
    starts = np.array([(x, FACE_GOAL[1], FACE_GOAL[2]) for x in WILD_X], dtype=np.float32)
    for n in (len(starts), 1):                                          # the packed route, and the direct copies one start at a time
        for lo in range(0, len(starts), n):
            part = np.ascontiguousarray(starts[lo:lo + n])
            rc, k, codes, out = device_paths(h, part, 0.2, 0.5, 300)
            assert rc == 0
            want = [host_path(h, s, 0.2, 0.5, 300)[0] for s in part]
            print("x = %s: device %s host %s" % (part[:, 0].tolist(), codes.tolist(), want))
            assert codes.tolist() == want == WILD_X_CODES[lo:lo + n]
            assert (k == 0).all() and np.isnan(out).all()


@pytest.mark.parametrize("step,cd", [(50.0, 0.5), (3.0, 0.5), (0.0, 0.5), (-0.2, 0.5), (0.2, 0.0), (0.2, 1.5), (0.2, 40.0)])
def test_step_sizes_and_precisions_the_host_handles(resident, step, cd):
    h = resident
    starts = seeded_starts(h.shape, h.locked_array(), n=60, seed=11)
    got = walk_and_compare(h, starts, step, cd, 300, read_back=False)
    codes = [code for code, _ in got]
    longest = max([len(b) // 12 for _, b in got] + [0])
    print("step %g cd %g: codes %s, longest %d points" % (step, cd, {c: codes.count(c) for c in sorted(set(codes))}, longest))
    if step == 0.0:
        assert longest == 300                                           # never stuck (distance 0 is not < 0): runs to the length bound


# ---- 5. the 2-D walker after the solver's own passes -----------------------------------------------------------------
PLANS = {"tiles": {}, "fused": {"EPIC_HIP_TILE": "0", "EPIC_HIP_FUSE_MIN_CELLS": "0"}, "singles": {}}
PLAN_RUNS = [("tiles", 1), ("tiles", 2), ("tiles", 3), ("fused", 1), ("fused", 2), ("fused", 3), ("singles", 3)]
_host_walks_2d = {}    # (map, sha1 of the field) -> [(code, bytes)]: the plans of one (math, scheme, k) leave the same field


def host_walks_2d(name, h, starts, step, cd, max_len):
    key = (name, hashlib.sha1(h.u_array().tobytes()).hexdigest())
    if key not in _host_walks_2d:
        rows = []
        for s in starts:
            kk, raw = U(0), PF()
            rc = E.harmonic_compute_path_2d_cpu(h, float(s[0]), float(s[1]), step, cd, max_len, ct.byref(kk), ct.byref(raw))
            if rc != 0:
                rows.append((rc, b""))
                continue
            rows.append((0, np.ctypeslib.as_array(raw, shape=(2 * kk.value,)).tobytes()))
            E.harmonic_free_path_cpu(ct.byref(raw))
        _host_walks_2d[key] = rows
    return _host_walks_2d[key]


@pytest.mark.parametrize("plan,k", PLAN_RUNS, ids=["%s-%d" % pk for pk in PLAN_RUNS])
@pytest.mark.parametrize("scheme", [JACOBI, REDBLACK], ids=SCHEME_IDS.get)
@pytest.mark.parametrize("math", [PRECISE, TOL], ids=MATH_IDS.get)
@pytest.mark.parametrize("name", ["maze", "umass"])
def test_2d_walker_after_the_solvers_own_passes(goldens, name, math, scheme, plan, k, monkeypatch):
    """The converged golden uploaded, then k iterations by the LDS tiles (default plan), by the fused pairs / single sweeps
    (EPIC_HIP_TILE=0, EPIC_HIP_FUSE_MIN_CELLS=0) or three single harmonic_update_gpu calls left pending: each flips cur or swaps the spare
    buffer.  The device walks the 300 starts of test_device_streamline_batch_equals_host_walk first; then the field is read back and the
    host walker says what they must be."""
    for var in ("EPIC_HIP_TILE", "EPIC_HIP_FUSE_MIN_CELLS"):
        monkeypatch.delenv(var, raising=False)
    for var, val in PLANS[plan].items():
        monkeypatch.setenv(var, val)
    m, _, locked = O.load_png_reference_rule(os.path.join(O.ROOT, "tests", "golden", "maps", name + ".png"))
    golden = np.asarray(goldens["maps"][name + "/converged_1e-06"], dtype=np.float32)
    h = make(m, golden, locked)
    gpu_init(h)
    assert E.epic_hip_config_reload(h) == 0
    set_modes(h, math, scheme)
    path = plain_batch_path(h)
    if plan == "tiles":
        assert path.startswith("LDS tiles")
    elif plan == "fused":
        assert ("fused" in path) if (math == TOL or scheme == REDBLACK) else path.startswith("single sweeps")   # precise Jacobi has no fused pass
    if plan == "singles":
        for _ in range(k):
            assert E.harmonic_update_gpu(h, NT) == 0
    else:
        assert E.epic_hip_update_n_gpu(h, k, 0) == 0
    rows, cols = m
    rng = np.random.default_rng(99)
    n, max_len, step, cd = 300, 6000, 0.45, 0.5
    starts = np.empty((n, 2), dtype=np.float32)
    starts[:, 0] = rng.uniform(-3.0, cols + 2.0, n)
    starts[:, 1] = rng.uniform(-3.0, rows + 2.0, n)
    rc, kk, codes, out = device_paths(h, starts, step, cd, max_len)
    assert rc == 0
    assert E.harmonic_get_potential_values_gpu(h) == 0
    assert h.currentIteration == k
    moved = int((bits(h.u_array()) != bits(golden)).sum())             # (0 under precise red-black: the golden is that iteration's fixed point)
    want = host_walks_2d(name, h, starts, step, cd, max_len)
    gpu_fini(h)
    ok = 0
    for i, (code, pts) in enumerate(want):
        assert codes[i] == code, (i, starts[i], codes[i], code)
        assert 8 * kk[i] == len(pts), (i, starts[i])
        assert out[i, :2 * kk[i]].tobytes() == pts, "path %d from %s" % (i, starts[i])
        assert np.isnan(out[i, 2 * kk[i]:]).all()
        ok += code == 0
    print("%s %s %s %s x %d (%s): %d cells moved, %d of %d walks succeed" % (name, MATH_IDS[math], SCHEME_IDS[scheme], plan, k, path, moved, ok, n))
    assert ok > 50
