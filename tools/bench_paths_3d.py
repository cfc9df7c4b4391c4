#!/usr/bin/env python3
"""Streamlines and sparse edits on a device-resident 3-D field against the routes they replace (include/epic_hip.h, "3-D fields").
A tool, not a test; bench.py does not know about it.

On a seeded synthetic n^3 grid (default 512^3, the next smaller size that fits otherwise), relaxed on the device:
  paths, for 1, 64 and 4096 start points at interior free cells:
    host route    harmonic_get_potential_values_gpu (the whole field over the bus) followed by epic_hip_compute_path_3d_cpu for every
                  start -- before the device walk existed the copy was the only way out of the device, and a caller's own walker
                  followed it; both parts are timed and given on their own
    device route  epic_hip_compute_paths_3d_gpu, one call
    the two routes' way-points are compared, byte for byte
  edits, for a handful of cells:
    sparse        epic_hip_set_cells_3d_gpu
    re-upload     epic_hip_set_cells_3d_cpu on the host arrays, then harmonic_initialize_potential_values_gpu +
                  harmonic_initialize_locked_gpu: both arrays over the bus again
Each figure is the median wall time of --calls calls (default 20) after --warmup (default 3).  A lone walk is a chain of dependent
memory round trips: per step the device is slower than the host, and the table says so next to the copy it avoids.

    python tools/bench_paths_3d.py [--size 512] [--epsilon 1e-4] [--calls 20] [--warmup 3] [--out profiles/paths_3d.txt]
"""
import argparse
import ctypes as ct
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epic_amd import epic_harmonic as eh   # noqa: E402
from epic_amd.harmonic import Harmonic   # noqa: E402
from epic_amd.synthetic import synthetic_grid   # noqa: E402

E = eh._epic
PF, UP, PI = ct.POINTER(ct.c_float), ct.POINTER(ct.c_uint), ct.POINTER(ct.c_int)
NT = 1024
STEP, CD = 0.5, 0.5


def resident_grid(n, density):
    """A Harmonic over the seeded n^3 grid with its device state, or None when the device state does not fit."""
    m = [n, n, n]
    u0, l0 = synthetic_grid(m, 20240601, density)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        if fn(h) != 0:
            for undo in (E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu, E.harmonic_uninitialize_locked_gpu):
                undo(h)
            return None
    assert E.harmonic_initialize_gpu(h, NT) == 0
    return h


def relax(h, epsilon, max_iterations):
    h.epsilon = epsilon
    t0 = time.perf_counter()
    converged = False
    while h.currentIteration < max_iterations and not converged:
        rc = E.epic_hip_update_n_gpu(h, 100, 1)
        assert rc in (0, 1), rc
        converged = rc == 1
    return converged, time.perf_counter() - t0


def median_ms(samples):
    return 1e3 * statistics.median(samples)


def starts_at_free_cells(h, count, seed=12):
    rng = np.random.default_rng(seed)
    n = h.shape[0]
    locked = h.locked_array()
    pts = []
    while len(pts) < count:
        z, y, x = (int(v) for v in rng.integers(2, n - 2, 3))
        if locked[z, y, x] == 0:
            pts.append((x, y, z))
    return np.ascontiguousarray(np.array(pts, dtype=np.float32) + rng.uniform(-0.3, 0.3, (count, 3)).astype(np.float32))


def host_route(h, starts, max_len):
    """(seconds of the copy, seconds of the walks, way-points per start, codes)"""
    t0 = time.perf_counter()
    assert E.harmonic_get_potential_values_gpu(h) == 0
    t1 = time.perf_counter()
    pts, codes = h.compute_paths(starts, STEP, CD, max_len, process='cpu')
    return t1 - t0, time.perf_counter() - t1, pts, codes


def device_route(h, starts, max_len, k, codes, out):
    t0 = time.perf_counter()
    rc = E.epic_hip_compute_paths_3d_gpu(h, len(starts), starts.ctypes.data_as(PF), STEP, CD, max_len, k.ctypes.data_as(UP),
                                         codes.ctypes.data_as(PI), out.ctypes.data_as(PF))
    assert rc == 0, rc
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--epsilon", type=float, default=1e-4)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 4096])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if E.epic_hip_device_count() < 1:
        raise SystemExit("bench_paths_3d.py: no HIP device visible")
    err = os.dup(2)   # the host walker reports every failed walk on stderr: thousands of lines that say nothing here
    devnull = os.open(os.devnull, os.O_WRONLY)

    h, n = None, a.size
    while h is None:
        h = resident_grid(n, a.density)
        if h is None:
            n = n * 3 // 4
            assert n >= 32, "no size fits"
    converged, relax_s = relax(h, a.epsilon, a.max_iterations)
    lines = ["# %s; %d^3 seeded grid (%.0f %% obstacles, one goal), %s after %d iterations (%.2f s) at epsilon %g; step %g, cdPrecision %g;"
             % (E.epic_hip_version().decode(), n, 100 * a.density, "converged" if converged else "NOT converged", h.currentIteration, relax_s,
                a.epsilon, STEP, CD),
             "# wall times: medians of %d calls after %d warm-up calls; field %.0f MB" % (a.calls, a.warmup, 4.0 * n ** 3 / 1e6)]
    max_len = 4 * n
    assert E.harmonic_get_potential_values_gpu(h) == 0
    for count in a.counts:
        starts = starts_at_free_cells(h, count)
        k = np.zeros(count, dtype=np.uint32)
        codes = np.zeros(count, dtype=np.int32)
        out = np.empty((count, 3 * max_len), dtype=np.float32)
        t_copy, t_walk, t_dev = [], [], []
        same = True
        for i in range(a.warmup + a.calls):
            os.dup2(devnull, 2)
            c, w, pts, host_codes = host_route(h, starts, max_len)
            os.dup2(err, 2)
            d = device_route(h, starts, max_len, k, codes, out)
            if i >= a.warmup:
                t_copy.append(c), t_walk.append(w), t_dev.append(d)
            elif i == 0:
                same = np.array_equal(codes, host_codes) and all(out[j, :3 * k[j]].tobytes() == pts[j].tobytes() for j in range(count))
        ok = codes == 0
        points = int(k.sum())
        host_ms = median_ms(t_copy) + median_ms(t_walk)
        lines.append("paths %5d starts  %5d walked, %8d way-points (longest %5d) | host route %9.3f ms (copy %9.3f + walks %9.3f) | device route %8.3f ms "
                     "(%6.1f KB back) | host / device %6.1fx | per way-point: host walks %7.3f us, device route %7.3f us | identical: %s"
                     % (count, int(ok.sum()), points, int(k.max()), host_ms, median_ms(t_copy), median_ms(t_walk), median_ms(t_dev), 12.0 * points / 1e3,
                        host_ms / median_ms(t_dev), 1e3 * median_ms(t_walk) / max(points, 1), 1e3 * median_ms(t_dev) / max(points, 1), "yes" if same else "NO"))

    # a handful of edits: the sparse call against the re-upload it replaces
    rng = np.random.default_rng(5)
    cells = np.ascontiguousarray(np.unique(rng.integers(2, n - 2, (8, 3)), axis=0).astype(np.uint32))
    t_sparse, t_upload = [], []
    for i in range(a.warmup + a.calls):
        types = np.full(len(cells), eh.EPIC_CELL_TYPE_OBSTACLE if i % 2 == 0 else eh.EPIC_CELL_TYPE_FREE, dtype=np.uint32)
        args = (len(types), cells.ctypes.data_as(UP), types.ctypes.data_as(UP))
        t0 = time.perf_counter()
        assert E.epic_hip_set_cells_3d_gpu(h, *args) == 0
        t1 = time.perf_counter()
        assert E.epic_hip_set_cells_3d_cpu(h, *args) == 0
        assert E.harmonic_initialize_potential_values_gpu(h) == 0 and E.harmonic_initialize_locked_gpu(h) == 0
        t2 = time.perf_counter()
        if i >= a.warmup:
            t_sparse.append(t1 - t0), t_upload.append(t2 - t1)
    lines.append("edits %5d cells   | sparse (epic_hip_set_cells_3d_gpu) %8.3f ms | re-upload (u and locked, %.0f MB) %9.3f ms | re-upload / sparse %7.1fx"
                 % (len(cells), median_ms(t_sparse), 8.0 * n ** 3 / 1e6, median_ms(t_upload), median_ms(t_upload) / median_ms(t_sparse)))
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        fn(h)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_paths_3d.py on one MI355X: streamlines and sparse edits on the device-resident 3-D field against the routes they replace\n" + text)


if __name__ == "__main__":
    main()
