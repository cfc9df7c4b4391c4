#!/usr/bin/env python3
"""A map message into the device-resident field: the callers' list route against the dense route (include/epic_hip.h:
epic_hip_set_occupancy_2d_*).  A tool, not a test; bench.py does not know about it.

Per grid (default 1024^2 and 8192^2; synthetic grid, an image that flips about 1 % of the interior cells):
  list    wall time of the route the reference's node takes: build the (x, y) and type lists as subOccupancyGrid does
          (src/epic_navigation_node_harmonic.cpp:403-422), harmonic_utilities_set_cells_2d_cpu, harmonic_utilities_set_cells_2d_gpu;
          the list building is numpy here (the node's is a C++ loop with push_back): it is timed, and reported on its own too
  dense   wall time of epic_hip_set_occupancy_2d_cpu followed by epic_hip_set_occupancy_2d_gpu
  kernel  device time of the ingestion kernel alone (HIP events on the library's stream: epic_hip_timed_occupancy_2d_gpu)
Each figure is the median of --calls calls (default 20) after --warmup (default 3).  Every call applies the same image to the same
previous state (the state is uploaded again before each call, untimed), so every call does the same work.

    python tools/bench_occupancy.py [--sizes 1024 8192] [--calls 20] [--warmup 3] [--out profiles/occupancy_ingest.txt]
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
UP = ct.POINTER(ct.c_uint)
NT = 1024


def message(m, locked, flip=0.01, seed=4):
    """int8 image restating `locked` (100 / 0) with about `flip` of the cells inverted."""
    rng = np.random.default_rng(seed)
    occ = np.where(locked.reshape(m) != 0, 100, 0).astype(np.int8)
    flips = rng.random(occ.shape) < flip
    occ[flips] = 100 - occ[flips]
    return occ


def node_lists(m, occ, u, locked):
    """subOccupancyGrid's lists for every interior cell (no_change -2 and goals skipped), vectorised."""
    inner = np.zeros(m, dtype=bool)
    inner[1:-1, 1:-1] = True
    take = inner & (occ != -2) & ~((locked.reshape(m) == 1) & (u.reshape(m) == 0.0))
    ys, xs = np.nonzero(take)
    v = np.empty(2 * len(xs), dtype=np.uint32)
    v[0::2], v[1::2] = xs, ys
    types = np.where(occ[take] >= 50, eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_CELL_TYPE_FREE).astype(np.uint32)
    return v, types


def median_ms(samples):
    return 1e3 * statistics.median(samples)


def run(n, calls, warmup):
    m = [n, n]
    u0, l0 = synthetic_grid(m, 20240601, 0.05)
    occ = message(m, l0)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0
    changed, ms = ct.c_ulonglong(0), ct.c_float(0.0)

    def restore():   # the previous state again, host and device (untimed)
        h.u_array().ravel()[:] = u0
        h.locked_array().ravel()[:] = l0
        assert E.harmonic_update_model_gpu(h) == 0

    t_list, t_build, t_dense, t_kernel, k = [], [], [], [], 0
    for i in range(warmup + calls):
        restore()
        t0 = time.perf_counter()
        v, types = node_lists(m, occ, h.u_array(), h.locked_array())
        t1 = time.perf_counter()
        assert E.harmonic_utilities_set_cells_2d_cpu(h, len(types), v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 0
        assert E.harmonic_utilities_set_cells_2d_gpu(h, NT, len(types), v.ctypes.data_as(UP), types.ctypes.data_as(UP)) == 0
        t2 = time.perf_counter()
        k = len(types)
        restore()
        t3 = time.perf_counter()
        assert E.epic_hip_set_occupancy_2d_cpu(h, occ.ctypes.data, 50, -2, 0, None) == 0
        assert E.epic_hip_set_occupancy_2d_gpu(h, occ.ctypes.data, 50, -2, 0, ct.byref(changed)) == 0
        t4 = time.perf_counter()
        restore()
        assert E.epic_hip_timed_occupancy_2d_gpu(h, occ.ctypes.data, 50, -2, 0, ct.byref(changed), ct.byref(ms)) == 0
        if i >= warmup:
            t_list.append(t2 - t0)
            t_build.append(t1 - t0)
            t_dense.append(t4 - t3)
            t_kernel.append(ms.value * 1e-3)
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    return ("%5d x %-5d  list entries %10d (%6.1f MB up)  changed %8d | list route %9.3f ms (building the lists %9.3f ms) | "
            "dense route %8.3f ms (%5.1f MB up) | kernel %7.4f ms | list / dense %.1fx"
            % (n, n, k, 12.0 * k / 1e6, changed.value, median_ms(t_list), median_ms(t_build), median_ms(t_dense), n * n / 1e6,
               median_ms(t_kernel), median_ms(t_list) / median_ms(t_dense)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--label", default="", help="a word put in front of every line (a build variant's name)")
    args = ap.parse_args()
    if args.calls < 20 or args.warmup < 3:
        ap.error("at least 20 calls after 3 warm-up calls")
    if E.epic_hip_device_count() < 1:
        sys.exit("bench_occupancy: no HIP device visible")
    head = "# %s; wall times and the kernel's device time: medians of %d calls after %d warm-up calls" % (
        E.epic_hip_version().decode(), args.calls, args.warmup)
    lines = [head] + [(args.label + " " if args.label else "") + run(n, args.calls, args.warmup) for n in args.sizes]
    for line in lines:
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
