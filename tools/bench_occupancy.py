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

--regions vox512 box64 win256: the region calls (epic_hip_set_occupancy_region_*) on a whole 512^3 voxel grid, a 64^3 box in it and a
256^2 window of an 8192^2 map, each against the routes it replaces in the same run (run_region: the list route, the host edit followed
by harmonic_update_model_gpu, and for the 2-D window the whole-image call).  The 512^3 grid needs about 10 GB of host memory.

    python tools/bench_occupancy.py [--sizes 1024 8192] [--regions vox512 box64 win256] [--calls 20] [--warmup 3] [--out profiles/occupancy_ingest.txt]
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


REGIONS = {   # name: (grid, origin, extent, calls, warm-up calls); a call of the 512^3 list route moves 2 GB and takes seconds: fewer of them
    "vox512": ([512, 512, 512], None, None, 5, 1),
    "box64": ([512, 512, 512], (224, 224, 224), (64, 64, 64), 20, 3),
    "win256": ([8192, 8192], (4000, 4000), (256, 256), 20, 3),
}


def region_lists(m, occ, origin, u, locked):
    """The node's lists for the cells of a region (occ: the region's bytes, shape = its extent): off the faces, no_change -2 and goals
    skipped; entries are (x, y[, z]), the fastest axis first.  Only the region's cells are looked at, as a caller's loop would."""
    n = len(m)
    sl = tuple(slice(o, o + e) for o, e in zip(origin, occ.shape))
    take = (occ != -2) & ~((locked.reshape(m)[sl] == 1) & (u.reshape(m)[sl] == 0.0))
    for ax in range(n):
        keep = np.zeros(occ.shape[ax], dtype=bool)
        keep[max(1 - origin[ax], 0):min(m[ax] - 1 - origin[ax], occ.shape[ax])] = True
        take &= keep.reshape([-1 if a == ax else 1 for a in range(n)])
    idx = np.nonzero(take)
    v = np.empty(n * len(idx[0]), dtype=np.uint32)
    for ax in range(n):
        v[n - 1 - ax::n] = idx[ax] + origin[ax]
    types = np.where(occ[take] >= 50, eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_CELL_TYPE_FREE).astype(np.uint32)
    return v, types


def run_region(name):
    """One region case (epic_hip_set_occupancy_region_*) against the routes it replaces, every route on the same previous state:
      list    build the lists for the region's cells, set_cells _cpu and _gpu (harmonic_utilities_set_cells_2d_* / epic_hip_set_cells_3d_*)
      host    epic_hip_set_occupancy_region_cpu, then harmonic_update_model_gpu (field and lock array over the bus again)
      image   (2-D) a whole image that says no_change outside the window -- building it is timed --, epic_hip_set_occupancy_2d_cpu / _gpu
      region  epic_hip_set_occupancy_region_cpu, then epic_hip_set_occupancy_region_gpu
      kernel  device time of the ingestion kernel alone (epic_hip_timed_occupancy_region_gpu)"""
    m, origin, extent, calls, warmup = REGIONS[name]
    n = len(m)
    origin, extent = origin or (0,) * n, extent or tuple(m)
    u0, l0 = synthetic_grid(m, 20240601, 0.05)
    sl = tuple(slice(o, o + e) for o, e in zip(origin, extent))
    occ = np.ascontiguousarray(message(m, l0)[sl])
    print("# %s: grid %s, region %s at %s, state and message built" % (name, "x".join(map(str, m)), "x".join(map(str, extent)), origin), flush=True)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0
    changed, ms = ct.c_ulonglong(0), ct.c_float(0.0)
    o, e = (ct.c_uint * n)(*origin), (ct.c_uint * n)(*extent)
    rule = (50, -2, 0)

    def restore():   # the previous state again, host and device (untimed)
        h.u_array().ravel()[:] = u0
        h.locked_array().ravel()[:] = l0
        assert E.harmonic_update_model_gpu(h) == 0

    t = {key: [] for key in ("list", "build", "host", "upload", "image", "region", "region_gpu", "kernel")}
    k = 0
    for i in range(warmup + calls):
        restore()
        t0 = time.perf_counter()
        v, types = region_lists(m, occ, origin, h.u_array(), h.locked_array())
        t1 = time.perf_counter()
        args = (len(types), v.ctypes.data_as(UP), types.ctypes.data_as(UP))
        if n == 2:
            assert E.harmonic_utilities_set_cells_2d_cpu(h, *args) == 0 and E.harmonic_utilities_set_cells_2d_gpu(h, NT, *args) == 0
        else:
            assert E.epic_hip_set_cells_3d_cpu(h, *args) == 0 and E.epic_hip_set_cells_3d_gpu(h, *args) == 0
        t2 = time.perf_counter()
        k = len(types)
        del v, types
        restore()
        t3 = time.perf_counter()
        assert E.epic_hip_set_occupancy_region_cpu(h, occ.ctypes.data, o, e, *rule, None) == 0
        t3b = time.perf_counter()
        assert E.harmonic_update_model_gpu(h) == 0
        t4 = time.perf_counter()
        t_image = 0.0
        if n == 2:
            restore()
            t5 = time.perf_counter()
            image = np.full(m, -2, dtype=np.int8)
            image[sl] = occ
            assert E.epic_hip_set_occupancy_2d_cpu(h, image.ctypes.data, *rule, None) == 0
            assert E.epic_hip_set_occupancy_2d_gpu(h, image.ctypes.data, *rule, None) == 0
            t_image = time.perf_counter() - t5
        restore()
        t6 = time.perf_counter()
        assert E.epic_hip_set_occupancy_region_cpu(h, occ.ctypes.data, o, e, *rule, None) == 0
        t6b = time.perf_counter()
        assert E.epic_hip_set_occupancy_region_gpu(h, occ.ctypes.data, o, e, *rule, ct.byref(changed)) == 0
        t7 = time.perf_counter()
        restore()
        assert E.epic_hip_timed_occupancy_region_gpu(h, occ.ctypes.data, o, e, *rule, ct.byref(changed), ct.byref(ms)) == 0
        if i >= warmup:
            for key, value in (("list", t2 - t0), ("build", t1 - t0), ("host", t4 - t3), ("upload", t4 - t3b), ("image", t_image),
                               ("region", t7 - t6), ("region_gpu", t7 - t6b), ("kernel", ms.value * 1e-3)):
                t[key].append(value)
        print("# %s: call %d of %d" % (name, i + 1, warmup + calls), flush=True)
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    med = {key: median_ms(value) for key, value in t.items()}
    image_part = " | whole image %9.3f ms (%5.1f MB up)" % (med["image"], m[0] * m[1] / 1e6) if n == 2 else ""
    return ("%-6s %s, region %s (%d calls after %d)  changed %8d | list route %10.3f ms (%d entries, %7.1f MB up; building the lists %10.3f ms) | "
            "host edit + update_model %9.3f ms (update_model alone %9.3f ms, %6.1f MB up)%s | region route %8.3f ms (the _gpu call alone %8.3f ms, "
            "%6.2f MB up) | kernel %7.4f ms | list / region %.1fx, update_model / region %.1fx"
            % (name, "x".join(map(str, m)), "x".join(map(str, extent)), calls, warmup, changed.value, med["list"], k, 4.0 * (n + 1) * k / 1e6,
               med["build"], med["host"], med["upload"], 8.0 * u0.size / 1e6, image_part, med["region"], med["region_gpu"], occ.size / 1e6,
               med["kernel"], med["list"] / med["region"], med["host"] / med["region"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 8192])
    ap.add_argument("--regions", nargs="*", choices=sorted(REGIONS), default=[],
                    help="region cases (epic_hip_set_occupancy_region_*): vox512 a whole 512^3 grid, box64 a 64^3 box in 512^3, "
                         "win256 a 256^2 window in 8192^2; each against the routes it replaces (run_region)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--label", default="", help="a word put in front of every line (a build variant's name)")
    args = ap.parse_args()
    if args.calls < 20 or args.warmup < 3:
        ap.error("at least 20 calls after 3 warm-up calls")
    if E.epic_hip_device_count() < 1:
        sys.exit("bench_occupancy: no HIP device visible")
    head = "# %s; wall times and the kernel's device time: medians of %d calls after %d warm-up calls (region cases: as each line says)" % (
        E.epic_hip_version().decode(), args.calls, args.warmup)
    print(head, flush=True)
    lines = [head]
    jobs = [lambda n=n: run(n, args.calls, args.warmup) for n in args.sizes] + [lambda r=r: run_region(r) for r in args.regions]
    for job in jobs:
        lines.append((args.label + " " if args.label else "") + job())
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
