#!/usr/bin/env python3
"""Queries of the device-resident field against the only route they replace (include/epic_hip.h, "Field queries").  A tool, not a
test; bench.py does not know about it.

Before these calls every question asked of a resident field went through harmonic_get_potential_values_gpu -- the whole field over
the bus -- followed by host calls.  Here each new route is timed against that one in the same run:
  2-D, 8192^2 (--size2):  one cell (epic_hip_get_cells_gpu); the flow field of a 256^2 window; the whole-grid flow field with host
                          output and with device output; 4096 and 1 048 576 gradient samples
  2-D, 512^2 (--small):   one cell, 16 and 4096 gradient samples -- where the copy is cheap and the device route can lose
  3-D, 512^3 (--size3):   the flow field of a 64^3 box and of the whole grid (host and device output)
  host route              the copy, then the host twin of the call (epic_hip_flow_field_cpu / epic_hip_sample_gradient_cpu: the
                          arithmetic of harmonic_compute_gradient_2d_cpu / epic_hip_compute_gradient_3d_cpu in a C loop, i.e. the
                          fastest that route can be); both parts are given on their own.  Results are compared byte for byte.
Each figure is the median wall time of --calls calls (default 20) after --warmup (default 3); the host twin on a WHOLE grid takes
seconds per call and is timed --host-whole-calls times (default 1) without warm-up.
For the two whole-grid kernels: the time of the call with device output (kernel + launch + synchronise; the stream is the library's
own), the bytes the shapes move (2-D: 4 + 1/8 read, 8 + 1 written per cell; 3-D: 4 + 1/8 and 12 + 1) and the time a device-to-device
copy takes to move the same number of bytes (half of them read, half written) in the same run.
The field: the seeded synthetic grid with a developed-like start (epic_amd.synthetic.ramp_rows: every free cell away from -1e6) and
--iterations sweeps -- a field with a gradient at nearly every cell; convergence at these sizes takes minutes and changes no load.

    python tools/bench_field_queries.py [--size2 8192] [--size3 512] [--calls 20] [--warmup 3] [--out profiles/field_queries.txt]
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
from epic_amd.synthetic import ramp_rows, synthetic_grid   # noqa: E402

E = eh._epic
UP = ct.POINTER(ct.c_uint)
NT = 1024
CD = 0.5
DEVICE_OUT = eh.EPIC_HIP_QUERY_DEVICE_OUT


def resident(m, density, iterations):
    u0, l0 = synthetic_grid(m, 20240601, density)
    ramp_rows(m, 0, m[0], u0, l0)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0
    assert E.epic_hip_update_n_gpu(h, iterations, 1) in (0, 1)
    assert E.harmonic_get_potential_values_gpu(h) == 0
    return h


def release(h):
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        fn(h)


def timed(fn, calls, warmup):
    """median wall time in ms of `calls` calls of fn after `warmup`"""
    samples = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            samples.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(samples)


def copy_back(h):
    assert E.harmonic_get_potential_values_gpu(h) == 0


def region(origin, extent):
    o, e = np.array(origin, dtype=np.uint32), np.array(extent, dtype=np.uint32)
    return o.ctypes.data_as(UP), e.ctypes.data_as(UP), (o, e)


def row(name, dev_ms, copy_ms, host_ms, same, extra=""):
    return ("%-44s | device route %10.3f ms | host route %10.3f ms (copy %9.3f + host calls %10.3f) | host / device %8.1fx | identical: %s%s"
            % (name, dev_ms, copy_ms + host_ms, copy_ms, host_ms, (copy_ms + host_ms) / dev_ms, "yes" if same else "NO", extra))


def flow_cases(h, a, lines, label, window):
    """the flow field of `window` and of the whole grid on h"""
    import torch

    m, n = h.shape, len(h.shape)
    copy_ms = timed(lambda: copy_back(h), a.calls, a.warmup)
    for origin, extent, whole in ((window[0], window[1], False), (None, None, True)):
        shape = tuple(extent) if extent is not None else m
        cells = int(np.prod(shape))
        o, e, keep = region(origin, extent) if origin is not None else (None, None, ())
        g_dev, s_dev = np.empty(shape + (n,), dtype=np.float32), np.empty(shape, dtype=np.uint8)
        g_host, s_host = np.empty(shape + (n,), dtype=np.float32), np.empty(shape, dtype=np.uint8)

        def device():
            assert E.epic_hip_flow_field_gpu(h, o, e, CD, 0, g_dev.ctypes.data, s_dev.ctypes.data) == 0

        def host():
            assert E.epic_hip_flow_field_cpu(h, o, e, CD, 0, g_host.ctypes.data, s_host.ctypes.data) == 0

        dev_ms = timed(device, a.calls, a.warmup)
        host_ms = timed(host, a.host_whole_calls, 0) if whole else timed(host, a.calls, a.warmup)
        same = g_dev.tobytes() == g_host.tobytes() and s_dev.tobytes() == s_host.tobytes()
        ok = float((s_dev == 0).mean())
        name = "%s flow field %s" % (label, "whole grid, host output" if whole else "x".join(map(str, shape)) + " window")
        lines.append(row(name, dev_ms, copy_ms, host_ms, same, " | %.0f %% of the cells OK, %.1f MB back" % (100 * ok, (4 * n + 1) * cells / 1e6)))
        if not whole:
            continue
        dev = torch.device("cuda", 0)
        tg = torch.empty(shape + (n,), dtype=torch.float32, device=dev)
        ts = torch.empty(shape, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def device_out():
            assert E.epic_hip_flow_field_gpu(h, None, None, CD, DEVICE_OUT, tg.data_ptr(), ts.data_ptr()) == 0

        out_ms = timed(device_out, a.calls, a.warmup)
        same_out = tg.cpu().numpy().tobytes() == g_host.tobytes() and ts.cpu().numpy().tobytes() == s_host.tobytes()
        moved = (4 + 1 / 8 + 4 * n + 1) * cells
        half = int(moved // 2)
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        src.zero_()
        torch.cuda.synchronize()

        def d2d():
            dst.copy_(src)
            torch.cuda.synchronize()

        d2d_ms = timed(d2d, a.calls, a.warmup)
        lines.append(row("%s flow field whole grid, device output" % label, out_ms, copy_ms, host_ms, same_out,
                         " | kernel (call with device output) %.3f ms for %.0f MB by the shapes = %.0f GB/s; a device-to-device copy "
                         "moving the same bytes %.3f ms; kernel / copy %.2fx"
                         % (out_ms, moved / 1e6, moved / out_ms / 1e6, d2d_ms, out_ms / d2d_ms)))
        del tg, ts, src, dst
        torch.cuda.empty_cache()
    return copy_ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size2", type=int, default=8192)
    ap.add_argument("--size3", type=int, default=512)
    ap.add_argument("--small", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-whole-calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if E.epic_hip_device_count() < 1:
        raise SystemExit("bench_field_queries.py: no HIP device visible")
    lines = ["# %s; seeded grids (5 %% / 2 %% obstacles, one goal), developed-like start and %d sweeps; cdPrecision %g"
             % (E.epic_hip_version().decode(), a.iterations, CD),
             "# wall times: medians of %d calls after %d warm-up calls (the host twin on a whole grid: %d call(s), no warm-up)"
             % (a.calls, a.warmup, a.host_whole_calls)]

    # ---- 2-D ----
    n2 = a.size2
    h = resident([n2, n2], 0.05, a.iterations)
    lines.append("# 2-D: %d^2, field %.0f MB" % (n2, 4.0 * n2 * n2 / 1e6))
    copy_ms = flow_cases(h, a, lines, "2-D", ((n2 // 2 - 128, n2 // 2 - 128), (min(256, n2 // 2), min(256, n2 // 2))))
    # one cell
    cell = np.array([[n2 // 2 + 3, n2 // 2 - 5]], dtype=np.uint32)
    u1, l1 = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.uint32)

    def one_cell():
        assert E.epic_hip_get_cells_gpu(h, 1, cell.ctypes.data, u1.ctypes.data, l1.ctypes.data) == 0

    dev_ms = timed(one_cell, a.calls, a.warmup)
    t0 = time.perf_counter()
    value = h.u_array()[cell[0, 1], cell[0, 0]]
    index_ms = 1e3 * (time.perf_counter() - t0)
    lines.insert(3, row("2-D one cell (srvGetCell)", dev_ms, copy_ms, index_ms, u1[0].tobytes() == np.float32(value).tobytes()))
    # gradient samples
    rng = np.random.default_rng(12)
    for count in (4096, 1 << 20):
        pts = np.ascontiguousarray(rng.uniform(2.0, n2 - 3.0, (count, 2)).astype(np.float32))
        gd, sd = np.empty((count, 2), dtype=np.float32), np.empty(count, dtype=np.uint8)
        gh, sh = np.empty((count, 2), dtype=np.float32), np.empty(count, dtype=np.uint8)

        def device():
            assert E.epic_hip_sample_gradient_gpu(h, count, pts.ctypes.data, CD, gd.ctypes.data, sd.ctypes.data) == 0

        def host():
            assert E.epic_hip_sample_gradient_cpu(h, count, pts.ctypes.data, CD, gh.ctypes.data, sh.ctypes.data) == 0

        dev_ms, host_ms = timed(device, a.calls, a.warmup), timed(host, a.calls, a.warmup)
        same = gd.tobytes() == gh.tobytes() and sd.tobytes() == sh.tobytes()
        lines.append(row("2-D %7d gradient samples" % count, dev_ms, copy_ms, host_ms, same, " | %.0f %% OK" % (100 * float((sd == 0).mean()))))
    release(h)
    del h

    # ---- a small map: the copy is cheap there, and a device call has a floor (an allocation, a launch, two copies, a synchronise) ----
    ns = a.small
    h = resident([ns, ns], 0.05, a.iterations)
    lines.append("# 2-D small map: %d^2, field %.1f MB" % (ns, 4.0 * ns * ns / 1e6))
    copy_ms = timed(lambda: copy_back(h), a.calls, a.warmup)
    cell = np.array([[ns // 2 + 3, ns // 2 - 5]], dtype=np.uint32)
    dev_ms = timed(one_cell, a.calls, a.warmup)
    lines.append(row("small one cell", dev_ms, copy_ms, index_ms, u1[0].tobytes() == np.float32(h.u_array()[cell[0, 1], cell[0, 0]]).tobytes()))
    for count in (16, 4096):
        pts = np.ascontiguousarray(rng.uniform(2.0, ns - 3.0, (count, 2)).astype(np.float32))
        gd, sd = np.empty((count, 2), dtype=np.float32), np.empty(count, dtype=np.uint8)
        gh, sh = np.empty((count, 2), dtype=np.float32), np.empty(count, dtype=np.uint8)
        dev_ms, host_ms = timed(device, a.calls, a.warmup), timed(host, a.calls, a.warmup)
        same = gd.tobytes() == gh.tobytes() and sd.tobytes() == sh.tobytes()
        lines.append(row("small %7d gradient samples" % count, dev_ms, copy_ms, host_ms, same, " | %.0f %% OK" % (100 * float((sd == 0).mean()))))
    release(h)
    del h

    # ---- 3-D ----
    n3 = a.size3
    h = resident([n3, n3, n3], 0.02, a.iterations)
    lines.append("# 3-D: %d^3, field %.0f MB" % (n3, 4.0 * n3 ** 3 / 1e6))
    box = min(64, n3 // 2)
    flow_cases(h, a, lines, "3-D", ((n3 // 2 - box // 2,) * 3, (box,) * 3))
    release(h)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_field_queries.py on one MI355X: queries of the device-resident field against "
                    "harmonic_get_potential_values_gpu plus host calls\n" + text)


if __name__ == "__main__":
    main()
