#!/usr/bin/env python3
"""The rolling-window shift of the resident field (include/epic_hip.h: epic_hip_shift_field_gpu) against the copy it cannot beat and
the host route it replaces.  A tool, not a test; bench.py does not know about it.

Per grid (default 1024^2, 8192^2, 64^3, 128^3, 512^3; synthetic grid) and per shift (one cell along each axis, and a diagonal of
(3, -33) / (1, 3, -33): a column shift that is no multiple of 4):
  kernel  *kernel_ms of the call: the one launch that moves values and lock bits (HIP events on the library's stream)
  copy    a device-to-device copy of ONE u buffer of that grid (rows x pitch floats), timed with events on torch's stream in the
          same process: the floor -- the kernel reads and writes that much, plus 1/32 of it in lock bits
  host    once per grid, the route a caller had: harmonic_get_potential_values_gpu, the shift in numpy on u and locked,
          harmonic_update_model_gpu (wall time)
kernel and copy: medians of --calls (default 20) after --warmup (default 3); host: of --host-calls (default 3) after 1.

    python tools/bench_shift.py [--grids 1024x1024 8192x8192 64x64x64 128x128x128 512x512x512] [--out profiles/shift_field.txt]
"""
import argparse
import ctypes as ct
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epic_amd import epic_harmonic as eh   # noqa: E402
from epic_amd.harmonic import Harmonic   # noqa: E402
from epic_amd.synthetic import synthetic_grid   # noqa: E402

E = eh._epic
NT = 1024


def copy_floor_ms(floats, calls, warmup):
    src, dst = torch.zeros(floats, dtype=torch.float32, device="cuda"), torch.empty(floats, dtype=torch.float32, device="cuda")
    ms = []
    for i in range(warmup + calls):
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
        dst.copy_(src, non_blocking=True)
        ev[1].record()
        ev[1].synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def numpy_shift(a, shift, fill):
    """new[x] = old[x + shift] on the interior, in place (through a copy of the interior, as a caller would write it)"""
    inner = a[tuple(slice(1, d - 1) for d in a.shape)]
    old = inner.copy()
    inner[...] = fill
    spans = [(max(0, -s), min(d, d - s)) for d, s in zip(inner.shape, shift)]
    inner[tuple(slice(lo, hi) for lo, hi in spans)] = old[tuple(slice(lo + s, hi + s) for (lo, hi), s in zip(spans, shift))]


def run(m, calls, warmup, host_calls):
    n = len(m)
    u0, l0 = synthetic_grid(m, 20240601, 0.05)
    h = Harmonic()
    h.set_grid(m, u0, l0)
    for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    assert E.harmonic_initialize_gpu(h, NT) == 0
    floats = int(np.prod(m[:-1])) * int(E.epic_hip_pitch_for_cols(m[-1]))
    copy = copy_floor_ms(floats, calls, warmup)
    diagonal = ((1, 3, -33) if n == 3 else (3, -33))
    host = []
    for i in range(1 + host_calls):
        t0 = time.perf_counter()
        assert E.harmonic_get_potential_values_gpu(h) == 0
        numpy_shift(h.u_array(), diagonal, np.float32(-1e6))
        numpy_shift(h.locked_array(), diagonal, 0)
        assert E.harmonic_update_model_gpu(h) == 0
        if i >= 1:
            host.append(1e3 * (time.perf_counter() - t0))
    lines = []
    kept, ms = ct.c_ulonglong(0), ct.c_float(0.0)
    for shift in [tuple(int(a == i) for a in range(n)) for i in range(n)] + [diagonal]:
        t = []
        for i in range(warmup + calls):
            assert E.epic_hip_shift_field_gpu(h, (ct.c_int * n)(*shift), eh.EPIC_CELL_TYPE_FREE, ct.byref(kept), ct.byref(ms)) == 0
            if i >= warmup:
                t.append(ms.value)
        kernel = statistics.median(t)
        lines.append("%-11s shift %-12s kept %10d | kernel %8.4f ms | copy of one u buffer (%7.1f MB) %8.4f ms | kernel / copy %5.2f | "
                     "host route %10.3f ms (%d calls after 1) | host / kernel %.0fx"
                     % ("x".join(map(str, m)), shift, kept.value, kernel, 4e-6 * floats, copy, kernel / copy, statistics.median(host), host_calls,
                        statistics.median(host) / kernel))
        print(lines[-1], flush=True)
    for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
               E.harmonic_uninitialize_locked_gpu):
        assert fn(h) == 0, fn.__name__
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", nargs="*", default=["1024x1024", "8192x8192", "64x64x64", "128x128x128", "512x512x512"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.calls < 20 or args.warmup < 3:
        ap.error("at least 20 calls after 3 warm-up calls")
    if E.epic_hip_device_count() < 1:
        sys.exit("bench_shift: no HIP device visible")
    lines = ["# %s; kernel and copy: device times, medians of %d calls after %d warm-up calls" % (E.epic_hip_version().decode(), args.calls, args.warmup)]
    print(lines[0], flush=True)
    for grid in args.grids:
        lines += run([int(d) for d in grid.split("x")], args.calls, args.warmup, args.host_calls)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
