"""Small 3-D grids: the LDS bricks (kernels_brick3d.hip) against the per-iteration kernels, same process, alternating.

Per grid and mode ({precise, tol} x {red-black, Jacobi}) and per path (bricks forced on / EPIC_HIP_BRICK=0, the parent's code path):
  * us per iteration of a warmed batch of plain iterations (epic_hip_timed_sweeps_gpu: eager launches between two device events);
  * wall time of harmonic_complete_gpu to epsilon = 1e-6 (the callers' loop: captured graphs, checks every 100 iterations);
three repetitions each, alternating between the paths; min and spread ((max - min) / min) are printed.  The two paths' fields are
compared for equality after the same number of iterations and after the relaxation.

    python tools/bench_bricks_3d.py [--grids 32x32x32,64x64x200] [--modes precise_rb,tol_jacobi] [--iters 3000] [--complete-max-cells N]
profiles/bricks_3d.txt is this tool's output.
"""
import argparse
import ctypes as ct
import os
import sys
import time

os.environ.setdefault("EPIC_HIP_STUDY", "1")   # this tool steers the kernel plan with study knobs (epic_amd/csrc/driver_config.cpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GRIDS = "32x32x32,48x48x48,64x64x64,96x96x96,128x128x128,160x160x160,256x256x256,32x128x128,64x64x200"
MODES = {"precise_rb": (None, "redblack"), "precise_jacobi": (None, "jacobi"), "tol_rb": ("tol", "redblack"), "tol_jacobi": ("tol", "jacobi")}
PATHS = {"bricks": {"EPIC_HIP_BRICK": None, "EPIC_HIP_BRICK_MAX_CELLS": str(1 << 40)}, "sweeps": {"EPIC_HIP_BRICK": "0", "EPIC_HIP_BRICK_MAX_CELLS": None}}


def set_env(kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default=GRIDS)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--complete-max-cells", type=int, default=1 << 40, help="grids above it: no harmonic_complete_gpu leg (printed as 'not measured')")
    args = ap.parse_args()
    from epic_amd import epic_harmonic as eh
    from epic_amd.harmonic import Harmonic
    from epic_amd.synthetic import synthetic_grid

    E = eh._epic

    def fresh(m, u0, locked):
        h = Harmonic()
        h.set_grid(m, u0, locked)
        h.epsilon = 1e-6
        h.numIterationsToStaggerCheck = 100
        return h

    def resident(m, u0, locked):
        h = fresh(m, u0, locked)
        for fn in (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu):
            assert fn(h) == 0
        assert E.harmonic_initialize_gpu(h, 1024) == 0
        return h

    def release(h):
        assert E.harmonic_get_potential_values_gpu(h) == 0
        for fn in (E.harmonic_uninitialize_gpu, E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu,
                   E.harmonic_uninitialize_locked_gpu):
            assert fn(h) == 0
        return h.u_array().ravel().copy()

    def stat(v):
        return "%9.3f (+%4.1f %%)" % (min(v), 100.0 * (max(v) - min(v)) / min(v))

    print("# us per plain iteration (eager batch of %d, device events) and seconds of harmonic_complete_gpu to 1e-6; min of %d (spread)" % (args.iters, args.reps))
    print("# %-25s %-14s %-34s | %-21s %-21s %6s | %-21s %-21s %6s %8s | %s" % ("grid", "mode", "brick plan", "us/it bricks", "us/it sweeps", "ratio",
                                                                                 "s complete bricks", "s complete sweeps", "ratio", "iters", "equal"))
    for g in args.grids.split(","):
        m = [int(x) for x in g.split("x")]
        u0, locked = synthetic_grid(m, seed=7, density=0.05)
        # Above 4 Mi padded cells (m0 x m1 x pitch) the library switches activity tracking on by itself, and a tracked context takes
        # neither the bricks nor the untracked sweeps: both paths are measured with tracking off there, and the row says so.
        tracked = m[0] * m[1] * ((m[2] + 255) // 256 * 256) > 1 << 22
        set_env({"EPIC_HIP_TRACK": "0" if tracked else None})
        if tracked:
            g += " (track off)"
        for mode in args.modes.split(","):
            set_env({"EPIC_HIP_MATH": MODES[mode][0], "EPIC_HIP_SCHEME": MODES[mode][1]})
            # the same 37 iterations (36 plain ones and a check) through either path: the fields must be equal
            fields, plan = {}, "none"
            for path, kv in PATHS.items():
                set_env(kv)
                h = resident(m, u0, locked)
                if path == "bricks":
                    bp = eh.config_dump(h)["path"]["brick_plan"]
                    if bp["iterations_per_launch"]:
                        plan = "H=%d %dx%dx64 x %s" % (bp["iterations_per_launch"], bp["brick"][0], bp["brick"][1], "x".join(str(b) for b in bp["bricks"]))
                assert E.epic_hip_update_n_gpu(h, 37, 1) in (0, 1)
                fields[path] = (release(h), float(h.delta))
            equal = np.array_equal(fields["bricks"][0], fields["sweeps"][0]) and fields["bricks"][1] == fields["sweeps"][1]
            if plan == "none":
                print("  %-25s %-14s no brick plan" % (g, mode), flush=True)
                continue
            # a warmed batch of plain iterations on a developed field, the paths alternating on ONE resident context
            h = resident(m, u0, locked)
            ms = ct.c_float(0)
            us = {"bricks": [], "sweeps": []}
            for rep in range(args.reps + 1):   # (the first round develops the field and warms both paths: not counted)
                for path, kv in PATHS.items():
                    set_env(kv)
                    assert E.epic_hip_config_reload(h) == 0
                    assert E.epic_hip_timed_sweeps_gpu(h, args.iters, 0, ct.byref(ms)) == 0
                    if rep:
                        us[path].append(ms.value / args.iters * 1e3)
            release(h)
            # the callers' loop, from scratch
            sec = {"bricks": [], "sweeps": []}
            done = {}
            if int(np.prod(m)) <= args.complete_max_cells:
                for rep in range(args.reps):
                    for path, kv in PATHS.items():
                        set_env(kv)
                        h = fresh(m, u0, locked)
                        t0 = time.perf_counter()
                        assert E.harmonic_complete_gpu(h, 1024) == 0
                        sec[path].append(time.perf_counter() - t0)
                        done[path] = (h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta))
                equal = equal and np.array_equal(done["bricks"][0], done["sweeps"][0]) and done["bricks"][1:] == done["sweeps"][1:]
                wall = "%-21s %-21s %6.2f %8d" % (stat(sec["bricks"]), stat(sec["sweeps"]), min(sec["sweeps"]) / min(sec["bricks"]), done["bricks"][1])
            else:
                wall = "%-21s %-21s %6s %8s" % ("not measured", "not measured", "-", "-")
            print("  %-25s %-14s %-34s | %-21s %-21s %6.2f | %s | %s" % (g, mode, plan, stat(us["bricks"]), stat(us["sweeps"]),
                                                                        min(us["sweeps"]) / min(us["bricks"]), wall, equal), flush=True)


if __name__ == "__main__":
    main()
