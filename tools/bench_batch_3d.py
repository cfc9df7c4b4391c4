"""Several voxel fields on one box: epic_hip_complete_batch_gpu against the loop of harmonic_complete_gpu it replaces, same process, alternating.

Per shape, epsilon and number of fields B -- every field has the box's seeded obstacles and ONE goal of its own, a free cell drawn from
a fixed seed -- the wall time of either route, `--reps` repetitions alternating; min and spread ((max - min) / min), fields per second
and us per field-iteration of the batch, and whether both routes left equal fields (u, iteration count, delta).  Then forced rows: the
LDS capacity of the batched bricks forced to 288 and 576 rows (EPIC_HIP_BATCH_BRICK_ROWS) and their shell depth to 2, 3 and 4
(EPIC_HIP_BATCH_HALO).  `--loop-only` prints the loop column alone: run against the parent commit's library (EPIC_LIB) it confirms the
baseline.  `--resident` times epic_hip_execute_batch_gpu against a loop of harmonic_execute_gpu on fields that are already on the device
(the three initialisations and releases outside the timing): the relaxation without the uploads, which is where the kernels show.

    python tools/bench_batch_3d.py [--shapes 16x16x16,32x32x32,64x64x64,96x96x96,128x128x128,64x64x200] [--fields 2,4,8,16,32,64]
                                   [--eps 1e-3,1e-6] [--forced-rows 288,576] [--forced-halo 2,3,4] [--forced-fields 2,8,32] [--loop-only] [--resident]
profiles/batch_3d.txt is this tool's output.
"""
import argparse
import os
import sys
import time

os.environ.setdefault("EPIC_HIP_STUDY", "1")   # this tool steers the kernel plan with study knobs (epic_amd/csrc/driver_config.cpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KNOBS = ("EPIC_HIP_BATCH_BRICK_ROWS", "EPIC_HIP_BATCH_HALO")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16x16,32x32x32,64x64x64,96x96x96,128x128x128,64x64x200")
    ap.add_argument("--fields", default="2,4,8,16,32,64")
    ap.add_argument("--eps", default="1e-3,1e-6")
    ap.add_argument("--forced-rows", default="288,576", help="LDS capacities of the forced-plan rows")
    ap.add_argument("--forced-halo", default="2,3,4", help="shell depths of the forced-plan rows")
    ap.add_argument("--forced-fields", default="2,8,32", help="B of the forced-plan rows")
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--resident", action="store_true")
    args = ap.parse_args()
    from epic_amd import epic_harmonic as eh
    from epic_amd.harmonic import Harmonic
    from epic_amd.synthetic import synthetic_grid

    E = eh._epic
    for knob in ("EPIC_HIP_SCHEME", "EPIC_HIP_MATH") + KNOBS:
        os.environ.pop(knob, None)
    # every row measures the BATCH, also where the shipped crossover (batch3d_from_fields) keeps the loop: a forced fields-per-workgroup
    # (1, the only value of the 3-D bricks) batches from two fields everywhere, as in tools/bench_batch_2d.py's forced rows
    os.environ["EPIC_HIP_BATCH_FIELDS"] = "1"

    def stat(v):
        return "%9.4f (+%4.1f %%)" % (min(v), 100.0 * (max(v) - min(v)) / min(v))

    def make(m, u0, locked0, goals, eps):
        out = []
        for g in goals:
            u, locked = u0.copy(), locked0.copy()
            u[g], locked[g] = 0.0, 1
            h = Harmonic()
            h.set_grid(m, u, locked)
            h.epsilon, h.numIterationsToStaggerCheck = eps, 100
            out.append(h)
        return out

    INIT = (E.harmonic_initialize_dimension_size_gpu, E.harmonic_initialize_potential_values_gpu, E.harmonic_initialize_locked_gpu)
    UNINIT = (E.harmonic_uninitialize_dimension_size_gpu, E.harmonic_uninitialize_potential_values_gpu, E.harmonic_uninitialize_locked_gpu)

    def batch(fields):
        return (E.epic_hip_execute_batch_gpu if args.resident else E.epic_hip_complete_batch_gpu)(eh.field_array(fields), len(fields), 1024, None)

    def loop(fields):
        return max((E.harmonic_execute_gpu if args.resident else E.harmonic_complete_gpu)(h, 1024) for h in fields)

    def row(name, m, u0, locked0, goals, eps, **forced):
        for knob in KNOBS:
            os.environ.pop(knob, None)
        for knob, v in forced.items():
            os.environ[knob] = str(v)
        routes = (("loop", loop),) if args.loop_only else (("batch", batch), ("loop", loop))
        sec, done, plan = {"batch": [], "loop": []}, {}, None
        for rep in range(args.reps):
            for route, run in routes:
                fields = make(m, u0, locked0, goals, eps)
                if route == "batch" and plan is None:   # what the call will do, asked of resident fields outside the timing
                    for h in fields:
                        assert E.harmonic_initialize_dimension_size_gpu(h) == 0 and E.harmonic_initialize_potential_values_gpu(h) == 0
                        assert E.harmonic_initialize_locked_gpu(h) == 0
                    plan = eh.batch_plan(fields)
                    for h in fields:
                        assert E.harmonic_uninitialize_dimension_size_gpu(h) == 0 and E.harmonic_uninitialize_potential_values_gpu(h) == 0
                        assert E.harmonic_uninitialize_locked_gpu(h) == 0
                if args.resident:
                    for h in fields:
                        assert all(fn(h) == 0 for fn in INIT)
                t0 = time.perf_counter()
                assert run(fields) == 0
                sec[route].append(time.perf_counter() - t0)
                if args.resident:
                    for h in fields:
                        assert all(fn(h) == 0 for fn in UNINIT)
                done[route] = [(h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta)) for h in fields]
        its = sum(d[1] for d in done["loop"])
        tag = " ".join("%s=%s" % (k.replace("EPIC_HIP_BATCH_", "").lower(), v) for k, v in forced.items()) or "default"
        if args.loop_only:
            print("  %-11s %-16s %5g %3d %-18s | %-20s %-20s %6s | %9s %8s %9d | %s" % (name, tag, eps, len(goals), "-", "-", stat(sec["loop"]), "-", "-", "-", its, "-"),
                  flush=True)
            return
        equal = all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(done["batch"], done["loop"]))
        p = "H=%d %dx%d" % (plan["halo"], plan["tile_rows"], plan["tile_cols"]) if plan["batched"] else "loop"
        print("  %-11s %-16s %5g %3d %-18s | %-20s %-20s %6.2f | %9.1f %8.3f %9d | %s" % (
            name, tag, eps, len(goals), p, stat(sec["batch"]), stat(sec["loop"]), min(sec["loop"]) / min(sec["batch"]), len(goals) / min(sec["batch"]),
            min(sec["batch"]) / its * 1e6, its, equal), flush=True)

    print("# seconds of epic_hip_%s_batch_gpu and of a loop of harmonic_%s_gpu over the same fields; min of %d (spread); stagger 100; "
          "obstacle density %g%s" % (("execute", "execute", args.reps, args.density, "; fields resident, uploads outside the timing") if args.resident
                                     else ("complete", "complete", args.reps, args.density, "")))
    print("# %-11s %-16s %5s %3s %-18s | %-20s %-20s %6s | %9s %8s %9s | %s" % ("shape", "plan", "eps", "B", "batch plan (S0xS1)", "s batch", "s loop", "ratio",
                                                                                 "fields/s", "us/f-it", "f-iters", "equal"))
    for name in args.shapes.split(","):
        m = [int(x) for x in name.split("x")]
        u0, locked0 = synthetic_grid(m, 20240601, args.density)
        goal = (u0 == 0.0) & (locked0 != 0)
        u0[goal], locked0[goal] = -1e6, 0    # the generator's own goal becomes a free cell
        free = np.flatnonzero(locked0 == 0)
        goals = np.random.default_rng(20240601).choice(free, size=64, replace=False)
        for eps in [float(e) for e in args.eps.split(",") if e]:
            for b in [int(x) for x in args.fields.split(",") if x]:
                row(name, m, u0, locked0, goals[:b], eps)
            if args.loop_only:
                continue
            for b in [int(x) for x in args.forced_fields.split(",") if x]:
                for r in [int(x) for x in args.forced_rows.split(",") if x]:
                    row(name, m, u0, locked0, goals[:b], eps, EPIC_HIP_BATCH_BRICK_ROWS=r)
                for h in [int(x) for x in args.forced_halo.split(",") if x]:
                    row(name, m, u0, locked0, goals[:b], eps, EPIC_HIP_BATCH_HALO=h)


if __name__ == "__main__":
    main()
