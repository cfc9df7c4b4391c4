"""Several fields on one map: epic_hip_complete_batch_gpu against the loop of harmonic_complete_gpu it replaces, same process, alternating.

Per map (tests/golden/maps), epsilon and number of fields B -- every field has the map's obstacles and ONE goal of its own, a free cell
drawn from a fixed seed -- the wall time of either route, `--reps` repetitions alternating; min and spread ((max - min) / min), fields
per second and us per field-iteration of the batch, and whether both routes left equal fields (u, iteration count, delta).  Then the
same with the fields per workgroup forced to 1, 2 and 4 (EPIC_HIP_BATCH_FIELDS), so that the interleave's worth is visible on its own,
and with the tile width forced to 64 and 128 columns (EPIC_HIP_BATCH_WIDTH), fields per workgroup 1, for the wide tile's.

    python tools/bench_batch_2d.py [--maps basic,maze,umass] [--fields 1,2,4,8,16,32,64] [--eps 1e-3,1e-6] [--forced 1,2,4] [--forced-width 64,128] [--forced-fields 2,8,32]
                                   [--math precise|tol|fast] [--scheme redblack|jacobi]
profiles/batch_2d.txt is this tool's output; profiles/batch_2d_modes.txt its output with --math / --scheme, where the batch is forced
(EPIC_HIP_BATCH=1: those modes' groups are off by default) and the loop is harmonic_complete_gpu in the same mode.
"""
import argparse
import os
import sys
import time

os.environ.setdefault("EPIC_HIP_STUDY", "1")   # this tool steers the kernel plan with study knobs (epic_amd/csrc/driver_config.cpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="basic,maze,umass")
    ap.add_argument("--fields", default="1,2,4,8,16,32,64")
    ap.add_argument("--eps", default="1e-3,1e-6")
    ap.add_argument("--forced", default="1,2,4", help="fields per workgroup of the forced-plan rows")
    ap.add_argument("--forced-width", default="64,128", help="tile widths of the forced-plan rows (one field per workgroup)")
    ap.add_argument("--forced-fields", default="2,8,32", help="B of the forced-plan rows")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--math", default="precise")
    ap.add_argument("--scheme", default="redblack")
    args = ap.parse_args()
    from epic_amd import epic_harmonic as eh
    from epic_amd.harmonic import Harmonic
    from epic_amd.harmonic_map import HarmonicMap

    E = eh._epic
    for knob in ("EPIC_HIP_SCHEME", "EPIC_HIP_MATH", "EPIC_HIP_BATCH_FIELDS", "EPIC_HIP_BATCH_WIDTH"):
        os.environ.pop(knob, None)
    if (args.math, args.scheme) != ("precise", "redblack"):
        os.environ.update(EPIC_HIP_MATH=args.math, EPIC_HIP_SCHEME=args.scheme, EPIC_HIP_BATCH="1")
        print("# math %s, scheme %s, batch forced" % (args.math, args.scheme))

    def stat(v):
        return "%9.4f (+%4.1f %%)" % (min(v), 100.0 * (max(v) - min(v)) / min(v))

    def make(base, goals, eps):
        out = []
        for g in goals:
            u, locked = base.u_array().ravel().copy(), base.locked_array().ravel().copy()
            goal = (u == 0.0) & (locked != 0)
            u[goal], locked[goal] = -1e6, 0    # the map's own goals become free cells
            u[g], locked[g] = 0.0, 1
            h = Harmonic()
            h.set_grid(list(base.shape), u, locked)
            h.epsilon, h.numIterationsToStaggerCheck = eps, 100
            out.append(h)
        return out

    def batch(fields):
        return E.epic_hip_complete_batch_gpu(eh.field_array(fields), len(fields), 1024, None)

    def loop(fields):
        return max(E.harmonic_complete_gpu(h, 1024) for h in fields)

    def row(name, base, goals, eps, forced, width=0):
        os.environ.pop("EPIC_HIP_BATCH_FIELDS", None)
        os.environ.pop("EPIC_HIP_BATCH_WIDTH", None)
        if forced:
            os.environ["EPIC_HIP_BATCH_FIELDS"] = str(forced)
        if width:
            os.environ["EPIC_HIP_BATCH_WIDTH"] = str(width)
        sec, done, plan = {"batch": [], "loop": []}, {}, None
        for rep in range(args.reps):
            for route, run in (("batch", batch), ("loop", loop)):
                fields = make(base, goals, eps)
                if route == "batch" and plan is None:   # what the call will do, asked of resident fields outside the timing
                    for h in fields:
                        assert E.harmonic_initialize_dimension_size_gpu(h) == 0 and E.harmonic_initialize_potential_values_gpu(h) == 0
                        assert E.harmonic_initialize_locked_gpu(h) == 0
                    plan = eh.batch_plan(fields)
                    for h in fields:
                        assert E.harmonic_uninitialize_dimension_size_gpu(h) == 0 and E.harmonic_uninitialize_potential_values_gpu(h) == 0
                        assert E.harmonic_uninitialize_locked_gpu(h) == 0
                t0 = time.perf_counter()
                assert run(fields) == 0
                sec[route].append(time.perf_counter() - t0)
                done[route] = [(h.u_array().ravel().copy(), int(h.currentIteration), float(h.delta)) for h in fields]
        equal = all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(done["batch"], done["loop"]))
        its = sum(d[1] for d in done["batch"])
        p = "F=%d H=%d %dx%d" % (plan["fields_per_workgroup"], plan["halo"], plan["tile_rows"], plan["tile_cols"]) if plan["batched"] else "loop"
        print("  %-6s %-9s %5g %3d %-16s | %-20s %-20s %6.2f | %9.1f %8.3f %9d | %s" % (
            name, ("F=%d" % forced + (" W=%d" % width if width else "")) if forced else "default", eps, len(goals), p, stat(sec["batch"]), stat(sec["loop"]),
            min(sec["loop"]) / min(sec["batch"]), len(goals) / min(sec["batch"]), min(sec["batch"]) / its * 1e6, its, equal), flush=True)

    print("# seconds of epic_hip_complete_batch_gpu and of a loop of harmonic_complete_gpu over the same fields; min of %d (spread); stagger 100" % args.reps)
    print("# %-6s %-9s %5s %3s %-16s | %-20s %-20s %6s | %9s %8s %9s | %s" % ("map", "plan", "eps", "B", "batch plan", "s batch", "s loop", "ratio",
                                                                              "fields/s", "us/f-it", "f-iters", "equal"))
    for name in args.maps.split(","):
        base = HarmonicMap().load(os.path.join(ROOT, "tests", "golden", "maps", name + ".png"))
        free = np.flatnonzero(base.locked_array().ravel() == 0)
        goals = np.random.default_rng(20240601).choice(free, size=64, replace=False)
        for eps in [float(e) for e in args.eps.split(",")]:
            for b in [int(x) for x in args.fields.split(",") if x]:
                row(name, base, goals[:b], eps, 0)
            for b in [int(x) for x in args.forced_fields.split(",") if x]:
                for f in [int(x) for x in args.forced.split(",") if x]:
                    row(name, base, goals[:b], eps, f)
                for w in [int(x) for x in args.forced_width.split(",") if x]:
                    row(name, base, goals[:b], eps, 1, w)


if __name__ == "__main__":
    main()
