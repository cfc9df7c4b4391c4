#!/usr/bin/env python3
"""One application of the cell update against its exact value, recorded for the checker's two arithmetics.

Runs oracle/liboracle.so only (this project's own checker: the reference's rounding sequence, oracle_jacobi_run, and the tol
arithmetic, oracle_tol_run) over the regimes of tests/update_accuracy_cases.py, 2-D and 3-D, and writes
tests/golden/update_accuracy.json: per regime the statistics of both arithmetics against the exact value, tol paired with the
reference arithmetic, the two excesses the conditions of tests/test_update_accuracy_cpu.py are built on, and the sha256 of the input
field (so that a changed generator shows); at the top `max_excess_margin`, the largest max_excess rounded up to the next half unit.
Seconds on a CPU; deterministic, so a second run reproduces the file byte for byte.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import update_accuracy_cases as C  # noqa: E402


def main(path=C.GOLDEN):
    if not C.longdouble_is_80_bit():
        sys.exit("numpy.longdouble has fewer than 64 significand bits here: the exact values need them")
    out = {"samples": {str(d): int(C.np.prod(C.BLOCKS[d])) for d in (2, 3)}, "rng_seed": C.RNG_SEED, "regimes": {}}
    for dim, name in C.CASES:
        c = C.Case(dim, name)
        rec = c.measure(c.checker("ref"), c.checker("tol"))
        rec["sha256"] = c.sha256
        out["regimes"]["%dd/%s" % (dim, name)] = rec
        print(C.table_row("%dd/%s" % (dim, name), "ref", rec["ref"]))
        print(C.table_row("", "tol", rec["tol"], rec["paired"]))
    worst = max(out["regimes"].items(), key=lambda kv: kv[1]["max_excess"])
    out["max_excess_largest"] = {"regime": worst[0], "value": worst[1]["max_excess"]}
    out["max_excess_margin"] = C.half_unit_up(worst[1]["max_excess"])
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("max_excess_margin %.1f (largest excess %.4f in %s)" % (out["max_excess_margin"], worst[1]["max_excess"], worst[0]))


if __name__ == "__main__":
    main(*sys.argv[1:])
