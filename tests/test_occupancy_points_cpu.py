"""epic_hip_set_occupancy_points_cpu (include/epic_hip.h; epic_amd/csrc/occupancy_points_cpu.cpp, occupancy_points_rule.h) against the numpy
statement of occupancy_points_cases.py through the existing epic_hip_set_occupancy_inflated_cpu, bit for bit; the rays against their segments
in float64; the error returns; the rule's host code under AddressSanitizer and UBSan in a program of its own."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import occupancy_points_cases as P
from epic_amd import epic_harmonic as eh

I = P.I
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sensor", P.SENSORS)
@pytest.mark.parametrize("geom", P.GEOMS)
def test_points_cpu_equals_the_inflated_call_on_the_numpy_block(geom, sensor):
    m, _, _, where = P.box(geom)
    points, s = P.cloud(geom, 65, sensor)
    block = functools.lru_cache(maxsize=None)(lambda no_change, flags: P.block(geom, points, s, no_change, flags))
    results = []
    for r2, rule in P.RULES:
        want = I.region_cpu(m, block(rule["no_change"], rule["flags"]), *where, **rule, fn=eh._epic.epic_hip_set_occupancy_inflated_cpu, r2=(r2,))
        results.append(P.twin(geom, points, s, r2, rule))
        assert I.same(results[-1], want) and want[2] > 0, (r2, rule)
    if geom.endswith("129") and sensor == "corner":   # a goal lies under a ray: OVER_GOALS frees it, the node's rule leaves it
        assert not I.same(results[2], results[3])


@pytest.mark.parametrize("geom", ["2d-129", "3d-129", "3d-grid"])
def test_every_cleared_cell_meets_its_segment(geom):
    """float64: the closed cube of a cleared cell, grown by MARGIN, meets the segment sensor -> point (so no cell farther than that from every
    segment is cleared).  MARGIN covers the f32 rounding of tMax: two boundaries the walk takes in the wrong order lie that close together."""
    MARGIN = 1e-4
    _, o, e, _ = P.box(geom)
    points, s = P.cloud(geom, 65, "corner")
    s64, cleared = s[::-1].astype(np.float64), 0
    for p in points[np.all(np.isfinite(points), axis=1)][:, ::-1]:
        d = p.astype(np.float64) - s64
        for c in np.array(list(P.ray_cells(o, e, s[::-1], p))).reshape(-1, len(o)):
            with np.errstate(all="ignore"):
                t0, t1 = (c - MARGIN - s64) / d, (c + 1 + MARGIN - s64) / d
            flat = d == 0   # the segment does not move along this axis: it lies inside the cell's slab
            assert np.all(((c - MARGIN <= s64) & (s64 <= c + 1 + MARGIN))[flat])
            assert max(np.minimum(t0, t1)[~flat].max(initial=0.0), 0.0) <= min(np.maximum(t0, t1)[~flat].min(initial=1.0), 1.0), (p, c)
            cleared += 1
    assert cleared > 500


@pytest.mark.parametrize("bad", P.bad_calls("2d-65"))
@pytest.mark.parametrize("geom", ["2d-65", "3d-65"])
def test_invalid_arguments_touch_nothing(geom, bad, capfd):
    got = P.twin(geom, **P.bad_calls(geom)[bad], expect=eh.EPIC_ERROR_INVALID_DATA)
    assert "Error[epic_hip_set_occupancy_points_cpu]: Invalid data." in capfd.readouterr().err and I.same(got, I.state(P.box(geom)[0]) + (777,))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_rule_is_clean_under_asan_and_ubsan(tmp_path):
    build = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off"]
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    if (subprocess.run([*build, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0):
        pytest.skip("this g++ has no sanitizer runtime that runs here")
    exe = str(tmp_path / "occupancy_points_main")
    subprocess.run([*build, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "occupancy_points_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and "occupancy points host code: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert not any(word in run.stderr for word in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed")), run.stderr[-2000:]
