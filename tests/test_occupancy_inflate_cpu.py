"""epic_hip_set_occupancy_inflated_cpu (include/epic_hip.h; epic_amd/csrc/occupancy_cpu.cpp, occupancy_rule.h) against the reference of
occupancy_inflate_cases.py -- B' by brute force through the existing epic_hip_set_occupancy_region_cpu --, bit for bit."""
import numpy as np
import pytest

import occupancy_inflate_cases as I
from epic_amd import epic_harmonic as eh

INFLATED = dict(fn=eh._epic.epic_hip_set_occupancy_inflated_cpu)


@pytest.mark.parametrize("r2", I.RADII)
@pytest.mark.parametrize("pattern", ["marks", "sprinkle"])
@pytest.mark.parametrize("geom", I.GEOMS)
def test_inflated_cpu_equals_the_region_call_on_the_brute_force_block(geom, pattern, r2):
    m, _, _, where = I.region(geom)
    for flavour, (rule, _, _) in I.FLAVOURS.items():
        got = I.region_cpu(m, I.block(geom, pattern, flavour), *where, **rule, **INFLATED, r2=(r2,))
        assert I.same(got, I.expected(geom, pattern, flavour, r2)), flavour


def test_a_radius_past_the_limit_touches_nothing(capfd):
    m, _, _, where = I.region("2d-tiny")
    got = I.region_cpu(m, I.block("2d-tiny", "marks", "node"), *where, **I.C.NODE, **INFLATED, r2=(257,), expect=eh.EPIC_ERROR_INVALID_DATA)
    assert "Error[epic_hip_set_occupancy_inflated_cpu]: Invalid data." in capfd.readouterr().err and I.same(got, I.state(m) + (777,))
