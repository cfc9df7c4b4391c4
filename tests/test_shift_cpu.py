"""epic_hip_shift_field_cpu (include/epic_hip.h; epic_amd/csrc/field_shift_cpu.cpp, field_shift_rule.h) against a numpy slicing statement of
the rule, bit for bit: u, locked, kept, the untouched border and faces; the error returns; the host code under AddressSanitizer and UBSan
in a program of its own (tests/sanitize/field_shift_main.cpp)."""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

from epic_amd import epic_harmonic as eh
from epic_amd.harmonic import Harmonic
from epic_amd.synthetic import synthetic_grid

E = eh._epic
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -2 ** 31
FREE, OBSTACLE, BAD = eh.EPIC_CELL_TYPE_FREE, eh.EPIC_CELL_TYPE_OBSTACLE, eh.EPIC_ERROR_INVALID_DATA


def shifts_for(m):
    """zero; +-1 on each axis; the two misaligned diagonals; a column shift of a whole strip; |shift| = m - 2 (all uncovered); INT_MIN"""
    n, lead = len(m), (1,) * (len(m) - 2)
    unit = [tuple(s if a == i else 0 for a in range(n)) for i in range(n) for s in (1, -1)]
    return [(0,) * n] + unit + [lead + (3, -33), lead + (-2, 31), lead + (1, 256), (m[0] - 2,) + (0,) * (n - 1), (0,) * (n - 1) + (INT_MIN,)]


def seeded_field(m):
    """The synthetic grid (border locked, 5 % obstacles, a goal in the centre) with a second goal at (2, ..., 2) -- the unit shifts keep
    both, the diagonals drop one -- and a value of its own in every free cell, so that a cell in the wrong place shows."""
    u, locked = (a.reshape(m) for a in synthetic_grid(list(m), 20240601, 0.05))
    u[(2,) * len(m)], locked[(2,) * len(m)] = 0.0, 1
    free = locked == 0
    u[free] = -(1.0 + (np.flatnonzero(free.ravel()) * 7919 % 4096) / 16.0).astype(np.float32)
    return u.ravel().copy(), locked.ravel().copy()


def numpy_shift(m, u, locked, shift, fill):
    """The rule by slices of the interior: new[x] = old[x + shift] where both are interior, the fill elsewhere.  Returns (u, locked, kept)."""
    u, locked = u.reshape(m).copy(), locked.reshape(m).copy()
    inner = tuple(slice(1, d - 1) for d in m)
    old_u, old_l = u[inner].copy(), locked[inner].copy()
    u[inner], locked[inner] = np.float32(-1e6), int(fill == OBSTACLE)
    spans = [(max(0, -s), min(d - 2, d - 2 - s)) for d, s in zip(m, shift)]
    kept = int(np.prod([max(0, hi - lo) for lo, hi in spans], dtype=object))
    if kept:
        dst = tuple(slice(lo, hi) for lo, hi in spans)
        src = tuple(slice(lo + s, hi + s) for (lo, hi), s in zip(spans, shift))
        u[inner][dst], locked[inner][dst] = old_u[src], old_l[src]
    return u.ravel(), locked.ravel(), kept


def make(m, u, locked):
    h = Harmonic()
    h.set_grid(list(m), u, locked)
    return h


def call(fn, h, shift, fill, *tail):
    kept = ct.c_ulonglong(777)
    return fn(h, None if shift is None else (ct.c_int * len(shift))(*shift), fill, ct.byref(kept), *tail), kept.value


def bits(a):
    return np.asarray(a, dtype=np.float32).ravel().view(np.uint32)


@pytest.mark.parametrize("fill", [FREE, OBSTACLE], ids=["free", "obstacle"])
@pytest.mark.parametrize("m", [(5, 5), (37, 300), (6, 7, 70)], ids=lambda m: "x".join(map(str, m)))
def test_shift_cpu_equals_the_numpy_slices(m, fill):
    u0, l0 = seeded_field(m)
    u0.view(np.uint32)[np.ravel_multi_index((1,) * len(m), m)] = 0x7fc12345   # a NaN payload survives a copy of bit patterns
    goals = []
    for shift in shifts_for(m):
        h = make(m, u0, l0)
        rc, kept = call(E.epic_hip_shift_field_cpu, h, shift, fill)
        want_u, want_l, want_kept = numpy_shift(m, u0, l0, shift, fill)
        assert rc == 0 and kept == want_kept == (0 if max(map(abs, shift)) > 256 or abs(shift[0]) == m[0] - 2 else kept), (shift, kept, want_kept)
        assert np.array_equal(bits(h.u_array()), bits(want_u)) and np.array_equal(h.locked_array().ravel(), want_l), shift
        goals.append(int(((want_u == 0) & (want_l != 0)).sum()))
    assert goals[0] == goals[1] > min(goals[1:]) and np.array_equal(bits(numpy_shift(m, u0, l0, shifts_for(m)[0], fill)[0]), bits(u0))
    assert E.epic_hip_shift_field_cpu(make(m, u0, l0), (ct.c_int * len(m))(*([1] * len(m))), fill, None) == 0   # kept may be NULL


def test_invalid_arguments_touch_nothing(capfd):
    m = (6, 7, 70)
    u0, l0 = seeded_field(m)
    h = make(m, u0, l0)
    no_u, no_locked, no_m, four_d = make(m, u0, l0), make(m, u0, l0), make(m, u0, l0), make((3, 3, 3, 3), np.zeros(81), np.ones(81))
    no_u.u, no_locked.locked, no_m.m = ct.POINTER(ct.c_float)(), ct.POINTER(ct.c_uint)(), ct.POINTER(ct.c_uint)()
    for who, shift, fill in [(None, (1, 1, 1), FREE), (h, None, FREE), (h, (1, 1, 1), eh.EPIC_CELL_TYPE_GOAL), (h, (1, 1, 1), 3), (no_u, (1, 1, 1), FREE),
                             (no_locked, (1, 1, 1), FREE), (no_m, (1, 1, 1), FREE), (four_d, (1, 1, 1, 1), FREE), (make((9,), np.zeros(9), np.ones(9)), (1,), FREE)]:
        assert call(E.epic_hip_shift_field_cpu, who, shift, fill) == (BAD, 777)
        assert "Error[epic_hip_shift_field_cpu]: Invalid data." in capfd.readouterr().err
    assert np.array_equal(bits(h.u_array()), bits(u0)) and np.array_equal(h.locked_array().ravel(), l0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    build = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-ffp-contract=off"]
    (tmp_path / "probe.cpp").write_text("int main() { return 0; }\n")
    if (subprocess.run([*build, str(tmp_path / "probe.cpp"), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0):
        pytest.skip("this g++ has no sanitizer runtime that runs here")
    exe = str(tmp_path / "field_shift_main")
    subprocess.run([*build, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "field_shift_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and "field shift host code: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert not any(word in run.stderr for word in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed")), run.stderr[-2000:]
