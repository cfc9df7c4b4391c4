"""The host twins of the field queries (epic_amd/csrc/field_query_cpu.cpp) as a stand-alone program under AddressSanitizer and UBSan
(tests/sanitize/field_query_main.cpp): exactly-sized arrays, samples at and beside every cell with cdPrecision up to 1.5, goals on a
face and in both corners, the edge coordinates (NaN, +-inf, negative, |x| >= 2^63), regions in both corners, the error returns.
Host code only; nothing here touches a GPU or is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_field_query_twins_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "field_query_main")
    csrc = os.path.join(ROOT, "epic_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
                    "-fno-sanitize-recover=undefined,float-cast-overflow", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sanitize", "field_query_main.cpp"),
                    os.path.join(csrc, "field_query_cpu.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "field query host code: ok" in run.stdout
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed"):
        assert bad not in run.stderr, run.stderr[-2000:]
