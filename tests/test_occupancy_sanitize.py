"""The host half of the dense occupancy ingestion (epic_amd/csrc/occupancy_cpu.cpp with the rule of occupancy_rule.h) as a
stand-alone program under AddressSanitizer and UBSan (tests/sanitize/occupancy_main.cpp): exactly-sized arrays, odd shapes, every
flag combination, the error returns.  Host code only; nothing here touches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_walk_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "occupancy_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "sanitize", "occupancy_main.cpp"),
                    os.path.join(ROOT, "epic_amd", "csrc", "occupancy_cpu.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "occupancy host code: ok" in run.stdout
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed"):
        assert bad not in run.stderr, run.stderr[-2000:]
