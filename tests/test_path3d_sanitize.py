"""The host statement of the 3-D consumers and edits (epic_amd/csrc/harmonic_path3d_cpu.cpp) as a stand-alone program under
AddressSanitizer and UBSan (tests/sanitize/path3d_main.cpp): exactly-sized arrays, walks from every interior cell (with a step long
enough to leave the grid), starts on goal cells of a face and of the far corner with cdPrecision 1.5, sparse edits over every cell
and outside, the error returns.  Host code only; nothing here touches a GPU or is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_host_walk_3d_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "path3d_main")
    csrc = os.path.join(ROOT, "epic_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "sanitize", "path3d_main.cpp"), os.path.join(csrc, "harmonic_path3d_cpu.cpp"),
                    os.path.join(csrc, "harmonic_path_cpu.cpp"), "-o", exe], check=True)   # (harmonic_path_cpu.cpp: harmonic_free_path_cpu)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "3-D path host code: ok" in run.stdout
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error", "EXPECT failed"):
        assert bad not in run.stderr, run.stderr[-2000:]
