"""`python3 bench.py --gpus N` typed as is -- no torch.distributed.run in front, the way the driver's scaling run types it --
must start its own ranks and print ONE line.  On the one GPU of this box the ranks share the device and trade their halo rows
over gloo (EPIC_BENCH_BACKEND=gloo), and the in-library leg runs its slabs on device 0 twice (EPIC_BENCH_DEVLIST=0,0): the same
code paths as on a node with N devices, minus the links."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def test_plain_command_with_two_gpus_launches_its_own_ranks():
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "EPIC_HIP_SCHEME", "EPIC_HIP_MATH")}
    env.update({"EPIC_BENCH_BACKEND": "gloo", "EPIC_BENCH_DEVLIST": "0,0"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--develop", "2000", "--full"], env=env, capture_output=True, text=True, timeout=840, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]       # ONE JSON line, nothing else on stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    ranks = d["ranks"]
    assert ranks["ranks_seen"] == 2 and ranks["backend"] == "gloo"
    assert sorted(x["rank"] for x in ranks["per_rank"]) == [0, 1] and len({x["pid"] for x in ranks["per_rank"]}) == 2
    assert "in_library" in d and "error" not in d["in_library"], d.get("in_library")
    assert d["in_library"]["slabs"] == 2 and d["in_library"]["value"] > 0
    assert d["roofline"]["bound"] in ("hbm", "valu") and d["roofline"]["frac"] > 0


def test_plain_run_times_its_steps_dumps_the_last_field_and_runs_no_evidence_leg(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` is the headline and nothing beside it (the evidence legs are --full's); with
    --dump-outputs it leaves the field of the last timed step and the delta of its check, the same values in every run."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("EPIC_HIP_SCHEME", "EPIC_HIP_MATH")}
    fields = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "2048",
                            "--develop", "1000", "--dump-outputs", str(tmp_path / name)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["unit"] == "Mcell-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        for leg in ("roofline", "kernels", "cpu_baseline", "relax", "relax_default", "parity", "config4", "config5", "maps", "node_flow"):
            assert leg not in d, leg
        u, delta = np.load(tmp_path / name / "u.npy"), np.load(tmp_path / name / "delta.npy")
        assert u.dtype == np.float32 and u.shape == (2048 * 2048,) and delta.dtype == np.float64 and delta.shape == (1,)
        assert np.isfinite(u).all() and (u > -9e5).sum() > 1000 and 0.0 < delta[0] <= 1e6     # a developed field, not the initial one
        fields.append((u, delta))
    assert np.array_equal(fields[0][0], fields[1][0]) and fields[0][1][0] == fields[1][1][0]
