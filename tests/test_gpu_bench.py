"""bench.py as its users call it, in a fresh child process per run (never a re-exec of the pytest process, which has
initialised the GPU).  A plain run prints the contract's one JSON line with every side leg null and dumps the last timed
step; --full runs the side legs as well, around the same timed steps, whose outputs are bit for bit the plain run's.
BASELINE config 2 and short side legs keep both runs small."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("full_panel", "config4", "direct_route", "rotated_kinship_factor", "donor_collapsed", "cpu_baseline")


def _bench(dest, *flags):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg2", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(dest), *flags]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(dest, k + ".npy")) for k in ("pv", "rho1", "Q")}


def test_plain_run_times_the_headline_alone_and_full_adds_the_side_legs(tmp_path):
    plain, dumped = _bench(tmp_path / "plain")
    assert plain["metric"] == "variant-tests/sec (interaction test)" and plain["unit"] == "variant-tests/s"
    assert plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert (plain["n_gpus"], plain["steps"], plain["warmup"]) == (1, 2, 1)
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert [k for k in SIDE_LEGS if plain[k] is not None] == []
    assert plain["speedup_vs_cpu_baseline"] is None
    assert all(v.shape == (4096,) for v in dumped.values())

    full, dumped_full = _bench(tmp_path / "full", "--full", "--cpu-variants", "2", "--cpu-repeats", "1", "--genes", "2",
                               "--genes-variants", "512", "--direct-steps", "1", "--rotated-steps", "1")
    # (the direct-route leg runs where the headline takes the kinship-structure route)
    expected = [k for k in SIDE_LEGS if k != "direct_route" or full["config"]["route"].startswith("kinship")]
    assert [k for k in expected if full[k] is None] == []
    # the timed steps scan the same panel with or without the side legs around them
    for k in dumped:
        assert np.array_equal(dumped[k], dumped_full[k]), k
