"""bench.py's plain run: it times exactly --steps updates, its line carries the headline alone (the other legs are --full's), and
--dump-outputs writes what the timed path computed in its last step -- held here to the C oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import TOL_NORTH_STAR, rel
from x_multi_agent_amd import fleet, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("config", [4, 2])
def test_plain_run_dumps_what_its_last_step_computed(oracle_c, tmp_path, config):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--config", str(config),
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "updates/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3
    assert not {"roofline", "frame_loop", "other_configs", "nominal_rows", "small_frames", "parity", "cpu_baseline"} & set(d)

    got = {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"P", "correction", "inlier", "gamma"} | ({"inlier_slam", "gamma_slam"} if config == 2 else set())
    assert all(a.dtype == np.float64 for a in got.values())
    ref = oracle_c.visual_update(fleet.shared_scenario(synth, config, 0))
    assert np.array_equal(got["inlier"], ref["inlier"]), "MSCKF inlier masks differ"
    if config == 2:
        assert np.array_equal(got["inlier_slam"], ref["inlier_slam"])
    fin = np.isfinite(ref["gamma"])
    assert rel(got["gamma"][fin], ref["gamma"][fin]) <= 1e-8
    rp, rc = rel(got["P"], ref["P"]), rel(got["correction"], ref["correction"])
    assert rp <= 1e-8 and rp <= TOL_NORTH_STAR, rp
    assert rc <= 1e-7, rc
