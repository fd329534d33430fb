"""bench.py as a plain run on the GPU (100^3 grid_nodes: 50x50x100 cells, a few steps): the result
line's headline fields, what stays behind --full, and --dump-outputs.

The timed steps are attempted steps W+1 .. W+K from the initial condition whatever the clock
pre-warm ran before them, so two runs dump the same bits, and those are the bits a Simulation
stepped W then K attempted steps from the (host) initial condition holds.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P
from porousfreezethaw_amd import params as PR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
GN, W, K = 100, 3, 7
ARGS = ["--gpus", "1", "--grid-nodes", str(GN), "--steps", str(K), "--warmup", str(W), "--prewarm-s", "0.05"]


def _bench(extra):
    r = subprocess.run([sys.executable, BENCH] + ARGS + extra, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("\n") == 1                    # exactly one line on stdout
    return json.loads(r.stdout)


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_state_after_the_timed_steps(tmp_path):
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")
    base = PR.default_params(grid_nodes=GN)
    cells = base["n1"] * base["n2"] * base["n3"]
    outs = [_bench(["--dump-outputs", str(tmp_path / d)]) for d in "ab"]
    for out in outs:
        assert out["steps"] == K and out["warmup"] == W
        assert out["unit"] == "Mcells·steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        ms = out["ms_per_step"]
        assert ms > 0
        # value = cells / ms_per_step; both are rounded on the line (ms to 1e-4, value to 1e-2)
        assert cells / 1e3 / (ms + 0.5e-4) - 0.01 <= out["value"] <= cells / 1e3 / (ms - 0.5e-4) + 0.01
        assert out["roofline"] is None and out["cpu_baseline"] is None and out["parity"] is None
        assert out["config"]["clock_prewarm"]["attempted_steps"] >= 20      # there was a state to drop
        assert out["config"]["accepted_steps_total"] <= W + K
    xa, xb = (np.load(tmp_path / d / "x.npy") for d in "ab")
    ta, tb = (np.load(tmp_path / d / "trajectory.npy") for d in "ab")
    assert xa.dtype == np.float64 and ta.dtype == np.float64
    assert sorted(os.listdir(tmp_path / "a")) == ["trajectory.npy", "x.npy"]
    assert np.array_equal(xa, xb) and np.array_equal(ta, tb)

    sim = P.Simulation(base["n1"], base["n2"], base["n3"], (base["L1"], base["L2"], base["L3"]), 0,
                       P.params_array(base), beads=O.beads(), tau=base["tau"], tau_min=base["tau_min"],
                       delta=base["delta"], tile=1)
    assert sim.solve_ex(base["final_time"], W, P.PFT_SOLVE_KEEP_DEVICE) == 2
    assert sim.solve_ex(base["final_time"], K, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE) == 2
    sim.download()
    want = sim.interior().reshape(-1)
    traj = np.array([sim.t, sim.h, sim.system.steps, sim.system.steps_total])
    sim.close()
    assert traj[3] == W + K
    assert np.array_equal(ta, traj)
    assert xa.shape == want.shape and np.array_equal(xa, want)
