"""f5: what the device-side diagnostics cost against the route through the host, at 200x200x400
(default Params, device IC) after 20 attempted steps.  Prints one JSON line with
  1. kernel_us       HIP-event time of the diagnostics kernel alone (pft_slab_diag_timing): the median
                     of REPS calls after WARMUP warm-up calls, and the read bandwidth that is
                     (3 fields x 8 bytes per cell over that time);
  2. diagnostics_ms  wall time of Simulation.diagnostics() (the accumulators' reset, the kernel, the
                     record's copy and the host wait), median of REPS;
  3. download_ms     wall time of the route without it: Simulation.download() and the same
                     quantities in numpy, median of 3;
  4. stage1_us       the speculative stage-1 launch's HIP-event time (PFT_OPT_TIMING, every step of
                     the same process's 20 steps): it reads the same three fields, writes K1 and does
                     the whole right-hand side, so (1) has no reason to exceed it.
GRID_NODES (default 400: 200x200x400), REPS, WARMUP from the environment."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

import porousfreezethaw_amd as P  # noqa: E402
from porousfreezethaw_amd import params as PR  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0     # streaming reads, MI355X (8 TB/s peak)


def main():
    nodes = int(os.environ.get("GRID_NODES", "400"))
    reps, warm = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))
    base = PR.default_params(grid_nodes=nodes)
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("diag_time: no HIP device")
    L.pft_solver_set_option(P.PFT_OPT_TIMING, 1)
    sim = P.Simulation(base["n1"], base["n2"], base["n3"], (base["L1"], base["L2"], base["L3"]), 0,
                       P.params_array(base), beads=beads, tau=base["tau"], tau_min=base["tau_min"],
                       delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    st = sim.stats()
    L.pft_solver_set_option(P.PFT_OPT_TIMING, 0)
    stage_us = [1e3 * st.stage_ms[i] / st.stage_n[i] if st.stage_n[i] else None for i in range(6)]
    slab = C.c_void_p(L.pft_solver_slab())
    assert L.pft_slab_diag_timing(slab, 1) == 0
    cells = base["n1"] * base["n2"] * base["n3"]

    kernel_us, wall_ms = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        d = sim.diagnostics()
        t1 = time.perf_counter()
        ms = C.c_double()
        assert L.pft_slab_diag_last_ms(slab, C.byref(ms)) == 0
        if i >= warm:
            kernel_us.append(1e3 * ms.value)
            wall_ms.append(1e3 * (t1 - t0))
    L.pft_slab_diag_timing(slab, 0)

    down_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        sim.download()
        u, p, gl = sim.interior()
        ice = p > 0.5
        host = {"ice": int(ice.sum()), "pore": int((gl < 0.5).sum()),
                "ice_u_maxabs": float(np.abs(u[ice]).max()) if ice.any() else 0.0}
        down_ms.append(1e3 * (time.perf_counter() - t0))
    sim.close()
    assert all(host[k] == d[k] for k in host), (host, d)

    k_us = statistics.median(kernel_us)
    gbs = 3 * 8 * cells / (k_us * 1e-6) / 1e9
    print(json.dumps({
        "grid": [base["n1"], base["n2"], base["n3"]], "cells": cells, "reps": reps, "warmup": warm,
        "kernel_us": round(k_us, 2), "kernel_us_min_max": [round(min(kernel_us), 2), round(max(kernel_us), 2)],
        "read_GBs": round(gbs, 1), "hbm_achievable_GBs": HBM_ACHIEVABLE_GBS,
        "share_of_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 3),
        "diagnostics_ms": round(statistics.median(wall_ms), 4), "download_numpy_ms": round(statistics.median(down_ms), 2),
        "stage1_us": None if stage_us[1] is None else round(stage_us[1], 2),
        "stage_us": [None if v is None else round(v, 2) for v in stage_us[1:]],
        "ice": d["ice"], "ice_fraction": d["ice_fraction"],
        "diagnostics_below_download": statistics.median(wall_ms) < statistics.median(down_ms),
        "kernel_below_stage1": None if stage_us[1] is None else k_us < stage_us[1]}))


if __name__ == "__main__":
    main()
