"""f6: what the exact means cost on the device against the route through the host, at 200x200x400
(default Params, device IC) after 20 attempted steps.  Prints one JSON line with
  1. means_kernel_us  HIP-event time of the means kernel pair (pft_slab_means_timing), and beside
                      it diag_kernel_us, pft_slab_diag's kernel, in the same process: calls of the
                      two alternate, the median of REPS each after WARMUP warm-up calls; both read
                      the same 3 fields x 8 bytes per cell, read_GBs is that over the time;
  2. means_ms         wall time of Simulation.means() (the accumulators' reset, the two kernels,
                      the record's copy, the host wait and the rounding), median of REPS;
  3. download_numpy_ms  wall time of the route without it: Simulation.download() and the same four
                      means in numpy (whose sums depend on numpy's order: compared to 1e-12
                      relative here, the exact comparison is the tests'), median of 3.
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


def main():
    nodes = int(os.environ.get("GRID_NODES", "400"))
    reps, warm = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))
    base = PR.default_params(grid_nodes=nodes)
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("means_time: no HIP device")
    sim = P.Simulation(base["n1"], base["n2"], base["n3"], (base["L1"], base["L2"], base["L3"]), 0,
                       P.params_array(base), beads=beads, tau=base["tau"], tau_min=base["tau_min"],
                       delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    slab = C.c_void_p(L.pft_solver_slab())
    assert L.pft_slab_diag_timing(slab, 1) == 0 and L.pft_slab_means_timing(slab, 1) == 0
    cells = base["n1"] * base["n2"] * base["n3"]

    means_us, diag_us, wall_ms, profile_ms = [], [], [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        d = sim.means()
        t1 = time.perf_counter()
        ms = C.c_double()
        assert L.pft_slab_means_last_ms(slab, C.byref(ms)) == 0
        sim.diagnostics()
        ds = C.c_double()
        assert L.pft_slab_diag_last_ms(slab, C.byref(ds)) == 0
        t2 = time.perf_counter()
        sim.means(per_plane=True)
        t3 = time.perf_counter()
        if i >= warm:
            means_us.append(1e3 * ms.value)
            diag_us.append(1e3 * ds.value)
            wall_ms.append(1e3 * (t1 - t0))
            profile_ms.append(1e3 * (t3 - t2))
    L.pft_slab_diag_timing(slab, 0)
    L.pft_slab_means_timing(slab, 0)

    down_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        sim.download()
        u, p, gl = sim.interior()
        ice, pore = p > 0.5, gl < 0.5
        host = {"u_mean": float(u.mean()), "p_mean": float(p.mean()),
                "ice_u_mean": float(u[ice].mean()) if ice.any() else float("nan"),
                "pore_p_mean": float(p[pore].mean()) if pore.any() else float("nan")}
        down_ms.append(1e3 * (time.perf_counter() - t0))
    hd = sim.means(where="host")
    sim.close()
    assert all(abs(host[k] - d[k]) <= 1e-12 * abs(d[k]) for k in host), (host, d)
    assert all(hd[k] == d[k] for k in d), (hd, d)

    m_us, g_us = statistics.median(means_us), statistics.median(diag_us)

    def gbs(us):
        return round(3 * 8 * cells / (us * 1e-6) / 1e9, 1)

    print(json.dumps({
        "grid": [base["n1"], base["n2"], base["n3"]], "cells": cells, "reps": reps, "warmup": warm,
        "means_kernel_us": round(m_us, 2), "means_kernel_us_min_max": [round(min(means_us), 2), round(max(means_us), 2)],
        "means_read_GBs": gbs(m_us),
        "diag_kernel_us": round(g_us, 2), "diag_kernel_us_min_max": [round(min(diag_us), 2), round(max(diag_us), 2)],
        "diag_read_GBs": gbs(g_us), "means_over_diag": round(m_us / g_us, 3),
        "means_ms": round(statistics.median(wall_ms), 4),
        "means_per_plane_ms": round(statistics.median(profile_ms), 3),
        "download_numpy_ms": round(statistics.median(down_ms), 2),
        "download_over_means": round(statistics.median(down_ms) / statistics.median(wall_ms), 1),
        "means_below_download": statistics.median(wall_ms) < statistics.median(down_ms),
        "u_mean": d["u_mean"], "p_mean": d["p_mean"], "ice_u_mean": d["ice_u_mean"], "pore_p_mean": d["pore_p_mean"],
        "ice_u_n": d["ice_u_n"], "pore_p_n": d["pore_p_n"]}))


if __name__ == "__main__":
    main()
