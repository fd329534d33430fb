"""f12: what formula diagnostics cost on the device against the routes through the host, at
200x200x400 (default Params, device IC) after 20 attempted steps.  Prints one JSON line with
  1. kernel_us        HIP-event time of the formula kernel pair (pft_slab_formulas_timing) for the
                      formulas `p>0.5`, `u`, the sensible heat and `tanh((u-u_star)/10)` alone and
                      for 8 formulas in one call, and beside them, in the same process and with the
                      calls alternating, diag_kernel_us (pft_slab_diag's kernel) and means_kernel_us
                      (the means kernel pair): the median of REPS each after WARMUP warm-up calls;
  2. device_ms        wall time of Simulation.formulas() (compile, the programs' upload, the
                      accumulators' reset, the two kernels, the records' copy, the host wait and
                      the rounding), median of REPS;
  3. download_host_ms wall time of the route without it: Simulation.download() and the host twin
                      (Simulation.formulas(where="host")), median of 3, whose records must equal the
                      device's word for word; and for `p>0.5` download_numpy_ms, download() and numpy.
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

ONE = {
    "ice": "p>0.5",
    "u": "u",
    "heat": "(water_cp*water_rho*(1-p)+ice_cp*ice_rho*p)*(1-gl)*(u-u_star)",
    "tanh": "tanh((u-u_star)/10)",
}
EIGHT = dict(ONE, pore="gl<0.5", ice_u="(p>0.5)*u", supercooled="p<0.5 and gl<0.5 and u<u_star",
             disc="(x-L1/2)^2+(y-L2/2)^2 < (L1/3)^2 and p>0.5")


def main():
    nodes = int(os.environ.get("GRID_NODES", "400"))
    reps, warm = int(os.environ.get("REPS", "20")), int(os.environ.get("WARMUP", "3"))
    base = PR.default_params(grid_nodes=nodes)
    V = {k: float(v) for k, v in base.items()}
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("formula_time: no HIP device")
    sim = P.Simulation(base["n1"], base["n2"], base["n3"], (base["L1"], base["L2"], base["L3"]), 0,
                       P.params_array(base), beads=beads, tau=base["tau"], tau_min=base["tau_min"],
                       delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    slab = C.c_void_p(L.pft_solver_slab())
    assert L.pft_slab_diag_timing(slab, 1) == 0 and L.pft_slab_means_timing(slab, 1) == 0
    assert L.pft_slab_formulas_timing(slab, 1) == 0
    cells = base["n1"] * base["n2"] * base["n3"]
    sets = {name: {name: expr} for name, expr in ONE.items()}
    sets["eight"] = EIGHT

    kern = {k: [] for k in sets}
    wall = {k: [] for k in sets}
    diag_us, means_us, dev = [], [], {}
    ms = C.c_double()
    for i in range(warm + reps):
        for k, formulas in sets.items():
            t0 = time.perf_counter()
            dev[k] = sim.formulas(formulas, V)
            t1 = time.perf_counter()
            assert L.pft_slab_formulas_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                kern[k].append(1e3 * ms.value)
                wall[k].append(1e3 * (t1 - t0))
            sim.diagnostics()
            assert L.pft_slab_diag_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                diag_us.append(1e3 * ms.value)
            sim.means()
            assert L.pft_slab_means_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                means_us.append(1e3 * ms.value)
    for fn in (L.pft_slab_diag_timing, L.pft_slab_means_timing, L.pft_slab_formulas_timing):
        fn(slab, 0)

    down = {k: [] for k in sets}
    same = {}
    for k, formulas in sets.items():
        for _ in range(3):
            t0 = time.perf_counter()
            sim.download()
            host = sim.formulas(formulas, V, where="host")
            down[k].append(1e3 * (time.perf_counter() - t0))
        same[k] = all(host[n] == dev[k][n] or (str(host[n]) == str(dev[k][n])) for n in formulas)
    numpy_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        sim.download()
        frac = float((sim.interior()[1] > 0.5).mean())
        numpy_ms.append(1e3 * (time.perf_counter() - t0))
    sim.close()
    assert all(same.values()), same
    assert frac == dev["ice"]["ice"]["mean"], (frac, dev["ice"]["ice"]["mean"])

    med = statistics.median
    m_us, g_us = med(means_us), med(diag_us)
    out = {"grid": [base["n1"], base["n2"], base["n3"]], "cells": cells, "reps": reps, "warmup": warm,
           "diag_kernel_us": round(g_us, 2), "means_kernel_us": round(m_us, 2),
           "download_numpy_ms_ice": round(med(numpy_ms), 2), "formulas": {}}
    for k in sets:
        out["formulas"][k] = {
            "kernel_us": round(med(kern[k]), 2), "kernel_us_min_max": [round(min(kern[k]), 2), round(max(kern[k]), 2)],
            "over_means_kernel": round(med(kern[k]) / m_us, 2), "device_ms": round(med(wall[k]), 4),
            "download_host_ms": round(med(down[k]), 2),
            "device_below_download": med(wall[k]) < med(down[k]) and (k != "ice" or med(wall[k]) < med(numpy_ms))}
    out["device_below_every_download_route"] = all(v["device_below_download"] for v in out["formulas"].values())
    out["values"] = {n: {q: dev["eight"][n][q] for q in ("mean", "min", "max", "nonzero")} for n in EIGHT}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
