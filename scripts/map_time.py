"""f15: what a map costs on the device against the route through the host, at 200x200x400 (default
Params, device IC) after 20 attempted steps.  Prints one JSON line; per axis and case
  1. kernel_us           HIP-event time of map_kernel (pft_slab_map_timing), and beside it, in the
                         same process and with the calls alternating, formulas_kernel_us: f12's
                         kernel pair with per_plane=True for the same value formula and, where there
                         is a mask, the mask formula as a second program -- the same interpreter work
                         without the map: the median of REPS each after WARMUP warm-up calls;
  2. device_ms           wall time of Simulation.project() (compile, the programs' upload, the
                         accumulators' reset, the kernel, the map's copy and the host wait, the
                         records' decoding), median of REPS;
  3. download_ms         wall time of Simulation.download() alone, median of 3;
  4. download_host_ms    wall time of Simulation.download() and the host twin
                         (Simulation.project(where="host")), median of 3, whose map must equal the
                         device's bit for bit.
The cases: `p>0.5` (the front's height map, the ice thickness) and `u` where `p>0.5` (the warmest
ice).  GRID_NODES (default 400: 200x200x400), REPS, WARMUP from the environment; DOWNLOADS=0 leaves
the routes through the host out."""
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
    V = {k: float(v) for k, v in base.items()}
    n1, n2, n3 = base["n1"], base["n2"], base["n3"]
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("map_time: no HIP device")
    sim = P.Simulation(n1, n2, n3, (base["L1"], base["L2"], base["L3"]), 0, P.params_array(base), beads=beads,
                       tau=base["tau"], tau_min=base["tau_min"], delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    slab = C.c_void_p(L.pft_solver_slab())
    assert L.pft_slab_formulas_timing(slab, 1) == 0 and L.pft_slab_map_timing(slab, 1) == 0

    cases = {"ice": ("p>0.5", None), "warm_ice": ("u", "p>0.5")}
    keys = [(axis, k) for axis in (0, 1, 2) for k in cases]
    kern, wall, f12 = ({q: [] for q in keys} for _ in range(3))
    dev = {}
    ms = C.c_double()
    for i in range(warm + reps):
        for axis, k in keys:
            f, mask = cases[k]
            t0 = time.perf_counter()
            dev[axis, k] = sim.project(f, axis, mask=mask, variables=V)
            t1 = time.perf_counter()
            assert L.pft_slab_map_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                kern[axis, k].append(1e3 * ms.value)
                wall[axis, k].append(1e3 * (t1 - t0))
            sim.formulas({"v": f} if mask is None else {"v": f, "m": mask}, V, per_plane=True)
            assert L.pft_slab_formulas_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                f12[axis, k].append(1e3 * ms.value)
    L.pft_slab_formulas_timing(slab, 0)
    L.pft_slab_map_timing(slab, 0)

    downloads = os.environ.get("DOWNLOADS", "1") != "0"
    down, down_host, same = [], {q: [] for q in keys}, {}
    for _ in range(3 if downloads else 0):
        t0 = time.perf_counter()
        sim.download()
        down.append(1e3 * (time.perf_counter() - t0))
    for axis, k in keys if downloads else ():
        f, mask = cases[k]
        for _ in range(3):
            t0 = time.perf_counter()
            sim.download()
            host = sim.project(f, axis, mask=mask, variables=V, where="host")
            down_host[axis, k].append(1e3 * (time.perf_counter() - t0))
        same[axis, k] = all(np.array_equal(host[q].view(np.int64), dev[axis, k][q].view(np.int64)) for q in P.MAP_KEYS)
    sim.close()
    assert all(same.values()), same

    med = statistics.median
    out = {"grid": [n1, n2, n3], "cells": n1 * n2 * n3, "reps": reps, "warmup": warm, "cases": {}}
    if downloads:
        out["download_ms"] = round(med(down), 2)
    for axis, k in keys:
        d = dev[axis, k]
        c = {"axis": axis, "formula": cases[k][0], "mask": cases[k][1], "map": list(d["selected"].shape),
             "kernel_us": round(med(kern[axis, k]), 2),
             "kernel_us_min_max": [round(min(kern[axis, k]), 2), round(max(kern[axis, k]), 2)],
             "formulas_kernel_us": round(med(f12[axis, k]), 2),
             "over_formulas_kernel": round(med(kern[axis, k]) / med(f12[axis, k]), 2),
             "device_ms": round(med(wall[axis, k]), 4), "nonzero": int(d["nonzero"].sum()),
             "lines_with_a_nonzero_cell": int((d["first"] >= 0).sum())}
        if downloads:
            c.update({"download_host_ms": round(med(down_host[axis, k]), 2), "device_below_download": med(wall[axis, k]) < med(down)})
        out["cases"][f"{k}_axis{axis}"] = c
    if downloads:
        out["device_below_download_alone"] = all(v["device_below_download"] for v in out["cases"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
