"""f13: what a histogram costs on the device against the routes through the host, at 200x200x400
(default Params, device IC) after 20 attempted steps.  Prints one JSON line; per case
  1. kernel_us          HIP-event time of the histogram kernel pair (pft_slab_hist_timing), and beside
                        it, in the same process and with the calls alternating, formulas_kernel_us
                        (f12's kernel pair for the same value formula and, where there is a mask,
                        the mask formula as a second program) and diag_kernel_us (pft_slab_diag's
                        kernel): the median of REPS each after WARMUP warm-up calls;
  2. device_ms          wall time of Simulation.histogram() (compile, the programs' and edges'
                        upload, the accumulators' reset, the two kernels, the rows' copy and the
                        host wait), median of REPS;
  3. download_numpy_ms  wall time of Simulation.download() and numpy.histogram of the same values,
                        median of 3, whose counts must equal the device's;
  4. download_host_ms   wall time of Simulation.download() and the host twin
                        (Simulation.histogram(where="host")), median of 3, the same counts again.
The cases: `u` in 64 bins (concentrated: almost one bin), `p` in 256 bins, `u` where `p>0.5`, and a
formula of the coordinates that spreads evenly over 1024 bins (every lane of a wave another bin).
GRID_NODES (default 400: 200x200x400), REPS, WARMUP from the environment; DOWNLOADS=0 leaves the two
routes through the host out (the kernel times of another build of the library, PFT_LIB)."""
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
        raise SystemExit("hist_time: no HIP device")
    sim = P.Simulation(n1, n2, n3, (base["L1"], base["L2"], base["L3"]), 0, P.params_array(base), beads=beads,
                       tau=base["tau"], tau_min=base["tau_min"], delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    slab = C.c_void_p(L.pft_solver_slab())
    assert L.pft_slab_diag_timing(slab, 1) == 0 and L.pft_slab_formulas_timing(slab, 1) == 0
    assert L.pft_slab_hist_timing(slab, 1) == 0

    spread = f"(_x+_y/{n1})*1024"        # (0.5 + i) / n1 + (0.5 + j) / (n1 n2): n1 n2 values, evenly over (0, 1)
    # name: (formula, bins, range, mask, numpy's values and selection of an interior state x[3][n3][n2][n1])
    xs = ((0.5 + np.arange(n1)) / n1)[None, None, :]
    ys = ((0.5 + np.arange(n2)) / n2)[None, :, None]
    cases = {
        "u64": ("u", 64, (250.0, 300.0), None, lambda x: (x[0], None)),
        "p256": ("p", 256, (0.0, 1.0), None, lambda x: (x[1], None)),
        "u64_ice": ("u", 64, (250.0, 300.0), "p>0.5", lambda x: (x[0], x[1] > 0.5)),
        "spread1024": (spread, 1024, (0.0, 1024.0), None,
                       lambda x: (np.broadcast_to((xs + ys / n1) * 1024, x[0].shape), None)),
    }
    kern, wall, f12 = ({k: [] for k in cases} for _ in range(3))
    diag_us, dev = [], {}
    ms = C.c_double()
    for i in range(warm + reps):
        for k, (f, bins, rng, mask, _) in cases.items():
            t0 = time.perf_counter()
            dev[k] = sim.histogram(f, bins, rng, mask=mask, variables=V)
            t1 = time.perf_counter()
            assert L.pft_slab_hist_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                kern[k].append(1e3 * ms.value)
                wall[k].append(1e3 * (t1 - t0))
            sim.formulas({"v": f} if mask is None else {"v": f, "m": mask}, V)
            assert L.pft_slab_formulas_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                f12[k].append(1e3 * ms.value)
            sim.diagnostics()
            assert L.pft_slab_diag_last_ms(slab, C.byref(ms)) == 0
            if i >= warm:
                diag_us.append(1e3 * ms.value)
    for fn in (L.pft_slab_diag_timing, L.pft_slab_formulas_timing, L.pft_slab_hist_timing):
        fn(slab, 0)

    downloads = os.environ.get("DOWNLOADS", "1") != "0"
    down_np, down_host, same = ({k: [] for k in cases} for _ in range(3))
    for k, (f, bins, rng, mask, values) in cases.items() if downloads else ():
        for _ in range(3):
            t0 = time.perf_counter()
            sim.download()
            v, sel = values(sim.interior())
            counts = np.histogram(v if sel is None else v[sel], bins=dev[k]["edges"])[0]
            down_np[k].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            sim.download()
            host = sim.histogram(f, bins, rng, mask=mask, variables=V, where="host")
            down_host[k].append(1e3 * (time.perf_counter() - t0))
        same[k] = bool((counts == dev[k]["counts"]).all() and (host["counts"] == dev[k]["counts"]).all()
                       and all(host[q] == dev[k][q] for q in ("cells", "selected", "nan", "under", "over")))
    sim.close()
    assert all(same.values()) or not downloads, same

    med = statistics.median
    out = {"grid": [n1, n2, n3], "cells": n1 * n2 * n3, "reps": reps, "warmup": warm,
           "diag_kernel_us": round(med(diag_us), 2), "cases": {}}
    for k in cases:
        c = dev[k]["counts"]
        out["cases"][k] = {
            "formula": cases[k][0], "bins": cases[k][1], "mask": cases[k][3],
            "kernel_us": round(med(kern[k]), 2), "kernel_us_min_max": [round(min(kern[k]), 2), round(max(kern[k]), 2)],
            "formulas_kernel_us": round(med(f12[k]), 2), "over_formulas_kernel": round(med(kern[k]) / med(f12[k]), 2),
            "device_ms": round(med(wall[k]), 4),
            "selected": dev[k]["selected"], "largest_bin_share": round(float(c.max()) / max(1, dev[k]["selected"]), 4),
            "bins_hit": int((c > 0).sum())}
        if downloads:
            out["cases"][k].update({
                "download_numpy_ms": round(med(down_np[k]), 2), "download_host_ms": round(med(down_host[k]), 2),
                "device_below_downloads": med(wall[k]) < med(down_np[k]) and med(wall[k]) < med(down_host[k])})
    if downloads:
        out["device_below_every_download_route"] = all(v["device_below_downloads"] for v in out["cases"].values())
    out["concentrated_not_slower_than_spread"] = out["cases"]["u64"]["kernel_us"] <= out["cases"]["spread1024"]["kernel_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
