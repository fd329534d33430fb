"""f11: what a region snapshot costs the solver, beside the three routes to the same cells without it,
at 200x200x400 (default Params, device IC) after 20 attempted steps.  Prints one JSON line with, for
each of four selections -- the central x-z section, the central y-z section, a stride-2 volume and a
200x200x16 box --
  image_MB      the region image's size (three fields);
  kernel_us     HIP-event time of region_kernel alone (pft_slab_snapshot_timing), median of REPS;
  stall_ms      wall time of Simulation.snapshot_device(region=, wait=False) until it returns -- the
                header, the gather, the image in pinned host memory, the job handed to the background
                writer -- median of REPS with its min and max, every call a new file, the write
                awaited and the file removed outside the timed part;
  region_ms     wall time of Simulation.region(sel): the same cells as a numpy array, no file;
and, measured in the same process:
  full_stall_ms / full_kernel_us   the f7 full snapshot_device(wait=False) and its export kernel;
  download_numpy_ms                download() followed by interior()[:, sel], per selection;
  save_snapshot_ms                 download() + save_snapshot (the host route's full dataset);
  stalls_below_full                per selection, whether its stall is below the full snapshot's.
GRID_NODES (default 400: 200x200x400), REPS and OUT (the directory of the files, default a temporary
one; the files are removed) from the environment."""
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

import porousfreezethaw_amd as P  # noqa: E402
from porousfreezethaw_amd import params as PR  # noqa: E402

FLAGS = P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE
ALL = slice(None)
med = statistics.median


def timed(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def main():
    nodes, reps = int(os.environ.get("GRID_NODES", "400")), int(os.environ.get("REPS", "5"))
    base = PR.default_params(grid_nodes=nodes)
    n1, n2, n3 = base["n1"], base["n2"], base["n3"]
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("region_time: no HIP device")
    own = "OUT" not in os.environ
    out = tempfile.mkdtemp(prefix="pft_region_time_") if own else os.environ["OUT"]
    os.makedirs(out, exist_ok=True)
    sels = {"xz_section": (ALL, n2 // 2, ALL), "yz_section": (ALL, ALL, n1 // 2),
            "stride2_volume": (slice(0, None, 2), slice(0, None, 2), slice(0, None, 2)),
            "box_16_planes": (slice(n3 // 2 - 8, n3 // 2 + 8), ALL, ALL)}
    res = {"grid": [n1, n2, n3], "reps": reps, "regions": {}}
    try:
        sim = P.Simulation(n1, n2, n3, (base["L1"], base["L2"], base["L3"]), 0, P.params_array(base), beads=beads,
                           tau=base["tau"], tau_min=base["tau_min"], delta=base["delta"], device_ic=True)
        sim.solve_ex(base["final_time"], 20, FLAGS)
        slab = C.c_void_p(L.pft_solver_slab())
        inf = P.snapshot_info(sim.t, sim.h, base["final_time"], base["delta"], 0, comment="region_time")
        assert L.pft_slab_snapshot_timing(slab, 1) == 0
        path = os.path.join(out, "stall.ncd")

        def one(region):
            """(stall ms, kernel us) of one background snapshot"""
            ms = timed(lambda: sim.snapshot_device(path, inf, wait=False, region=region))
            k = C.c_double()
            assert L.pft_slab_snapshot_last_ms(slab, C.byref(k)) == 0
            sim.snapshot_wait()
            os.remove(path)
            return ms, 1e3 * k.value

        runs = {name: [] for name in list(sels) + ["full"]}
        for i in range(1 + reps):                      # the routes alternate; the first round warms up
            for name in runs:
                v = one(sels.get(name))
                if i:
                    runs[name].append(v)
        res["full_image_MB"] = round(L.pft_slab_image_bytes(slab) / 1e6, 1)
        res["full_stall_ms"] = round(med(v[0] for v in runs["full"]), 3)
        res["full_stall_ms_min_max"] = [round(min(v[0] for v in runs["full"]), 3), round(max(v[0] for v in runs["full"]), 3)]
        res["full_kernel_us"] = round(med(v[1] for v in runs["full"]), 1)
        for name, sel in sels.items():
            r = P.region(*sel, sim.grid)
            got = sim.region(sel)
            live = [timed(lambda: sim.region(sel)) for _ in range(reps)]
            res["regions"][name] = {
                "count_kji": [r.count[2], r.count[1], r.count[0]], "image_MB": round(got.nbytes / 1e6, 3),
                "kernel_us": round(med(v[1] for v in runs[name]), 1),
                "stall_ms": round(med(v[0] for v in runs[name]), 3),
                "stall_ms_min_max": [round(min(v[0] for v in runs[name]), 3), round(max(v[0] for v in runs[name]), 3)],
                "region_ms": round(med(live), 3)}
        # the routes of the parent commit to the same cells
        dl = {name: [] for name in sels}
        for i in range(1 + reps):
            for name, sel in sels.items():
                t0 = time.perf_counter()
                sim.download()
                a = np.ascontiguousarray(sim.interior()[(ALL,) + tuple(s if isinstance(s, slice) else slice(s, s + 1) for s in sel)])
                ms = 1e3 * (time.perf_counter() - t0)
                if i:
                    dl[name].append(ms)
                assert np.array_equal(a.view(np.uint64), sim.region(sel).view(np.uint64)), name
        save = []
        for i in range(1 + min(reps, 3)):
            ms = timed(lambda: (sim.download(), P.save_snapshot(sim, path, inf)))
            os.remove(path)
            if i:
                save.append(ms)
        sim.close()
        for name in sels:
            res["regions"][name]["download_numpy_ms"] = round(med(dl[name]), 2)
        res["save_snapshot_ms"] = round(med(save), 2)
        res["stalls_below_full"] = {name: res["regions"][name]["stall_ms"] < res["full_stall_ms"] for name in sels}
    finally:
        if own:
            shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
