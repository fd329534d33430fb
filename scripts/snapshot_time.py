"""f7: what a snapshot costs the solver, from the resident state against the route through the host,
at 200x200x400 (default Params, device IC) after 20 attempted steps.  Prints one JSON line with
  (a) stall_ms        wall time of Simulation.snapshot_device(wait=False) until it returns -- the
                      header, the export, the image in pinned host memory, the job handed to the
                      background writer -- for both host links ("direct": the kernel stores into the
                      host-mapped buffer; "staged": into a device image, then one hipMemcpyAsync),
                      median of REPS, every call a new file as in a series, the write itself awaited
                      and the file removed outside the timed part; beside it
                      parent_ms, the route without it: download() + save_snapshot, in the same
                      process, with its spread (max - min) over its own repetitions;
  (b) export_kernel_us  HIP-event time of the export kernel alone (pft_slab_snapshot_timing), into
                      device memory and into the host-mapped buffer, with the bytes it moves (read +
                      written) per second; diag_kernel_us, pft_slab_diag's kernel, in the same
                      process; pinned_memcpy_ms, a bare device-to-pinned-host copy of the image's
                      size: the floor of the host link;
  (c) series_s        wall time of a 10-snapshot series (STEPS attempted steps between snapshots)
                      three ways, each from a fresh simulation: files written in the background
                      (async), files written before the next interval starts (sync), no files.
GRID_NODES (default 400: 200x200x400), REPS, STEPS and OUT (the directory of the files, default a
temporary one; the files are removed) from the environment."""
import ctypes as C
import hashlib
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


def make(base, beads):
    sim = P.Simulation(base["n1"], base["n2"], base["n3"], (base["L1"], base["L2"], base["L3"]), 0,
                       P.params_array(base), beads=beads, tau=base["tau"], tau_min=base["tau_min"],
                       delta=base["delta"], device_ic=True)
    sim.solve_ex(base["final_time"], 20, FLAGS)
    return sim


def info_of(sim, base, s=0, total=10):
    return P.snapshot_info(sim.t, sim.h, base["final_time"], base["delta"], 0, snapshot=s, total_snapshots=total,
                           comment="snapshot_time")


def file_hash(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def series(base, beads, out, mode, steps):
    """10 snapshots, `steps` attempted steps between them; mode "async", "sync" or "none"""
    sim = make(base, beads)
    try:
        t0 = time.perf_counter()
        for s in range(10):
            if s:
                sim.solve_ex(base["final_time"], steps, FLAGS)
            if mode != "none":
                sim.snapshot_device(os.path.join(out, "series.%03d.ncd" % s), info_of(sim, base, s), wait=mode == "sync")
        if mode == "async":
            sim.snapshot_wait()
        return time.perf_counter() - t0
    finally:
        sim.close()
        for s in range(10):
            f = os.path.join(out, "series.%03d.ncd" % s)
            if os.path.exists(f):
                os.remove(f)


def main():
    nodes = int(os.environ.get("GRID_NODES", "400"))
    reps, steps = int(os.environ.get("REPS", "5")), int(os.environ.get("STEPS", "200"))
    base = PR.default_params(grid_nodes=nodes)
    beads = np.load(os.path.join(REPO, "tests", "golden", "beads.npy"))
    L = P.lib()
    if P.device_count() < 1:
        raise SystemExit("snapshot_time: no HIP device")
    own = "OUT" not in os.environ
    out = tempfile.mkdtemp(prefix="pft_snapshot_time_") if own else os.environ["OUT"]
    os.makedirs(out, exist_ok=True)
    res = {"grid": [base["n1"], base["n2"], base["n3"]], "cells": base["n1"] * base["n2"] * base["n3"], "reps": reps}
    try:
        sim = make(base, beads)
        slab = C.c_void_p(L.pft_solver_slab())
        image = L.pft_slab_image_bytes(slab)
        res["image_MB"] = round(image / 1e6, 1)
        path = os.path.join(out, "stall.ncd")
        keep = os.path.join(out, "device.ncd")
        inf = info_of(sim, base)
        assert L.pft_slab_snapshot_timing(slab, 1) == 0 and L.pft_slab_diag_timing(slab, 1) == 0

        # (a), (b): the stall and the kernel, the two host links alternating
        stall = {"direct": [], "staged": []}
        kern = {"direct": [], "staged": []}
        diag_us = []
        for i in range(1 + reps):
            for link in ("direct", "staged"):
                t0 = time.perf_counter()
                sim.snapshot_device(path, inf, wait=False, link=link)
                t1 = time.perf_counter()
                sim.snapshot_wait()
                os.replace(path, keep)
                ms = C.c_double()
                assert L.pft_slab_snapshot_last_ms(slab, C.byref(ms)) == 0
                if i:
                    stall[link].append(1e3 * (t1 - t0))
                    kern[link].append(1e3 * ms.value)
            sim.diagnostics()
            ds = C.c_double()
            assert L.pft_slab_diag_last_ms(slab, C.byref(ds)) == 0
            if i:
                diag_us.append(1e3 * ds.value)
        dev_file = file_hash(keep)
        os.remove(keep)
        parent = []
        for i in range(1 + reps):
            t0 = time.perf_counter()
            sim.download()
            P.save_snapshot(sim, path, inf)
            if i:
                parent.append(1e3 * (time.perf_counter() - t0))
            os.replace(path, keep)
        assert file_hash(keep) == dev_file, "the device's file differs from the host's"
        os.remove(keep)

        # the floor of the host link: a bare copy of the image's size, device to pinned host
        L.pft_dev_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.pft_dev_free.argtypes = [C.c_void_p]
        L.pft_flat_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.pft_stream_sync.argtypes = [C.c_void_p]
        dev, host = C.c_void_p(), C.c_void_p()
        assert L.pft_dev_alloc(C.byref(dev), image) == 0 and L.pft_slab_image(slab, C.byref(host), None) == 0
        stream = L.pft_slab_stream(slab)
        copy = []
        for i in range(1 + reps):
            t0 = time.perf_counter()
            assert L.pft_flat_d2h(host, dev, image // 8, stream) == 0 and L.pft_stream_sync(stream) == 0
            if i:
                copy.append(1e3 * (time.perf_counter() - t0))
        L.pft_dev_free(dev)
        sim.close()

        med = statistics.median
        kept = "direct" if med(stall["direct"]) <= med(stall["staged"]) else "staged"
        res.update({
            "stall_ms": {k: round(med(v), 2) for k, v in stall.items()},
            "stall_ms_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in stall.items()},
            "faster_link": kept,
            "parent_ms": round(med(parent), 2), "parent_ms_min_max": [round(min(parent), 2), round(max(parent), 2)],
            "parent_spread_ms": round(max(parent) - min(parent), 2),
            "parent_over_stall": round(med(parent) / med(stall[kept]), 2),
            "stall_below_parent_by_more_than_its_spread": med(parent) - med(stall[kept]) > max(parent) - min(parent),
            "export_kernel_us": {k: round(med(v), 1) for k, v in kern.items()},
            "export_kernel_TBs": {k: round(2 * image / (med(v) * 1e-6) / 1e12, 3) for k, v in kern.items()},
            "diag_kernel_us": round(med(diag_us), 1),
            "pinned_memcpy_ms": round(med(copy), 2), "pinned_memcpy_GBs": round(image / (med(copy) * 1e-3) / 1e9, 1)})

        # (c) overlap
        res["series_steps_per_interval"] = steps
        res["series_s"] = {m: round(series(base, beads, out, m, steps), 3) for m in ("async", "sync", "none")}
        res["async_below_sync"] = res["series_s"]["async"] < res["series_s"]["sync"]
    finally:
        if own:
            shutil.rmtree(out, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
