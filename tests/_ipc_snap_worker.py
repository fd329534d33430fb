"""One rank of a two-process run of the f7 device snapshots over the ipc transport
(tests/test_snapshot_device_gpu.py).  Started as its own process -- never forked from a process that
uses the GPU -- with:

    python tests/_ipc_snap_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "icond_file", "t0", "tau", "T", "out": dataset to write, "res": result
prefix}; the case is the golden g20 (mode 0).  The rank reads its planes of icond_file on the device,
solves to T and writes its planes of `out` from the resident state (background write, then
snapshot_wait).  Writes <res>.<rank>.json: t, h and the diagnostics right after the read."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _oracle as O  # noqa: E402
import porousfreezethaw_amd as P  # noqa: E402


def main():
    spec = json.load(open(sys.argv[1]))
    rank = int(sys.argv[2])
    n = spec["nranks"]
    comm = P.comm_init_ipc(n, rank, spec["shm"], spec.get("device", 0))
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       nprocs=n, rank=rank, icond_file=spec["icond_file"], t0=spec["t0"], tau=spec["tau"],
                       tau_min=info["tau_min"], delta=info["delta"])
    d = sim.diagnostics()
    sim.solve_ex(spec["T"], 0, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    inf = P.snapshot_info(sim.t, sim.h, spec["T"], info["delta"], 0, snapshot=2, total_snapshots=4, comment="ipc")
    sim.snapshot_device(spec["out"], inf, wait=False)
    sim.snapshot_wait()
    out = {"t": sim.t, "h": sim.h, "diag": d}
    sim.close()
    P.comm_destroy(comm)
    with open(f"{spec['res']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
