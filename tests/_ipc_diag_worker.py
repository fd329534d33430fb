"""One rank of a two-process run of the f5 diagnostics over the ipc transport
(tests/test_diag_gpu.py).  Started as its own process -- never forked from a process that uses the
GPU -- with:

    python tests/_ipc_diag_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "times": [...], "out": output prefix}; the case is the golden g20 (mode 0).
Writes <out>.<rank>.json: run_series' rows (snapshot 0 from the host arrays, the others from the
device-resident state), and the final diagnostics with this rank's ice_per_plane and first_row."""
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
                       nprocs=n, rank=rank, initial=A["traj_m0_ic"], tau=1.0, tau_min=info["tau_min"],
                       delta=info["delta"])
    rows = sim.run_series(times=spec["times"])
    d = sim.diagnostics(per_plane=True)
    sim.close()
    P.comm_destroy(comm)
    out = {"rows": rows, "diag": {k: v for k, v in d.items() if k not in ("ice_per_plane", "local")},
           "local": d["local"], "ice_per_plane": [int(v) for v in d["ice_per_plane"]], "first_row": d["first_row"]}
    with open(f"{spec['out']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
