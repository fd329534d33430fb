"""One rank of a two-process run of the f6 means over the ipc transport (tests/test_means_gpu.py).
Started as its own process -- never forked from a process that uses the GPU -- with:

    python tests/_ipc_means_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "times": [...], "out": output prefix}; the case is the golden g20 (mode 0).
Writes <out>.<rank>.json: run_series(means=True)'s rows (snapshot 0 from the host arrays, the
others from the device-resident state), the final global record's raw words, this rank's own
record's, its planes' records' and first_row."""
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
    rows = sim.run_series(times=spec["times"], means=True)
    d = sim.means(per_plane=True)
    sim.close()
    P.comm_destroy(comm)
    out = {"rows": rows, "words": d["record"].words(), "plane_words": [m.words() for m in d["plane_records"]],
           "local": d["local"], "first_row": d["first_row"],
           "profiles": {k + "_profile": [float(x) for x in d[k + "_profile"]] for k in P.MEAN_KEYS}}
    with open(f"{spec['out']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
