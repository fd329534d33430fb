"""One rank of a two-process run of the f12 formula diagnostics over the ipc transport
(tests/test_formula_gpu.py).  Started as its own process -- never forked from a process that uses
the GPU -- with:

    python tests/_ipc_formula_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "times": [...], "formulas": {...}, "variables": {...}, "out": output prefix};
the case is the golden g20 (mode 0).  Writes <out>.<rank>.json: run_series(formulas=)'s rows
(snapshot 0 from the host arrays, the others from the device-resident state), per formula the final
global record's raw words, this rank's planes' records' and its own cell count, first_row, and the
exception a formula that is not device-exact raises (on both ranks alike, before any device work)."""
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
    rows = sim.run_series(times=spec["times"], formulas=spec["formulas"], variables=spec["variables"])
    d = sim.formulas(spec["formulas"], spec["variables"], per_plane=True)
    try:
        sim.formulas({"sq": "u^2"}, spec["variables"])
        not_exact = "none"
    except ValueError as e:
        not_exact = type(e).__name__
    sim.close()
    P.comm_destroy(comm)
    out = {"rows": rows, "first_row": sim.grid.first_row, "not_exact": not_exact,
           "words": {k: v["record"].words() for k, v in d.items()},
           "plane_words": {k: [m.words() for m in v["plane_records"]] for k, v in d.items()},
           "local_cells": {k: v["local"]["cells"] for k, v in d.items()}}
    with open(f"{spec['out']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
