"""One rank of a two-process run of the f13 histograms over the ipc transport
(tests/test_hist_gpu.py).  Started as its own process -- never forked from a process that uses the
GPU -- with:

    python tests/_ipc_hist_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "times": [...], "hist": {"formula", "bins", "range", "mask"}, "variables": {...},
"out": output prefix}; the case is the golden g20 (mode 0).  Writes <out>.<rank>.json:
run_series(histograms=)'s rows, the final histogram with this rank's planes, and the codes of two
calls that every rank must refuse alike before any device work: edges that differ between the ranks
(-2 from pft_solver_hist) and a formula that is not device-exact (ValueError)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

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
    h = spec["hist"]
    rows = sim.run_series(times=spec["times"], histograms={"sc": h}, variables=spec["variables"])
    d = sim.histogram(h["formula"], h["bins"], h["range"], mask=h["mask"], variables=spec["variables"], per_plane=True)
    # edges that depend on the rank: every rank answers -2, nothing is launched
    _, _, vops, vargs = P.formula_programs({"f": "u"}, spec["variables"])
    edges = np.array([0.0, 1.0 + rank, 400.0])
    head, counts = P.pft_hist_head(), (C.c_longlong * 2)()
    differ = sim.lib.pft_solver_hist(len(vops), P._ip(vops), P._dp(vargs), 0, None, None, 2, P._dp(edges), C.byref(head),
                                     counts, None, None, None, None)
    try:
        sim.histogram("u^2", 4, (0.0, 1.0), variables=spec["variables"])
        not_exact = "none"
    except ValueError as e:
        not_exact = type(e).__name__
    after = sim.histogram(h["formula"], h["bins"], h["range"], mask=h["mask"], variables=spec["variables"])
    sim.close()
    P.comm_destroy(comm)

    def plain(x):
        return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in x.items() if k != "local"}

    out = {"rows": [plain(r) for r in rows], "hist": plain(d), "local": plain(d["local"]), "differ": differ,
           "not_exact": not_exact, "after": plain(after)}
    with open(f"{spec['out']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
