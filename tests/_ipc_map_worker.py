"""One rank of a two-process run of the f15 maps over the ipc transport (tests/test_map_gpu.py).
Started as its own process -- never forked from a process that uses the GPU -- with:

    python tests/_ipc_map_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "times": [...], "maps": {name: {"formula", "axis", "mask"}}, "variables": {...},
"out": output prefix}; the case is the golden g20 (mode 0).  Writes <out>.<rank>.json:
run_series(maps=)'s rows, every map once more combined and as this rank's share, the wall time of
the combined calls, and the codes of two calls that every rank must refuse alike before any device
work: an axis that differs between the ranks (-2 from pft_solver_map) and a formula that is not
device-exact (ValueError)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import _oracle as O  # noqa: E402
import porousfreezethaw_amd as P  # noqa: E402


def plain(x):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in x.items()}


def main():
    spec = json.load(open(sys.argv[1]))
    rank = int(sys.argv[2])
    n = spec["nranks"]
    comm = P.comm_init_ipc(n, rank, spec["shm"], spec.get("device", 0))
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    V = spec["variables"]
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       nprocs=n, rank=rank, initial=A["traj_m0_ic"], tau=1.0, tau_min=info["tau_min"],
                       delta=info["delta"])
    rows = sim.run_series(times=spec["times"], maps=spec["maps"], variables=V)
    both, share, wall = {}, {}, {}
    for name, m in spec["maps"].items():
        t0 = time.perf_counter()
        both[name] = sim.project(m["formula"], m["axis"], mask=m.get("mask"), variables=V)
        wall[name] = time.perf_counter() - t0
        share[name] = sim.project(m["formula"], m["axis"], mask=m.get("mask"), variables=V, combine=False)
    # an axis that depends on the rank: every rank answers -2, nothing is launched
    _, _, vops, vargs = P.formula_programs({"f": "u"}, V)
    local = np.empty(info["n3"] * info["n1"], dtype=P.MAP_DTYPE)
    differ = sim.lib.pft_solver_map(len(vops), P._ip(vops), P._dp(vargs), 0, None, None, 1 + rank, None, P._map_ptr(local))
    try:
        sim.project("u^2", 0, variables=V)
        not_exact = "none"
    except ValueError as e:
        not_exact = type(e).__name__
    name, m = next(iter(spec["maps"].items()))
    after = sim.project(m["formula"], m["axis"], mask=m.get("mask"), variables=V)
    sim.close()
    P.comm_destroy(comm)
    out = {"rows": [{k: (plain(v) if isinstance(v, dict) else v) for k, v in r.items()} for r in rows],
           "both": {k: plain(v) for k, v in both.items()}, "share": {k: plain(v) for k, v in share.items()},
           "wall": wall, "differ": differ, "not_exact": not_exact, "after": plain(after)}
    with open(f"{spec['out']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
