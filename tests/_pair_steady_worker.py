"""One rank of tests/test_pair_steady_gpu.py's slab runs over the ipc transport: its own process,
started before it touches the GPU, pair kernels forced, a forced z-chunk length.

    python tests/_pair_steady_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "dims": [n1, n2, n3], "mode", "kz", "steps", "ic": .npy path or null (the
       default initial condition with the glass beads), "out": output prefix}
Writes <out>.<rank>.npz: (t.hex, h.hex, steps, steps_total), this slab's interior, stats.pairs."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _oracle as O  # noqa: E402
import porousfreezethaw_amd as P  # noqa: E402


def main():
    spec = json.load(open(sys.argv[1]))
    rank = int(sys.argv[2])
    n = spec["nranks"]
    comm = P.comm_init_ipc(n, rank, spec["shm"], 0)
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 2)
    meta, _ = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    n1, n2, n3 = spec["dims"]
    ic = np.load(spec["ic"]) if spec.get("ic") else None
    sim = P.Simulation(n1, n2, n3, (info["L1"], info["L2"], info["L3"]), spec["mode"], Pm, nprocs=n, rank=rank,
                       initial=ic, beads=None if ic is not None else O.beads(), tau=1.0, tau_min=info["tau_min"],
                       delta=info["delta"], tile=2, recompute=True, kz=spec["kz"])
    rc = sim.solve_ex(1e9, spec["steps"], 0)
    st = sim.stats()
    row = [sim.t.hex(), sim.h.hex(), str(sim.system.steps), str(sim.system.steps_total), str(rc)]
    x = sim.interior()
    n3_slab = sim.grid.n3
    sim.close()
    P.comm_destroy(comm)
    np.savez(f"{spec['out']}.{rank}.npz", row=np.array(row), x=x, pairs=st.pairs, path=st.path, n3=n3_slab)


if __name__ == "__main__":
    main()
