"""One rank of a two-process run of the f11 region snapshots over the ipc transport
(tests/test_region_gpu.py).  Started as its own process -- never forked from a process that uses the
GPU -- with:

    python tests/_ipc_region_worker.py <spec.json> <rank>

spec: {"nranks", "shm", "icond_file", "t0", "tau", "T", "regions": {name: [[start, stop, step] x 3
in k, j, i order]}, "out": prefix of the datasets to write, "res": result prefix}; the case is the
golden g20 (mode 0).  The rank reads its planes of icond_file on the device, solves to T and writes
its share of every region dataset "<out>.<name>.ncd" from the resident state (background writes,
then snapshot_wait).  Writes <res>.<rank>.json: t, h and per region its (kfirst, kcount, klocal) and
the words of Simulation.region() as hex."""
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
                       nprocs=n, rank=rank, icond_file=spec["icond_file"], t0=spec["t0"], tau=spec["tau"],
                       tau_min=info["tau_min"], delta=info["delta"])
    sim.solve_ex(spec["T"], 0, P.PFT_SOLVE_KEEP_DEVICE | P.PFT_SOLVE_REUSE_DEVICE)
    inf = P.snapshot_info(sim.t, sim.h, spec["T"], info["delta"], 0, snapshot=2, total_snapshots=4, comment="ipc")
    out = {"t": sim.t, "h": sim.h, "regions": {}}
    for name, triples in spec["regions"].items():
        sel = tuple(slice(*t) for t in triples)
        sim.snapshot_device(f"{spec['out']}.{name}.ncd", inf, wait=False, region=sel)
        share = sim.region(sel)
        out["regions"][name] = {"share": list(sim.region_share(sel)), "shape": list(share.shape),
                                "words": np.ascontiguousarray(share).view(np.uint64).tobytes().hex()}
    sim.snapshot_wait()
    sim.close()
    P.comm_destroy(comm)
    with open(f"{spec['res']}.{rank}.json", "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
