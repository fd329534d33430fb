"""What the four reductions share on the host side, without a GPU: the transport's long allgather
(pft_comm_allgather_any) and the merges of Simulation.diagnostics / means / formulas / histogram
with where="host", over loopback ranks on threads (the loopback allgather is a host barrier)."""
import ctypes as C

import numpy as np
import pytest

import _diag as D
import _formula as Fm
import _loopback as Lb
import porousfreezethaw_amd as P

LENGTHS = [1, 255, 256, 257, 512, 8240]   # below, at and above a round; two whole rounds; a long record


def _message(rank, n):
    """rank's n bytes, derived from (rank, index)"""
    i = np.arange(n, dtype=np.uint64)
    v = i * np.uint64(7) + np.uint64(131 * rank + 3) + (i >> np.uint64(8)) * np.uint64(rank + 1)
    return (v % np.uint64(251)).astype(np.uint8).tobytes()


@pytest.mark.parametrize("nprocs", [1, 2, 3])
def test_allgather_any_concatenates_in_rank_order(nprocs):
    """every rank receives rank 0's bytes, then rank 1's, ... for messages below, at and above a
    round of 256 bytes; a rank that passes all=NULL takes part in every round and disturbs nobody"""
    L = P.lib()

    def body(rank):
        comm = L.pft_comm_current()
        got = []
        for n in LENGTHS:
            every = C.create_string_buffer(nprocs * n)
            assert L.pft_comm_allgather_any(comm, _message(rank, n), n, every) == 0
            got.append(every.raw)
        for n in LENGTHS:   # the last rank discards; the others must still receive everything
            every = None if rank == nprocs - 1 else C.create_string_buffer(nprocs * n)
            assert L.pft_comm_allgather_any(comm, _message(rank, n), n, every) == 0
            got.append(None if every is None else every.raw)
        assert L.pft_comm_allgather_any(comm, None, 8, C.create_string_buffer(8 * nprocs)) == -2
        return got

    want = [b"".join(_message(r, n) for r in range(nprocs)) for n in LENGTHS]
    for rank, got in enumerate(Lb.run_slabs(nprocs, body)):
        assert got[:len(LENGTHS)] == want, f"rank {rank} of {nprocs}"
        assert got[len(LENGTHS):] == ([None] * len(LENGTHS) if rank == nprocs - 1 else want), f"rank {rank} of {nprocs}"


N1, N2, N3 = 13, 11, 9
FORMULAS = {"warm": "u-273.15", "icy": "p*(1-gl)"}
HIST = dict(formula="u", bins=1000, range=(200.0, 350.0), mask="p>0.5")   # 8 040 bytes: 32 rounds


def _answers(a, nprocs, rank):
    """the four entries' where="host" answers on rank's slab of a, reduced to what every rank shares
    (the raw record words where the entry exposes them)"""
    g = D.grid(N1, N2, N3, nprocs, rank)
    part = np.ascontiguousarray(a[:, g.first_row:g.first_row + g.n3])
    sim = P.Simulation(N1, N2, N3, Fm.L, 0, P.params_array(Fm.VARIABLES), nprocs=nprocs, rank=rank, initial=part,
                       init_solver=False)
    try:
        diag = sim.diagnostics(where="host")
        means = sim.means(where="host", per_plane=True)
        forms = sim.formulas(FORMULAS, variables=Fm.VARIABLES, where="host", per_plane=True)
        hist = sim.histogram(variables=Fm.VARIABLES, where="host", **HIST)
    finally:
        sim.close()
    out = {"diag": diag, "means": {k: v for k, v in means.items() if k.endswith(("_n", "_sum", "_mean"))},
           "means words": bytes(means["record"])}
    for name, d in forms.items():
        out["formula " + name] = {k: d[k] for k in Fm.KEYS}
        out["formula words " + name] = bytes(d["record"])
    out["hist"] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
    return out


@pytest.fixture(scope="module")
def one_slab():
    a = D.random_state(N1, N2, N3, 61)
    return a, _answers(a, 1, 0)


@pytest.mark.parametrize("nprocs", [2, 3])
def test_host_merges_over_loopback_ranks_equal_one_slab(one_slab, nprocs):
    """13x11x9 cut into 2 and 3 loopback ranks: diagnostics, means, two formulas and a masked histogram
    of 1 000 bins (a message of many rounds) with where="host" return on every rank what the single
    slab returns, the raw record words included"""
    a, want = one_slab
    assert want["hist"]["selected"] > 0 and sum(want["hist"]["counts"]) > 0
    for rank, got in enumerate(Lb.run_slabs(nprocs, lambda r: _answers(a, nprocs, r))):
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key] == want[key], f"rank {rank} of {nprocs}: {key}"
