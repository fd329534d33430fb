"""The inline boundary placements at the edge of the ends-first fallback (csrc/pft_zplan.h).

44 x 24 x n3 with n3 = 6, the smallest slab on which ends-first holds (three chunks of two planes),
and its nearest fallbacks 5 and 7 (the cost model gives kz = 1 there; the interior of 5 is a single
plane): one process exchanging with itself over the copy engines, the pair kernels forced and stage
launches, six attempted steps from h = 1 s on the dense edge-value state (tests/_dense.py).  t, h, the
step counts and the fields equal the same run with no communicator bit for bit, and the launches are
cut as they were before the plan moved into pft_zplan.h.
"""
import ctypes as C
import os
import uuid

import numpy as np
import pytest

import _dense as D
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

PLACEMENTS = {"inline": {"PFT_CE_BND": "4", "PFT_CE_STAGE_INLINE": "1"},
              "ends": {"PFT_CE_BND": "5", "PFT_CE_BND45": "5", "PFT_CE_STAGE_INLINE": "1"}}

# pft_slab_launch_geometry after the run, (boundary launch, nwg, kz, ntile) of the launch that ended
# each stage: literals, what the library of the commit before the plan moved into pft_zplan.h
# reported for these cases (probed once on an MI355X with geometry() below).  Three tiles a plane
# on both routes (pair tiles of 16 x 24, automatic fused tiles of 64 x 8), every launch of a run
# cut alike.  Pairs (stage 1 and the pairs, which end stages 3 and 5, inline): n3 = 6 under "ends"
# three chunks of two planes; otherwise, and under the fallback, two boundary chunks a tile and the
# interior [2, n3 - 2) plane by plane.  Stage launches (not between pair kernels: the one-plane
# boundary launch first, so the last launch of a stage is its interior [1, n3 - 1), plane by plane).
_PAIRS = {("ends", 6): (0, 9, 2, 3), ("ends", 5): (0, 9, 1, 3), ("ends", 7): (0, 15, 1, 3),
          ("inline", 5): (0, 9, 1, 3), ("inline", 6): (0, 12, 1, 3), ("inline", 7): (0, 15, 1, 3)}
_STAGES = {5: (0, 9, 1, 3), 6: (0, 12, 1, 3), 7: (0, 15, 1, 3)}


def expected_geometry(placement, pair, n3):
    if pair:
        return {stage: _PAIRS[placement, n3] for stage in (1, 3, 5)}
    return {stage: _STAGES[n3] for stage in (1, 2, 3, 4, 5)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


def geometry():
    L = P.lib()
    L.pft_solver_slab.restype = C.c_void_p
    L.pft_slab_launch_geometry.argtypes = [C.c_void_p] + [C.c_int] + [C.POINTER(C.c_int)] * 3
    slab = L.pft_solver_slab()
    out = {}
    for stage in range(1, 6):
        nwg, kz, ntile = C.c_int(), C.c_int(), C.c_int()
        bnd = L.pft_slab_launch_geometry(slab, stage, C.byref(nwg), C.byref(kz), C.byref(ntile))
        if bnd >= 0:
            out[stage] = (bnd, nwg.value, kz.value, ntile.value)
    return out


def run(n3, pair, exchange):
    """six attempted steps on 44 x 24 x n3; exchange: with itself over the copy engines (PFT_IPC_CE=1
    and the placement's options in the environment), else no communicator.  ((t, h, steps,
    steps_total), state, launch geometry)"""
    info, Pm, x = D.grid_case((44, 24, n3), False)
    L = P.lib()
    comm = None
    L.pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        if exchange:
            comm = P.comm_init_ipc(1, 0, f"/pft_zplan_{os.getpid()}_{uuid.uuid4().hex[:12]}")
            assert L.pft_comm_set_self_exchange(comm, 1) == 0
            assert L.pft_comm_copy_engine(comm) == 1 and L.pft_comm_boundary_first(comm) == 1
        sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                           initial=np.array(x), tau=1.0, tau_min=info["tau_min"], delta=info["delta"], tile=2)
        assert sim.solve_ex(1e9, D.ATTEMPTS, 0) == 2
        assert sim.stats().pairs == (1 if pair else 0)
        out = ((sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total), sim.interior(), geometry())
        sim.close()
    finally:
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
        if comm is not None:
            P.comm_destroy(comm)
    return out


_alone = {}


def alone(n3, pair):
    """the run with no communicator, once per case"""
    if (n3, pair) not in _alone:
        rec, state, _ = run(n3, pair, False)
        state.setflags(write=False)
        _alone[n3, pair] = (rec, state)
    return _alone[n3, pair]


@pytest.mark.parametrize("n3", [5, 6, 7])
@pytest.mark.parametrize("pair", [2, 0])
@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
def test_inline_placements_at_the_fallback_edge(placement, pair, n3, monkeypatch):
    ref_rec, ref = alone(n3, pair)
    monkeypatch.setenv("PFT_IPC_CE", "1")
    for k, v in PLACEMENTS[placement].items():
        monkeypatch.setenv(k, v)
    rec, state, geo = run(n3, pair, True)
    print(placement, pair, n3, geo)
    assert rec == ref_rec
    assert np.array_equal(state, ref)
    assert geo == expected_geometry(placement, pair, n3)
