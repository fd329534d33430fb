"""The 40 x 20 pair tile's positions beyond the 512 threads (merson_pair): the last lanes of the
last wave load them into the operand sets that are dead for a load-only lane, one step ahead, and
store their stage-A input a step later.  The register rotation of the three unrolled phases, the
prologue's hand-over and the chunk's last steps (where the look-ahead stops) are exercised with
z-chunks of 1 .. 4 planes on slabs of 4 and 7 planes: a chunk ends in each of the three phases and
is shorter than the look-ahead.  Pair kernels forced (PFT_OPT_PAIR = 2) against the stage launches,
bit for bit, with and without GLX (a -0.0 in gl turns gl_keep off), calc_modes 0 and 1; every step
runs both pair kernels (2+3 and 4+5)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

STEPS = 6   # attempted steps (h starts at tau = 1 s: rejections included)

# (40, 20, n3): one tile, every ring position a mirror; (120, 60, 7): 3 x 3 tiles, the middle one's
# extra positions are real neighbours
GRIDS = [(40, 20, 4), (40, 20, 7), (120, 60, 7)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


@functools.lru_cache(maxsize=None)
def _case():
    meta, _ = O.load_case("g20")
    return O.params_from_meta(meta)


@functools.lru_cache(maxsize=None)
def _initial(dims, negzero):
    """the default initial condition with the glass beads; negzero: some -0.0 in gl (the state of
    test_pair_gpu.py::test_pair_gl_negative_zero, its z range cut to the slab)"""
    Pm, info = _case()
    n1, n2, n3 = dims
    sim = P.Simulation(n1, n2, n3, (info["L1"], info["L2"], info["L3"]), 0, Pm, beads=O.beads(), tau=1.0,
                       tau_min=info["tau_min"], delta=info["delta"], init_solver=False)
    ic = sim.interior().copy()
    sim.close()
    if negzero:
        ic[2, :, :5, :] = 0.0
        ic[2, 1:3, :3, 2:11] = -0.0
        assert np.signbit(ic[2]).sum() > 0
    ic.setflags(write=False)
    return ic


def _solve(dims, mode, negzero, pair, kz=None):
    Pm, info = _case()
    n1, n2, n3 = dims
    L = P.lib()
    L.pft_solver_set_option(P.PFT_OPT_PAIR, 2 if pair else 0)
    try:
        sim = P.Simulation(n1, n2, n3, (info["L1"], info["L2"], info["L3"]), mode, Pm,
                           initial=_initial(dims, negzero), tau=1.0, tau_min=info["tau_min"], delta=info["delta"],
                           tile=2, recompute=True, kz=kz)
        assert sim.solve_ex(1e9, STEPS, 0) == 2
        st = sim.stats()
        assert st.path == 1 and st.pairs == (1 if pair else 0)
        if pair:
            tx, ty = C.c_int(), C.c_int()
            L.pft_solver_slab.restype = C.c_void_p
            L.pft_slab_pair_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            assert L.pft_slab_pair_geometry(L.pft_solver_slab(), C.byref(tx), C.byref(ty)) == 0
            assert (tx.value, ty.value) == (40, 20)
        out = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, sim.interior().copy())
        sim.close()
    finally:
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    return out


@functools.lru_cache(maxsize=None)
def _reference(dims, mode, negzero):
    """one launch per stage; computed once for all chunk lengths"""
    out = _solve(dims, mode, negzero, False)
    out[4].setflags(write=False)
    return out


@pytest.mark.parametrize("negzero", [False, True], ids=["glx", "noglx"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kz", [1, 2, 3, 4])
@pytest.mark.parametrize("dims", GRIDS)
def test_pair_extras_equal_stage_kernels(dims, kz, mode, negzero):
    ref = _reference(dims, mode, negzero)
    got = _solve(dims, mode, negzero, True, kz=kz)
    assert got[:4] == ref[:4]
    assert np.array_equal(got[4], ref[4])
    assert np.array_equal(np.signbit(got[4]), np.signbit(ref[4]))
