"""Every stage route on dense edge-value states and on other parameters than the default ones.

The states come from tests/_dense.py: every cell differs from its neighbours, so a wrong neighbour,
mirrored slot or ring row changes K at that cell, and p and gl sit below, on and above the clamps
and thresholds of the right-hand side (tests/test_oracle_golden.py shows both, and pins the oracle
to the reference on them).  The three restatements of the right-hand side -- rhs_cell (cache and LDS
tile kernels), rhs_cell_f (merson_fused) and pair_rhs (merson_pair) -- are compared with the
reference's own golden (tests/golden/gedge, gedgep: 44 x 24 x 6, three pair tiles and 2 x 2 fused16
tiles) and, on grids of several tiles a side (tests/_dense.py lists them), with the oracle: stage 1 through
the model's RHS entry, stages 1-5, the error norm and the step control through six attempted steps
from h = 1 s (rejections included).  Everything bit for bit, calc_mode 2 included.
"""
import ctypes as C

import numpy as np
import pytest

import _dense as D
import _oracle as O
import porousfreezethaw_amd as P
from _loopback import run_slabs

pytestmark = pytest.mark.gpu

T_RHS = 100.0

# kernel flavours: (tile width, recompute stage inputs), as tests/test_gpu_parity.py
FLAVOURS = {"cache": (0, False), "fused32": (32, True), "fused16": (16, True), "default": (1, True),
            "fusedauto": (2, True)}
# stage routes: (flavour, PFT_OPT_PAIR, kz); PFT_OPT_PAIR 2: the pair kernels wherever they fit
ROUTES = {"cache": ("cache", 0, None), "fused16": ("fused16", 0, None), "fused32": ("fused32", 0, None),
          "fusedauto": ("fusedauto", 0, None), "default": ("default", 0, None),
          "pairs": ("fusedauto", 2, None), "pairs-kz2": ("fusedauto", 2, 2)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


def _sim(info, Pm, x, mode, flavour, **kw):
    tile, recompute = FLAVOURS[flavour]
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        initial=np.array(x), tau=1.0, tau_min=info["tau_min"], delta=info["delta"], tile=tile,
                        recompute=recompute, **kw)


def _rhs(info, Pm, x, mode, flavour):
    sim = _sim(info, Pm, x, mode, flavour, init_solver=False)
    dw, _ = P.rhs(sim, T_RHS)
    K = dw.reshape((3,) + sim.N)[:, 2:-2, 2:-2, 2:-2]
    sim.close()
    return K


def _pair_tile(L):
    tx, ty = C.c_int(), C.c_int()
    L.pft_solver_slab.restype = C.c_void_p
    L.pft_slab_pair_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert L.pft_slab_pair_geometry(L.pft_solver_slab(), C.byref(tx), C.byref(ty)) == 0
    return tx.value, ty.value


def _six_steps(info, Pm, x, mode, route, gl_static=False, noise=0.0):
    """six attempted steps from h = 1 s on one slab: ((t, h, steps, steps_total), state, pair tile or
    None, the u_noise field or None); asserts the route taken"""
    flavour, pair, kz = ROUTES[route]
    if noise:
        Pm = Pm.copy()
        Pm[O.PARAM_NAMES.index("u_noise_amp")] = noise
        C.CDLL("libc.so.6").srand(1)       # the field comes from rand() (equation.c:450-456)
    L = P.lib()
    L.pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _sim(info, Pm, x, mode, flavour, kz=kz, gl_static=gl_static)
        field = None
        if noise:
            n3, n2, n1 = info["n3"], info["n2"], info["n1"]
            field = np.ctypeslib.as_array(L.pft_model_noise(), shape=(n3, n2, n1)).copy()
            assert np.abs(field).max() > 0.2
        assert sim.solve_ex(1e9, D.ATTEMPTS, 0) == 2
        st = sim.stats()
        tile = _pair_tile(L) if pair else None
        rec = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total)
        got = sim.interior()
        sim.close()
    finally:
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    assert st.path == 1
    if pair:
        assert st.pairs == 1
        assert info["n1"] > tile[0] or info["n2"] > tile[1], tile      # more than one tile in the plane
    else:
        assert st.pairs == 0
    return rec, got, tile, field


def _golden_params(case, mode):
    meta, A, Pm, info = D.golden(case)
    assert meta[f"m{mode}_params"]["calc_mode"] == mode
    return meta, A, Pm, info


# ---- stage 1 through the model's RHS entry -----------------------------------------------------

@pytest.mark.parametrize("case", ["gedge", "gedgep"])
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_rhs_golden(case, mode, flavour):
    """the reference's own K on the edge state, default and perturbed constants"""
    meta, A, Pm, info = _golden_params(case, mode)
    assert meta["rhs_time"] == T_RHS
    assert np.array_equal(_rhs(info, Pm, A["state"], mode, flavour), D.golden_rhs(A, mode))


@pytest.mark.parametrize("dims", D.GRIDS[:2])
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_rhs_larger_grids(dims, perturbed, mode, flavour):
    """66 x 38 x 7 and 130 x 70 x 5 with h1 != h2 != h3, against the oracle"""
    info, Pm, x = D.grid_case(dims, perturbed)
    assert len({info["L1"] / info["n1"], info["L2"] / info["n2"], info["L3"] / info["n3"]}) == 3
    assert np.array_equal(_rhs(info, Pm, x, mode, flavour), D.oracle_rhs(dims, perturbed, mode, T_RHS))


# ---- six attempted steps from h = 1 s -------------------------------------------------------------

@pytest.mark.parametrize("case,mode", [("gedge", m) for m in D.MODES] + [("gedgep", 0), ("gedgep", 1)])
@pytest.mark.parametrize("route", list(ROUTES))
def test_six_steps_golden(case, mode, route):
    """the reference's own record and state after its first six attempts"""
    meta, A, Pm, info = _golden_params(case, mode)
    rec, got, _, _ = _six_steps(info, Pm, A["state"], mode, route)
    assert rec == D.golden_record(meta, mode)
    assert np.array_equal(got, D.golden_final(A, mode))


def _against_oracle(dims, mode, route, perturbed=False):
    info, Pm, x = D.grid_case(dims, perturbed)
    rec, got, tile, _ = _six_steps(info, Pm, x, mode, route)
    ref_rec, ref = D.oracle_steps(dims, perturbed, mode)
    assert rec == ref_rec
    assert np.array_equal(got, ref)
    return tile


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("route", ["pairs", "pairs-kz2", "fusedauto"])
def test_six_steps_interior_tile(mode, route):
    """120 x 60 x 6: the 40 x 20 pair tile 3 x 3 times, so one tile touches no wall"""
    tile = _against_oracle((120, 60, 6), mode, route)
    if route != "fusedauto":
        assert tile == (40, 20)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("route", list(ROUTES))
def test_six_steps_partial_tiles(mode, route):
    """66 x 38 x 7: partial tiles in x and y, an odd number of planes"""
    _against_oracle((66, 38, 7), mode, route)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("route", ["cache", "fused16", "fusedauto", "pairs"])
def test_six_steps_wide_plane(mode, route):
    """130 x 70 x 5: several tiles a side for every kernel, the fewest planes a slab marches"""
    _against_oracle((130, 70, 5), mode, route)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("route", ["pairs", "fusedauto"])
def test_six_steps_perturbed_constants(mode, route):
    """66 x 38 x 7 with every physical constant scaled on its own (alpha apart from water_rho *
    water_cp): a swapped or re-associated constant that rounds the same for the default values"""
    _against_oracle((66, 38, 7), mode, route, perturbed=True)


# ---- slabs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nprocs", [2, 3])
@pytest.mark.parametrize("route", ["pairs", "fused32"])
@pytest.mark.parametrize("grid", ["gedge", (66, 38, 7)])
@pytest.mark.parametrize("mode", [0, 2])
def test_six_steps_slabs(nprocs, route, grid, mode):
    """2 and 3 slabs of 2-4 planes over the loopback transport (6 planes: 3 + 3 and 2 + 2 + 2; 7:
    4 + 3 and 3 + 2 + 2): the concatenation equals the single-slab reference"""
    if grid == "gedge":
        meta, A, Pm, info = _golden_params("gedge", mode)
        x, ref_rec, ref = A["state"], D.golden_record(meta, mode), D.golden_final(A, mode)
    else:
        info, Pm, x = D.grid_case(grid, False)
        ref_rec, ref = D.oracle_steps(grid, False, mode)
    flavour, pair, kz = ROUTES[route]

    def body(r):
        sim = _sim(info, Pm, x, mode, flavour, nprocs=nprocs, rank=r)
        assert 2 <= sim.grid.n3 <= 4
        assert sim.solve_ex(1e9, D.ATTEMPTS, 0) == 2
        out = ((sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total), sim.interior(),
               sim.stats().pairs)
        sim.close()
        return out

    out = run_slabs(nprocs, body, pair=pair)                 # the option is per host thread
    for rec, _, pairs in out:
        assert rec == ref_rec
        assert pairs == (1 if pair else 0)
    assert np.array_equal(np.concatenate([o[1] for o in out], axis=1), ref)


# ---- gl_static and u_noise ---------------------------------------------------------------------------

@pytest.mark.parametrize("gl_static,noise", [(True, 0.0), (False, 0.5), (True, 0.5)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("route", ["pairs", "fusedauto"])
def test_six_steps_gl_static_and_noise(gl_static, noise, mode, route):
    """gl read from x (gl_static) and u_noise_amp = 0.5 K (equation.c:450-456, 676-687) on
    66 x 38 x 7, the oracle given the field the library drew"""
    dims = (66, 38, 7)
    info, Pm, x = D.grid_case(dims, False)
    rec, got, _, field = _six_steps(info, Pm, x, mode, route, gl_static=gl_static, noise=noise)
    ref_rec, ref = D.oracle_steps(dims, False, mode, noise=field)
    if noise:
        assert ref_rec != D.oracle_steps(dims, False, mode)[0]          # the noise is seen
    assert rec == ref_rec
    assert np.array_equal(got, ref)
