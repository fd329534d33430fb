"""calc_mode 2 ("Temp") bit for bit: the kernels evaluate cosh with the C library's algorithm restated
(porousfreezethaw_amd/csrc/pft_cosh.h).  The device function against its host twin and libm's cosh,
and mode 2's RHS, trajectory, pair kernels and slab decomposition against the reference's golden
vectors and the oracle, all by array_equal."""
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P
from test_gpu_parity import FLAVOURS, _loopback_run, make_sim
from test_pair_gpu import _loopback_pairs, _run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


# ---- the device function -----------------------------------------------------------------------

def _libm_cosh(x):
    """libm's own cosh, one call per element (numpy's may be its own vector code)"""
    m = C.CDLL(ctypes.util.find_library("m"))
    m.cosh.restype, m.cosh.argtypes = C.c_double, [C.c_double]
    return np.fromiter(map(m.cosh, x.tolist()), dtype=np.float64, count=x.size)


def _known():
    """the committed { bits of x, bits of cosh(x) } pairs of tests/native/cosh_check.c"""
    text = open(os.path.join(HERE, "native", "cosh_check.c")).read()
    pairs = re.findall(r"^\t\{0x([0-9a-f]{16})ULL, 0x([0-9a-f]{16})ULL\},", text, re.M)
    assert len(pairs) >= 40
    a = np.array([[int(p, 16), int(q, 16)] for p, q in pairs], dtype=np.uint64)
    return np.ascontiguousarray(a[:, 0]).view(np.float64), np.ascontiguousarray(a[:, 1]).view(np.float64)


def _hashed(n):
    """splitmix64 of 0 .. n-1 as doubles: every exponent, both signs, NaNs and infinities"""
    with np.errstate(over="ignore"):
        b = np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        b = (b ^ (b >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        b = (b ^ (b >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        b ^= b >> np.uint64(31)
    assert np.unique(b >> np.uint64(52)).size == 4096
    return b.view(np.float64)


def _assert_bitwise(got, ref, what):
    """equal bit for bit; a NaN equals any NaN"""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ"
    bad = np.flatnonzero(got.view(np.uint64)[~nan] != ref.view(np.uint64)[~nan])
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} results differ"


ARGS = {"hashed": lambda: _hashed(1 << 22),
        "uniform40": lambda: np.random.default_rng(2).uniform(-40.0, 40.0, 1 << 20),   # gamma (u - u*)
        "special": lambda: _known()[0]}


@pytest.mark.parametrize("which", sorted(ARGS))
def test_device_cosh_equals_host_twin_and_libm(which):
    x = ARGS[which]()
    got = P.cosh_device(x)
    _assert_bitwise(got, P.cosh_host(x), "device against the host twin")
    _assert_bitwise(got, _libm_cosh(x), "device against libm")
    if which == "special":
        _assert_bitwise(got, _known()[1], "device against the committed known answers")


# ---- the RHS and the trajectory against the reference's golden vectors -------------------------

@pytest.mark.parametrize("case,key", [("g20", "ic"), ("ragged", "state")])
@pytest.mark.parametrize("tag", ["t0", "t1"])
@pytest.mark.parametrize("flavour", sorted(FLAVOURS))
def test_rhs_mode2_bitwise(case, key, tag, flavour):
    meta, A = O.load_case(case)
    sim, Pm, info = make_sim(meta, A[key], mode=2, init_solver=False, flavour=flavour)
    dw, _ = P.rhs(sim, meta["rhs_times"][tag])
    K = dw.reshape((3,) + sim.N)[:, 2:-2, 2:-2, 2:-2]
    sim.close()
    assert np.array_equal(K, A[f"rhs_m2_{tag}"])


@pytest.mark.parametrize("flavour,gl_static", [(f, False) for f in sorted(FLAVOURS) + ["pairs"]] + [("default", True)])
def test_trajectory_mode2_bitwise(flavour, gl_static):
    """RK_MPI_SA_solve in calc_mode 2 to the three snapshot times: t, h, step counts, the return
    code and the fields equal the reference's, every kernel flavour and the pair kernels forced"""
    meta, A = O.load_case("g20")
    pair = flavour == "pairs"
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 2 if pair else 1)
    got = []
    try:
        sim, Pm, info = make_sim(meta, A["traj_m2_ic"], mode=2, gl_static=gl_static,
                                 flavour="fusedauto" if pair else flavour)
        try:
            for T in meta["traj_times"]:
                rc = sim.solve(T)
                got.append((sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, rc, sim.interior()))
            st = sim.stats()
        finally:
            sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    for i, g in enumerate(got):
        ref = meta["traj_m2"][i]
        assert g[:5] == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
        assert np.array_equal(g[5], A[f"traj_m2_state{i}"])
    assert st.path == 1 and bool(st.pairs) == pair


# ---- pair kernels, stage launches and the oracle -----------------------------------------------

# a plane narrower than a pair tile and one with a partial tile (test_pair_gpu.GRIDS)
@pytest.mark.parametrize("dims", [(18, 12, 30), (100, 36, 40)])
def test_mode2_pairs_stages_oracle(dims):
    """12 attempted steps of mode 2 from the default IC with the beads: pair kernels == one launch
    per stage == the oracle"""
    got, used, ic, info, Pm = _run(dims, 2, True, 12)
    ref, unused, *_ = _run(dims, 2, False, 12)
    assert used == 1 and unused == 0
    assert got[:4] == ref[:4]
    assert np.array_equal(got[4], ref[4])
    n1, n2, n3 = dims
    res = O.solve(dict(info, n1=n1, n2=n2, n3=n3), Pm, 2, ic, 0.0, 1.0, [1e9], max_steps_total=12)[0]
    assert got[:4] == (res[0].hex(), res[1].hex(), res[2], res[3])
    assert np.array_equal(got[4], res[5])


# ---- slabs -------------------------------------------------------------------------------------

@pytest.mark.parametrize("nprocs", [2, 3])
@pytest.mark.parametrize("pair", [False, True])
def test_mode2_multislab_loopback_golden(nprocs, pair):
    """g20 in mode 2 on 2 and 3 slabs (loopback transport on one GPU), one launch per stage and the
    pair kernels: the reference's single-rank trajectory bit for bit"""
    meta, A = O.load_case("g20")
    times = meta["traj_times"]
    if pair:
        out = _loopback_pairs(meta, A["traj_m2_ic"], nprocs, times, mode=2)
        assert all(o[1] == 1 for o in out)
        runs = [[(float.fromhex(r[0]), float.fromhex(r[1])) + tuple(r[2:]) for r in o[0]] for o in out]
    else:
        runs = _loopback_run(meta, A["traj_m2_ic"], nprocs, times, mode=2, flavour="default")
    for i in range(len(times)):
        ref = meta["traj_m2"][i]
        for r in runs:
            assert r[i][:5] == (float.fromhex(ref[0]), float.fromhex(ref[1]), ref[2], ref[3], ref[4])
        assert np.array_equal(np.concatenate([r[i][5] for r in runs], axis=1), A[f"traj_m2_state{i}"])
