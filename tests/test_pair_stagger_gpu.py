"""The pair kernels' staggered wave halves (merson_pair: waves 4-7 pass a plane step's barrier
between stage A and stage B, so their stage B runs in the next barrier interval, beside the other
half's top and stage A).  A stage B that reads a ring plane the other
half has already overwritten, or not yet written, computes from the wrong plane, so the initial
state here differs from plane to plane at every (x, y) in all three fields: the default initial
condition with the glass beads, plus a per-plane offset in u, p and gl.  gl stays within [0, 1] and
holds no -0.0, which keeps the GLX kernels on (stage B's gl neighbours come from stage A's ring: the
plane the stagger's hoisted reads protect); a second variant carries -0.0 in gl and selects the
kernels without it.

Pair kernels forced (PFT_OPT_PAIR = 2) against the stage launches, bit for bit and sign for sign on
the fields, and on t, h and both step counts, 6 attempted steps from tau = 1 s.  Shapes: the 40 x 20
tile alone (every ring position a mirror), 3 x 3 of them (an interior tile whose neighbours belong
to other waves of both halves), the 12-pair pitch's 20 x 34 tile; 4 planes in chunks of 1-4 (first
and last steps only: the late half's skipped barrier), 16 planes in chunks of 5, 8 and 16 (steady
triples); 200 x 200 x 16 in chunks of 4 (200 workgroups: every CU busy, the halves interleave under
load).  calc_modes 0 and 1 everywhere, 2 on one grid, u_noise_amp = 0.5 on one grid; 2 and 3 slabs
as processes over ipc (boundary chunks, the inline boundary's epilogue barrier).

Which kernels are staggered is the library's choice; the comparison is the same for the others,
and a library without the stagger passes this file too."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 6   # attempted steps (h starts at tau = 1 s)
TILE40 = (40, 20)      # one 40 x 20 tile
TILES9 = (120, 60)     # 3 x 3 tiles of 40 x 20
PITCH12 = (20, 34)     # one 20 x 34 tile, 12-pair row pitch
LOADED = (200, 200)    # 5 x 10 tiles of 40 x 20
GEOMETRY = {TILE40: (40, 20), TILES9: (40, 20), PITCH12: (20, 34), LOADED: (40, 20)}
SHAPES = [TILE40, TILES9, PITCH12]
PLANES = [(4, 1), (4, 2), (4, 3), (4, 4), (16, 5), (16, 8), (16, 16)]   # (n3, kz)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


@functools.lru_cache(maxsize=None)
def _case(noise):
    meta, _ = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    if noise:
        Pm = Pm.copy()
        Pm[O.PARAM_NAMES.index("u_noise_amp")] = noise
    return Pm, info


@functools.lru_cache(maxsize=None)
def _initial(dims, negzero):
    """the default initial condition with the glass beads plus a per-plane offset: no two
    neighbouring planes agree anywhere, in any field.  gl within [0, 1] without a -0.0 (GLX stays
    on); negzero: a few -0.0 in gl, which turns gl_keep (and with it GLX) off"""
    Pm, info = _case(0.0)
    n1, n2, n3 = dims
    sim = P.Simulation(n1, n2, n3, (info["L1"], info["L2"], info["L3"]), 0, Pm, beads=O.beads(), tau=1.0,
                       tau_min=info["tau_min"], delta=info["delta"], init_solver=False)
    ic = sim.interior().copy()
    sim.close()
    assert ic.shape == (3, n3, n2, n1)
    k = np.arange(n3, dtype=np.float64)[:, None, None]
    ic[0] += 1.0e-3 * (k + 1.0)                       # u: a millikelvin a plane
    ic[1] *= 1.0 + 1.0e-6 * (k + 1.0)
    ic[1] += 1.0e-6 * (k + 1.0)
    assert 0.0 <= ic[2].min() and ic[2].max() <= 1.0
    ic[2] = 0.875 * ic[2] + 2.0e-3 * (k + 1.0)        # n3 <= 48: at most 0.875 + 0.096
    assert 0.0 < ic[2].min() and ic[2].max() < 1.0 and not np.signbit(ic[2]).any()
    for q in range(3):
        assert (np.diff(ic[q], axis=0) != 0.0).all()
    if negzero:
        ic[2, 1:3, :3, 2:11] = -0.0
        assert np.signbit(ic[2]).sum() > 0
    assert np.isfinite(ic).all()
    ic.setflags(write=False)
    return ic


def _solve(dims, mode, negzero, pair, kz=None, noise=0.0):
    Pm, info = _case(noise)
    n1, n2, n3 = dims
    L = P.lib()
    L.pft_solver_set_option(P.PFT_OPT_PAIR, 2 if pair else 0)
    C.CDLL("libc.so.6").srand(1)       # u_noise comes from rand(): the same field for every run
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
            assert (tx.value, ty.value) == GEOMETRY[(n1, n2)]
        out = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, sim.interior().copy())
        sim.close()
    finally:
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    return out


@functools.lru_cache(maxsize=None)
def _reference(dims, mode, negzero, noise=0.0):
    """one launch per stage; computed once for all chunk lengths"""
    out = _solve(dims, mode, negzero, False, noise=noise)
    assert out[3] == STEPS and out[2] >= 1          # six attempts, at least one accepted
    assert np.isfinite(out[4]).all()
    out[4].setflags(write=False)
    return out


def _same(got, ref):
    assert got[:4] == ref[:4]
    assert np.array_equal(got[4], ref[4])
    assert np.array_equal(np.signbit(got[4]), np.signbit(ref[4]))


@pytest.mark.parametrize("negzero", [False, True], ids=["glx", "noglx"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n3,kz", PLANES)
@pytest.mark.parametrize("shape", SHAPES, ids=["tile40", "tiles9", "pitch12"])
def test_staggered_pairs_equal_stage_kernels(shape, n3, kz, mode, negzero):
    dims = shape + (n3,)
    _same(_solve(dims, mode, negzero, True, kz=kz), _reference(dims, mode, negzero))


@pytest.mark.parametrize("negzero", [False, True], ids=["glx", "noglx"])
def test_staggered_pairs_under_load(negzero):
    """200 workgroups of four planes each: every CU holds one, so the halves interleave as in the
    benchmark, and every chunk is first steps, one general step and last steps"""
    dims = LOADED + (16,)
    _same(_solve(dims, 0, negzero, True, kz=4), _reference(dims, 0, negzero))


@pytest.mark.parametrize("n3,kz", [(4, 3), (16, 8)])
def test_staggered_pairs_mode_2(n3, kz):
    dims = TILES9 + (n3,)
    _same(_solve(dims, 2, False, True, kz=kz), _reference(dims, 2, False))


@pytest.mark.parametrize("n3,kz", [(4, 2), (16, 8)])
def test_staggered_pairs_with_noise(n3, kz):
    """u_noise_amp = 0.5 K: every plane through the general body, with the noise loads"""
    dims = TILES9 + (n3,)
    _same(_solve(dims, 0, False, True, kz=kz, noise=0.5), _reference(dims, 0, False, noise=0.5))


def _run_slabs(tmp_path, nranks, dims, mode, negzero, kz):
    spec = dict(nranks=nranks, shm=f"/pft_stagger_{os.getpid()}_{uuid.uuid4().hex[:12]}", dims=list(dims), mode=mode,
                kz=kz, steps=STEPS, ic=str(tmp_path / "ic.npy"), out=str(tmp_path / "rank"))
    np.save(spec["ic"], _initial(dims, negzero))
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_pair_steady_worker.py"), str(path), str(r)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(nranks)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            outs.append(out.decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed ({p.returncode}):\n{outs[r][-3000:]}"
    return [dict(np.load(f"{spec['out']}.{r}.npz")) for r in range(nranks)]


@pytest.mark.parametrize("nranks,n3,kz,negzero", [(2, 16, 16, False), (3, 16, 5, True), (2, 4, 2, False)],
                         ids=["2x16-glx", "3x16-noglx", "2x4-glx"])
def test_staggered_slabs_equal_one_slab(tmp_path, nranks, n3, kz, negzero):
    """slabs as processes on one GPU: has_below / has_above chunks, the two-plane boundary chunks
    and the inline boundary's epilogue barrier, which both halves must reach"""
    dims = TILE40 + (n3 * nranks,)
    ref = _reference(dims, 0, negzero)
    res = _run_slabs(tmp_path, nranks, dims, 0, negzero, kz)
    for r in res:
        assert int(r["path"]) == 1 and int(r["pairs"]) == 1 and int(r["n3"]) == n3
        assert tuple(r["row"]) == (ref[0], ref[1], str(ref[2]), str(ref[3]), "2")
    full = np.concatenate([r["x"] for r in res], axis=1)
    assert np.array_equal(full, ref[4])
    assert np.array_equal(np.signbit(full), np.signbit(ref[4]))
