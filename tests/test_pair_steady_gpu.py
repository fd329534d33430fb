"""The pair kernels' steady-state plane step (merson_pair: step() with st = 1).  A z-chunk's
plane steps whose tests on the chunk position are all decided -- no wall plane, not the chunk's
first two or last steps, look-ahead and next-plane store running -- take a body of their own with
those tests compiled out, in triples (the register rotation's period); the chunk's first triple and
its last steps take the general body.  The existing pair tests use slabs of at most 7 planes with
chunks of 1-4 planes and never enter the steady body; here slabs of 16 planes are cut into chunks of
4 .. 9 and 16 planes, so that chunks without a steady triple, with exactly one, with two and three,
with one to five general steps after the last steady triple (the steady range ends in each of the
three phases), between two chunks, at one wall and spanning both walls all occur.

The steady range is restated here from the derivation beside the z-loop (_steady below) and the
cases are asserted against it.  Pair kernels forced (PFT_OPT_PAIR = 2) against the stage launches,
bit for bit and sign for sign, 6 attempted steps from tau = 1 s (rejections included), on the
40 x 20 tile (one tile, every ring position a mirror; 3 x 3 tiles with an interior one) and on the
12-pair pitch's 20 x 34 tile, calc_modes 0 and 1 (2 on one grid), with and without GLX (a -0.0 in
gl).  u_noise_amp != 0 takes the general body for every plane (the steady body is compiled without
u_noise); the same chunks run with it.  2 and 3 slabs as processes over the ipc transport run
has_below / has_above chunks and the two-plane boundary chunks beside steady interior chunks.

Which kernels hold the steady loop is the library's choice (the 22-pair
pitch, but for pair 4+5 in calc_mode 0 without GLX); the others run the same chunks through the
single z-loop, and the comparison is the same.  The parent commit's library, which has no steady
body, passes this file too: every comparison is against the stage kernels."""
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
STEPS = 6   # attempted steps (h starts at tau = 1 s: rejections included)
N3 = 16
KZS = [4, 5, 6, 7, 8, 9, 16]
TILE40 = (40, 20, N3)      # one 40 x 20 tile
TILES9 = (120, 60, N3)     # 3 x 3 tiles of 40 x 20
PITCH12 = (20, 34, N3)     # one 20 x 34 tile, 12-pair row pitch
GEOMETRY = {TILE40: (40, 20), TILES9: (40, 20), PITCH12: (20, 34)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


def _steady(n3, kz, k_begin=0, k_end=None, wlo=True, whi=True):
    """(steady triples, general steps after the last one) of every chunk of [k_begin, k_end) cut
    into kz planes -- merson_pair's chunk bounds and the steady range of its z-loop: a triple of
    steps starting at plane mm = mA0 + 3 j is steady when mm >= kb + 2 and mm + 4 <= mlast"""
    k_end = n3 if k_end is None else k_end
    out = []
    for kb in range(k_begin, k_end, kz):
        ke = min(kb + kz, k_end)
        mA0 = kb - 1 if kb > 0 else (0 if wlo else -1)
        mA1 = ke if ke < n3 else (n3 - 1 if whi else n3)
        mlast = min(mA1 + 1, n3 - 1 if whi else n3 + 1)
        mm, nt = mA0 + 3, 0
        while mm + 4 <= mlast:
            assert mm >= kb + 2          # mA0 >= kb - 1: true from the second triple on
            nt += 1
            mm += 3
        out.append((nt, ke - mm + 1))
    return out


def test_chunk_lengths_cover_the_steady_range():
    """what the chunk lengths of this file run, by the range formula (no GPU work)"""
    got = {kz: _steady(N3, kz) for kz in KZS}
    assert got[4] == [(0, 2), (0, 3), (0, 3), (0, 3)]              # no steady triple at all
    assert got[5] == [(0, 3), (1, 1), (0, 4), (0, 0)]              # exactly one, between two chunks
    assert got[6] == [(1, 1), (1, 2), (0, 3)]                      # at the bottom wall; none at the top wall
    assert got[7] == [(1, 2), (1, 3), (0, 1)]
    assert got[8] == [(1, 3), (1, 4)]                              # one in the chunk at each wall
    assert got[9] == [(2, 1), (1, 3)]
    assert got[16] == [(3, 5)]                                     # one chunk spanning both walls
    tails = {t % 3 for v in got.values() for n, t in v if n}
    assert tails == {0, 1, 2}                                      # the range ends in each phase
    # a slab between two others: its interior chunk [2, n3 - 2) and the whole slab in one chunk;
    # the two-plane boundary chunks have no steady triple
    assert _steady(N3, 16, 2, N3 - 2, False, False) == [(3, 2)]
    assert _steady(N3, 16, 0, N3, False, True) == [(4, 3)]
    assert [n for n, _ in _steady(N3, 2, 0, 2, False, False)] == [0]


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
    """the default initial condition with the glass beads; negzero: some -0.0 in gl, which turns
    gl_keep (and with it GLX) off"""
    Pm, info = _case(0.0)
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
            assert (tx.value, ty.value) == GEOMETRY[(n1, n2, N3)]
        out = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, sim.interior().copy())
        sim.close()
    finally:
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    return out


@functools.lru_cache(maxsize=None)
def _reference(dims, mode, negzero, noise=0.0):
    """one launch per stage; computed once for all chunk lengths"""
    out = _solve(dims, mode, negzero, False, noise=noise)
    assert out[2] < out[3]                 # a rejected step among the six
    out[4].setflags(write=False)
    return out


def _same(got, ref):
    assert got[:4] == ref[:4]
    assert np.array_equal(got[4], ref[4])
    assert np.array_equal(np.signbit(got[4]), np.signbit(ref[4]))


@pytest.mark.parametrize("negzero", [False, True], ids=["glx", "noglx"])
@pytest.mark.parametrize("kz", KZS)
@pytest.mark.parametrize("dims", [TILE40, TILES9, PITCH12])
def test_steady_chunks_equal_stage_kernels(dims, kz, negzero):
    _same(_solve(dims, 0, negzero, True, kz=kz), _reference(dims, 0, negzero))


@pytest.mark.parametrize("negzero", [False, True], ids=["glx", "noglx"])
@pytest.mark.parametrize("kz", [5, 8, 16])     # one triple between chunks; one at each wall; three, both walls
@pytest.mark.parametrize("dims", [TILE40, TILES9, PITCH12])
def test_steady_chunks_mode_1(dims, kz, negzero):
    _same(_solve(dims, 1, negzero, True, kz=kz), _reference(dims, 1, negzero))


@pytest.mark.parametrize("kz", [7, 16])
def test_steady_chunks_mode_2(kz):
    _same(_solve(TILE40, 2, False, True, kz=kz), _reference(TILE40, 2, False))


@pytest.mark.parametrize("kz", [8, 16])
def test_chunks_with_noise_equal_stage_kernels(kz):
    """u_noise_amp = 0.5 K (the gnoise setting): zc + nz[s] in both stages, every plane through the
    general body; without u_noise the same chunks run steady triples (the tests above)"""
    _same(_solve(TILE40, 0, False, True, kz=kz, noise=0.5), _reference(TILE40, 0, False, noise=0.5))


def _run_slabs(tmp_path, nranks, dims, mode, negzero, kz):
    spec = dict(nranks=nranks, shm=f"/pft_steady_{os.getpid()}_{uuid.uuid4().hex[:12]}", dims=list(dims), mode=mode,
                kz=kz, steps=STEPS, ic=None, out=str(tmp_path / "rank"))
    if negzero:
        spec["ic"] = str(tmp_path / "ic.npy")
        np.save(spec["ic"], _initial(dims, True))
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


@pytest.mark.parametrize("nranks,negzero", [(2, False), (3, True)], ids=["2-glx", "3-noglx"])
def test_steady_slabs_equal_one_slab(tmp_path, nranks, negzero):
    """slabs of 16 planes, one process each on one GPU: every slab's interior planes are one chunk
    with steady triples (the formula above), beside the two-plane boundary chunks and the chunks
    next to a neighbour, which have none or start and end with general steps"""
    dims = (40, 20, N3 * nranks)
    ref = _reference(dims, 0, negzero)
    res = _run_slabs(tmp_path, nranks, dims, 0, negzero, 16)
    for r in res:
        assert int(r["path"]) == 1 and int(r["pairs"]) == 1 and int(r["n3"]) == N3
        assert tuple(r["row"]) == (ref[0], ref[1], str(ref[2]), str(ref[3]), "2")
    full = np.concatenate([r["x"] for r in res], axis=1)
    assert np.array_equal(full, ref[4])
    assert np.array_equal(np.signbit(full), np.signbit(ref[4]))
