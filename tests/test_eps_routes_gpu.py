"""The error norm by cell position, multiplier and delta mode, through every route it takes on the
device (hybrid2.c:507-524, :578-611).

Every accepted or rejected step is decided by the maximum over all cells of em[q] |0.2 K1 - 0.9 K3 +
0.8 K4 - 0.1 K5|.  On the default initial condition that maximum always sits in the freezing front, so
a kernel that lost the contribution of any other cell would pass every other test.  Here the maximum
is put where a kernel could lose it.

The probe state: u = top_temp1, p = 0, gl = 0 everywhere and p = 1 at ONE target cell; tau = 1 s,
calc_mode 0, three attempted steps.  The g20 model parameters; the domain is sized so that a cell is
what it is on 40 x 20 x 7 at g20's L1 x L2 x L3 (where the probe was worked out): with g20's domain
itself a finer grid's first attempt at tau = 1 s overflows to 1e31 and symmetric neighbours of the
target tie for the maximum, so no single cell could be shown to matter.  For every target the CPU
oracle (pft_or_solve_ex) must say, or the test fails:
  - the arg-max of all three attempts is the target cell itself;
  - the same run with that one cell left out of the maximum has another h after the first attempt.
So a device result equal to the oracle's, bit for bit, proves that the target's contribution arrived.

Targets are derived from the geometry the slab reports (tile_geometry, pft_slab_pair_geometry,
pft_slab_launch_geometry): one cell per structural class -- plane corners, tile ends, partial tiles,
the last thread's cell pair, planes 0, 1, n3-2, n3-1, the ends of interior z-chunks, workgroups past
the 256 threads of the partial reduction and of every arrival shard.  A class names a set of
candidate cells (any plane of a corner column, any row of a partial tile's first column, ...); the
first candidate that satisfies the two CPU conditions is taken; where none does, a candidate moved
by a cell inside the same workgroup (tile, z-chunk) is tried and the move printed, and a class still
without a cell fails.  The block sizes and the block-to-tile map are the library's: the cache
kernel's workgroups per plane and the kernels' own xcd_remap (pft_xcd_remap) are asked for.

Routes, and how each case knows it was taken:
  cache kernel              tile_geometry kind 0, pairs 0, arrival atomics (pft_slab_eps_route 0)
  fused stage 5, deferred   kind 2, pairs 0, pft_slab_eps_route 1
  fused stage 5, arrival    kind 2, pairs 0, pft_slab_eps_route 0 (PFT_INKERNEL_PUBLISH=0)
  pair kernel 4+5           stats.pairs 1, pft_slab_pair_geometry, route 1
  gated step                stats.gated_steps > 0
  three slabs (loopback)    every rank path 1 and the same record; route 0 (max over ranks on the host)
  self-exchange             rccl: route 0; ipc: route 1

The non-finite flag travels beside the maximum in words of its own, so test_nan_* send one NaN
through the routes above.  Over three slabs (loopback, with and without pairs) the slabs are 12
planes tall and the NaN sits in the first plane of rank 0, the middle of rank 1 or the last plane of
rank 2; the CPU oracle must confirm that the non-finite planes of an attempt stay inside that rank,
so the other ranks give up only if its flag reaches them.  Over the self-exchange transports
(first, inner and last plane) and on one slab there is one flag word: a boundary launch's flag
cannot be isolated there, since the interior planes next to it are non-finite too.  The gated
give-up accepts no step, so it shows the host's rows with gating on, not gate_decide's d_nan branch.
"""
import ctypes as C
import functools
import os
import uuid

import numpy as np
import pytest

import _multi
import _oracle as O
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

MULT = (0.25, 3.0, 7.0)
STEPS = 3


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


@functools.lru_cache(maxsize=None)
def _g20():
    meta, _ = O.load_case("g20")
    return O.params_from_meta(meta)


def _info(dims):
    """g20 with the grid `dims` and the cell of 40 x 20 x 7 at g20's domain (see the module docstring)"""
    _, info = _g20()
    n1, n2, n3 = dims
    return dict(info, n1=n1, n2=n2, n3=n3, L1=n1 * (info["L1"] / 40), L2=n2 * (info["L2"] / 20),
                L3=n3 * (info["L3"] / 7))


def probe_state(dims, target):
    Pm, _ = _g20()
    n1, n2, n3 = dims
    x = np.zeros((3, n3, n2, n1))
    x[0] = Pm[O.PARAM_NAMES.index("top_temp1")]
    x[1][target] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def cpu_probe(dims, target, mult=None, delta_local=False, steps=STEPS):
    """(the two CPU conditions hold, the unskipped oracle run)"""
    Pm, _ = _g20()
    info = _info(dims)
    x = probe_state(dims, target)
    kw = dict(delta_local=delta_local, chunk_mult=mult)
    full = O.solve_ex(info, Pm, 0, x, 0.0, 1.0, [1e9], max_steps_total=steps, **kw)[0]
    if not all(cell[1:] == target for _, cell in full[6][:STEPS]):
        return False, full
    skip = np.zeros(x.shape, dtype=np.uint8)
    skip[(slice(None),) + target] = 1
    one = O.solve_ex(info, Pm, 0, x, 0.0, 1.0, [1e9], max_steps_total=1, **kw)[0]
    cut = O.solve_ex(info, Pm, 0, x, 0.0, 1.0, [1e9], max_steps_total=1, skip=skip, **kw)[0]
    return one[1] != cut[1], full


MOVES = [(0, -1, 0), (0, 1, 0), (0, 0, -2), (0, 0, 2), (0, -2, 0), (0, 2, 0), (-1, 0, 0), (1, 0, 0), (0, -1, -2),
         (0, 1, 2), (0, 0, -1), (0, 0, 1)]


def pick(dims, classes, mult=None, delta_local=False, group=None):
    """{class: the first candidate cell (k, j, i) that satisfies the CPU conditions}.  Where no cell
    of the class does (next to a wall the maximum falls on the wall cell, or two mirror images tie),
    the candidates moved by a row, a plane or a cell pair are tried and the move is printed; a class
    still without a cell fails the test (never a vacuous case).  group: cell -> the workgroup (tile,
    chunk, block) that handles it; a moved cell must stay in the group of the cell it was moved
    from, so a class never silently tests another workgroup than it names.  The classes that name
    one thread's cell or a corner (no group passed, or the name says so) are never moved."""
    n1, n2, n3 = dims
    out = {}
    for name, cands in classes.items():
        cands = list(cands)[:16]
        kfixed = name.startswith(("plane", "chunk", "rank"))      # classes that name their plane
        exact = name.startswith(("corner", "wg0_", "wg1_", "plane_lastcell"))
        moved = []
        if not exact and (group is not None or kfixed):
            moved = [(k + dk, j + dj, i + di) for dk, dj, di in MOVES for k, j, i in cands[:4]
                     if 0 <= k + dk < n3 and 0 <= j + dj < n2 and 0 <= i + di < n1 and not (kfixed and dk)
                     and (group is None or group((k + dk, j + dj, i + di)) == group((k, j, i)))]
        for tgt in cands + [m for m in dict.fromkeys(moved) if m not in cands]:
            if cpu_probe(dims, tgt, mult, delta_local)[0]:
                out[name] = tgt
                if tgt not in cands:
                    print(f"moved: {dims} {name}: {cands[0]} -> {tgt}")
                break
        assert name in out, f"{dims}: no cell of class {name!r} carries the maximum alone ({cands})"
    return out


def tile_group(dims, tile, kz=None):
    """cell -> (z-chunk, tile row, tile column): the workgroup of a TX x TY tiling marching kz planes
    (kz None: the chunk is left out, any plane of the tile stands for the class)"""
    TX, TY = tile
    return lambda c: (c[0] // kz if kz else 0, c[1] // TY, c[2] // TX)


# ---- the device side -------------------------------------------------------------------------

def _geometry(sim):
    """what the slab reports after a solve: kind, tile in cells, stage-5 launch, pair tile, route"""
    L = P.lib()
    L.pft_slab_pair_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pft_slab_launch_geometry.argtypes = [C.c_void_p] + [C.c_int] + [C.POINTER(C.c_int)] * 3
    L.pft_slab_eps_route.argtypes = [C.c_void_p]
    slab = L.pft_solver_slab()
    kind, wx, ty = sim.tile_geometry()[5]
    nwg, kz, ntile, px, py = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    bnd = L.pft_slab_launch_geometry(slab, 5, C.byref(nwg), C.byref(kz), C.byref(ntile))
    assert bnd in (0, 1)        # 1: a split stage's boundary launch came last (nwg, kz are its own)
    L.pft_slab_pair_geometry(slab, C.byref(px), C.byref(py))
    return {"bnd_launch": bnd, "kind": kind, "tile": (2 * wx, ty), "nwg": nwg.value, "kz": kz.value, "ntile": ntile.value,
            "pair_tile": (px.value, py.value), "route": L.pft_slab_eps_route(slab)}


def gpu_run(dims, x0, tile=2, recompute=True, pair=0, gate=0, kz=None, publish=True, steps=STEPS, mult=None,
            delta_local=False, nprocs=1, rank=0, handle_nan=None, final=1e9):
    """one slab's solve of `steps` attempted steps from x0 (global interior); call per host thread"""
    Pm, _ = _g20()
    info = _info(dims)
    L = P.lib()
    L.pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    L.pft_solver_set_option(P.PFT_OPT_GATE, gate)
    if not publish:
        os.environ["PFT_INKERNEL_PUBLISH"] = "0"
    if handle_nan is not None:
        L.RK_MPI_SA_handle_NAN(handle_nan)
    sim = None
    try:
        sim = P.Simulation(dims[0], dims[1], dims[2], (info["L1"], info["L2"], info["L3"]), 0, Pm, nprocs=nprocs,
                           rank=rank, initial=x0, tau=1.0, tau_min=info["tau_min"], delta=info["delta"], tile=tile,
                           recompute=recompute, kz=kz, chunk_mult=mult,
                           delta_mode=P.DELTA_LOCAL if delta_local else P.DELTA_GLOBAL)
        rc = L.pft_solve_ex(final, C.byref(sim.system), steps, 0)
        st = sim.stats()
        out = {"rc": rc, "rec": (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total),
               "x": sim.interior(), "path": st.path, "pairs": st.pairs, "gated": st.gated_steps,
               "nan": L.RK_MPI_SA_check_NAN()}
        if st.path == 1:
            out.update(_geometry(sim))
        return out
    finally:
        if sim is not None:
            sim.close()
        if handle_nan is not None:
            L.RK_MPI_SA_handle_NAN(0)
        if not publish:
            del os.environ["PFT_INKERNEL_PUBLISH"]
        L.pft_solver_set_option(P.PFT_OPT_GATE, 0)
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)


def same_as_oracle(got, ref):
    assert got["rc"] == ref[4]
    assert got["rec"] == (ref[0].hex(), ref[1].hex(), ref[2], ref[3])
    assert np.array_equal(got["x"], ref[5])


def check_targets(dims, targets, claim, mult=None, delta_local=False, **route):
    """every target through one route: the CPU conditions, then the device equal to the oracle and
    on the claimed route"""
    for name, tgt in targets.items():
        ok, ref = cpu_probe(dims, tgt, mult, delta_local)
        assert ok, (name, tgt)
        got = gpu_run(dims, probe_state(dims, tgt), mult=mult, delta_local=delta_local, **route)
        try:
            same_as_oracle(got, ref)
        except AssertionError as e:
            raise AssertionError(f"target {name} {tgt}: {e}") from e
        for key, want in dict(claim, bnd_launch=0).items():
            assert got[key] == want, (name, key, got[key], want)


# ---- targets from the reported geometry ---------------------------------------------------------

def _planes(n3, first=()):
    """every plane, the given ones first, then from the middle outwards"""
    mid = sorted(range(n3), key=lambda k: abs(k - n3 // 2))
    return list(dict.fromkeys(list(first) + mid))


def _spread(n):
    """indices of an axis: the middle first, then outwards"""
    return sorted(range(n), key=lambda v: abs(v - n // 2))


def plane_classes(dims):
    """the four corners of the plane (in any plane) and planes 0, 1, n3-2, n3-1 (at any cell)"""
    n1, n2, n3 = dims
    c = {}
    for name, (j, i) in {"corner00": (0, 0), "corner0X": (0, n1 - 1), "cornerY0": (n2 - 1, 0),
                         "cornerYX": (n2 - 1, n1 - 1)}.items():
        c[name] = [(k, j, i) for k in _planes(n3, (0, n3 - 1))]
    for name, k in {"plane0": 0, "plane1": 1, "planeN-2": n3 - 2, "planeN-1": n3 - 1}.items():
        if 0 <= k < n3:
            c[name] = [(k, j, i) for j in _spread(n2)[:4] for i in _spread(n1)[:6]]
    return c


def tile_classes(dims, tile):
    """cells at the ends of a TX x TY-cell tiling of the plane: the last cell (both cells of its
    pair: the tile's last thread) of the last full tile, the first and last cell of a partial tile
    in x and in y"""
    n1, n2, n3 = dims
    TX, TY = tile
    fx, fy = n1 // TX, n2 // TY
    ks = _planes(n3)
    c = {}
    if fx and fy:
        j, i = fy * TY - 1, fx * TX - 1
        c["lastfull_odd"] = [(k, j, i) for k in ks]
        c["lastfull_even"] = [(k, j, i - 1) for k in ks]
        c["tile0_lastthread"] = [(k, TY - 1, TX - 1) for k in ks] + [(k, TY - 1, TX - 2) for k in ks]
    if n1 % TX:
        rows = _spread(n2)[:6]
        c["partialx_first"] = [(k, j, fx * TX) for k in ks[:4] for j in rows]
        c["partialx_last"] = [(k, j, n1 - 1) for k in ks[:4] for j in rows]
        # the last row of a tile that is partial in x (the tile row's end, or the plane's)
        inside = [i for i in _spread(n1) if i >= fx * TX][:6]
        c["partialx_lastrow"] = [(k, min(TY, n2) - 1, i) for k in ks[:3] for i in inside]
        c["partialx_lastrow_wall"] = [(k, n2 - 1, i) for k in ks[:3] for i in [n1 - 1] + inside]
    if n2 % TY:
        cols = _spread(n1)[:6]
        c["partialy_first"] = [(k, fy * TY, i) for k in ks[:4] for i in cols]
        c["partialy_last"] = [(k, n2 - 1, i) for k in ks[:4] for i in [0, n1 - 1] + cols]
    return c


def flat_classes(dims, ntile, block=256):
    """the cache kernel's workgroups hold `block` consecutive cells of the plane (merson_stage: one
    thread per cell): the last thread of the first workgroup, the first of the second, and the
    plane's last cell (the last active thread of a partial workgroup).  ntile: the workgroups per
    plane that the launch reports, which must be what `block` threads a workgroup give"""
    n1, n2, n3 = dims
    assert ntile == (n1 * n2 + block - 1) // block, (ntile, n1 * n2, block)
    ks = _planes(n3)
    c = {}
    if n1 * n2 > block:
        c["wg0_lastthread"] = [(k, (block - 1) // n1, (block - 1) % n1) for k in ks]
        c["wg1_firstthread"] = [(k, block // n1, block % n1) for k in ks]
    c["plane_lastcell"] = [(k, n2 - 1, n1 - 1) for k in ks]
    return c


def chunk_classes(dims, kz):
    """the first and last plane of an interior z-chunk of kz planes"""
    n1, n2, n3 = dims
    nch = (n3 + kz - 1) // kz
    assert nch >= 3, "no interior chunk"
    cells = [(j, i) for j in _spread(n2)[:4] for i in _spread(n1)[:6]]
    c = {}
    for ch in list(dict.fromkeys([1, nch - 2])):
        c[f"chunk{ch}_first"] = [(ch * kz, j, i) for j, i in cells]
        c[f"chunk{ch}_last"] = [(min(ch * kz + kz, n3) - 1, j, i) for j, i in cells]
    return c


def xcd_remap(b, n):
    """the launch's block index -> the linear (chunk, tile) index: the kernels' own xcd_remap,
    compiled for the host (pft_xcd_remap)"""
    return P.lib().pft_xcd_remap(b, n)


def block_classes(dims, tile, kz, nwg, ntile):
    """fused stage 5 (merson_fused: lin = xcd_remap(blockIdx), tile = lin % ntile, chunk =
    lin / ntile): a cell in the LAST workgroup, one in a workgroup past the 256 threads of the
    partial reduction's first pass, and one per residue of blockIdx % 8 (the arrival shards)"""
    n1, n2, n3 = dims
    TX, TY = tile
    ntx = (n1 + TX - 1) // TX
    assert ntile == ntx * ((n2 + TY - 1) // TY) and nwg == ntile * ((n3 + kz - 1) // kz)

    def cells(b):
        lin = xcd_remap(b, nwg)
        t, ch = lin % ntile, lin // ntile
        x0, y0 = (t % ntx) * TX, (t // ntx) * TY
        ks = range(ch * kz, min(ch * kz + kz, n3))
        return [(k, j, i) for k in ks for j in range(y0, min(y0 + TY, n2))[:3] for i in range(x0, min(x0 + TX, n1))[:4]]

    assert sorted(xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg))
    c = {"wg_last": cells(nwg - 1)}
    if nwg > 256:
        c["wg_ge256"] = [cell for b in range(256, min(nwg, 256 + 4)) for cell in cells(b)[:6]]
    for r in range(min(8, nwg)):
        bs = [b for b in range(nwg) if b % 8 == r]
        c[f"shard{r}"] = [cell for b in bs[-3:] for cell in cells(b)[:8]]
    return c


def _some(classes, keep):
    return {k: v for k, v in classes.items() if k in keep}


@functools.lru_cache(maxsize=None)
def geometry_of(dims, tile, recompute, pair, kz):
    """the geometry a route reports on this grid (one attempted step of a corner probe)"""
    x = probe_state(dims, (0, 0, 0))
    geo = gpu_run(dims, x, tile=tile, recompute=recompute, pair=pair, kz=kz, steps=1)
    assert geo["bnd_launch"] == 0       # one slab: nwg, kz and ntile are the whole launch's
    return geo


# ---- single slab --------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(66, 38, 21), (17, 9, 13)])
def test_cache_kernel(dims):
    geo = geometry_of(dims, 0, False, 0, None)
    assert geo["kind"] == 0 and geo["pairs"] == 0 and geo["path"] == 1
    classes = dict(plane_classes(dims), **flat_classes(dims, geo["ntile"]))
    check_targets(dims, pick(dims, classes), {"kind": 0, "pairs": 0, "path": 1, "route": 0},
                  tile=0, recompute=False)


@pytest.mark.parametrize("kz", [1, 3])
def test_cache_kernel_z_chunks(kz):
    dims = (17, 9, 13)
    check_targets(dims, pick(dims, chunk_classes(dims, kz)), {"kind": 0, "kz": kz, "route": 0},
                  tile=0, recompute=False, kz=kz)


@pytest.mark.parametrize("publish", [True, False], ids=["deferred", "arrival"])
@pytest.mark.parametrize("kz", [None, 1, 3])
@pytest.mark.parametrize("dims", [(66, 38, 21), (30, 30, 24)])
def test_fused_stage5(dims, kz, publish):
    """merson_fused stage 5 on 66 x 38 x 21 (the fitted tile spans the plane's width and leaves a
    partial tile in y) and 30 x 30 x 24 (a tile wider than the plane: partial in x): the workgroups'
    maxima as deferred partials reduced by the next stage 1, or (PFT_INKERNEL_PUBLISH=0) on the
    arrival shards"""
    geo = geometry_of(dims, 2, True, 0, kz)
    assert geo["kind"] == 2 and geo["pairs"] == 0
    assert dims[1] % geo["tile"][1] if dims == (66, 38, 21) else dims[0] % geo["tile"][0]
    classes = tile_classes(dims, geo["tile"])
    if kz is None:
        classes.update(plane_classes(dims))
    else:
        assert geo["kz"] == kz
        classes = dict(_some(classes, ("lastfull_odd", "partialx_last", "partialy_first")), **chunk_classes(dims, kz))
    classes.update(_some(block_classes(dims, geo["tile"], geo["kz"], geo["nwg"], geo["ntile"]), ("wg_last",)))
    group = tile_group(dims, geo["tile"], geo["kz"])
    check_targets(dims, pick(dims, classes, group=group), {"kind": 2, "pairs": 0, "path": 1, "route": 1 if publish else 0,
                                              "nwg": geo["nwg"]}, tile=2, pair=0, kz=kz, publish=publish)


@pytest.mark.parametrize("publish", [True, False], ids=["deferred", "arrival"])
def test_fused_stage5_many_workgroups(publish):
    """120 x 60 x 20 with one plane per workgroup: more than 256 workgroups, so the partial
    reduction's 256 threads stride (eps_part_load) and every arrival shard holds several"""
    dims, kz = (120, 60, 20), 1
    geo = geometry_of(dims, 2, True, 0, kz)
    assert geo["kind"] == 2 and geo["kz"] == 1 and geo["nwg"] > 256 and geo["nwg"] == geo["ntile"] * 20
    classes = block_classes(dims, geo["tile"], 1, geo["nwg"], geo["ntile"])
    assert "wg_ge256" in classes and all(f"shard{r}" in classes for r in range(8))
    classes.update(_some(plane_classes(dims), ("corner00", "cornerYX")))
    group = tile_group(dims, geo["tile"], 1)        # (chunk, tile) <-> block: xcd_remap is a bijection
    check_targets(dims, pick(dims, classes, group=group), {"kind": 2, "pairs": 0, "route": 1 if publish else 0,
                                                           "nwg": geo["nwg"]}, tile=2, pair=0, kz=kz, publish=publish)


@pytest.mark.parametrize("kz", [None, 2])
@pytest.mark.parametrize("dims", [(40, 20, 7), (120, 60, 7), (66, 38, 21), (66, 37, 6)])
def test_pair_kernel(dims, kz):
    """merson_pair 4+5: one 40 x 20 tile, 3 x 3 tiles, tiles partial in x, and (n2 = 37, which no
    tile height divides) partial in x and y"""
    geo = geometry_of(dims, 2, True, 2, kz)
    assert geo["pairs"] == 1 and geo["pair_tile"][0] > 0
    if dims == (66, 38, 21):
        assert dims[0] % geo["pair_tile"][0]
    if dims == (66, 37, 6):
        assert dims[0] % geo["pair_tile"][0] and dims[1] % geo["pair_tile"][1]
    if dims == (40, 20, 7):
        assert geo["pair_tile"] == (40, 20)
    if dims == (120, 60, 7):
        assert geo["ntile"] == 9
    classes = dict(plane_classes(dims), **tile_classes(dims, geo["pair_tile"]))
    if kz:
        assert geo["kz"] == kz
        classes.update(chunk_classes(dims, kz))
    group = tile_group(dims, geo["pair_tile"], geo["kz"])
    check_targets(dims, pick(dims, classes, group=group),
                  {"pairs": 1, "path": 1, "route": 1, "pair_tile": geo["pair_tile"]}, tile=2, pair=2, kz=kz)


def test_pair_kernel_arrival():
    dims = (66, 38, 21)
    geo = geometry_of(dims, 2, True, 2, None)
    classes = _some(dict(plane_classes(dims), **tile_classes(dims, geo["pair_tile"])),
                    ("cornerYX", "lastfull_odd", "partialx_first", "partialy_last", "plane1"))
    group = tile_group(dims, geo["pair_tile"], geo["kz"])
    check_targets(dims, pick(dims, classes, group=group), {"pairs": 1, "route": 0}, tile=2, pair=2, publish=False)


GATE_STEPS = 12


@pytest.mark.parametrize("delta_local", [False, True], ids=["global", "local"])
def test_gated_step(delta_local):
    """the device's own decision (gate_decide) on the error norm its speculative stage 1 reduced"""
    dims = (30, 30, 24)
    geo = geometry_of(dims, 2, True, 0, None)
    classes = _some(dict(plane_classes(dims), **tile_classes(dims, geo["tile"])),
                    ("corner00", "cornerYX", "plane1", "planeN-2", "lastfull_odd", "partialx_last", "partialy_first"))
    gated = 0
    for name, tgt in pick(dims, classes, None, delta_local, group=tile_group(dims, geo["tile"], geo["kz"])).items():
        ok, _ = cpu_probe(dims, tgt, None, delta_local)
        assert ok, (name, tgt)
        ref = cpu_probe(dims, tgt, None, delta_local, steps=GATE_STEPS)[1]
        got = gpu_run(dims, probe_state(dims, tgt), tile=2, pair=0, gate=1, steps=GATE_STEPS, delta_local=delta_local)
        print(name, tgt, "gated steps", got["gated"], "of", GATE_STEPS)
        same_as_oracle(got, ref)
        assert got["pairs"] == 0 and got["path"] == 1 and got["gated"] > 0, (name, got["gated"])
        gated += got["gated"]
    assert gated > 0


# ---- several slabs ------------------------------------------------------------------------------

def _slab_targets(dims, nprocs):
    """per rank: a cell in the slab's first plane, its last plane and (3 planes or more) an interior one"""
    n1, n2, n3 = dims
    cells = [(j, i) for j in _spread(n2)[:4] + [0, n2 - 1] for i in _spread(n1)[:4] + [0, n1 - 1]]
    c = {}
    for r in range(nprocs):
        m, f = O.decompose(n3, nprocs, r)
        c[f"rank{r}_first"] = [(f, j, i) for j, i in cells]
        c[f"rank{r}_last"] = [(f + m - 1, j, i) for j, i in cells]
        if m >= 3:
            c[f"rank{r}_inner"] = [(f + 1, j, i) for j, i in cells]
    return c


class _Run:
    """a rank of a loopback run: _multi.loopback_run builds it on the rank's thread, runs and closes it"""

    def __init__(self, dims, x0, kw):
        self.args, self.kw = (dims, x0), kw

    def go(self):
        return gpu_run(*self.args, **self.kw)

    def close(self):
        pass


def loopback_outs(dims, x0, nprocs=3, pair=0, **kw):
    """nprocs slabs of one GPU on host threads: every rank's gpu_run, each on the split-slab route
    (the maximum over ranks is taken on the host, so the arrival atomics)"""
    out = _multi.loopback_run(nprocs, lambda r: _Run(dims, x0, dict(kw, tile=2, pair=pair, nprocs=nprocs, rank=r)),
                              lambda run: run.go(), timeout=120)
    for o in out:
        assert o["path"] == 1 and o["pairs"] == (1 if pair else 0) and o["route"] == 0
    return out


def run_loopback(dims, x0, ref, nprocs=3, pair=0, **kw):
    """every rank's record and the joined state equal the (single-slab) oracle's"""
    out = loopback_outs(dims, x0, nprocs, pair, **kw)
    for o in out:
        assert o["rc"] == ref[4] and o["rec"] == (ref[0].hex(), ref[1].hex(), ref[2], ref[3]), o["rec"]
    assert np.array_equal(np.concatenate([o["x"] for o in out], axis=1), ref[5])


def run_self_exchange(transport, dims, x0, ref, pair=0, **kw):
    same_as_oracle(self_exchange_out(transport, dims, x0, pair, **kw), ref)


def self_exchange_out(transport, dims, x0, pair=0, **kw):
    """one rank exchanging with itself over RCCL or ipc (as test_pair_gpu.test_pair_self_exchange)"""
    L = P.lib()
    if transport == "rccl":
        uid = (C.c_char * 128)()
        assert L.pft_comm_get_unique_id(uid) == 0
        comm = C.c_void_p()
        assert L.pft_comm_init_rccl(C.byref(comm), 1, 0, uid, 0) == 0
        L.pft_comm_set_current(comm)
    else:
        comm = P.comm_init_ipc(1, 0, f"/pft_epsx_{os.getpid()}_{uuid.uuid4().hex[:12]}")
    try:
        assert L.pft_comm_set_self_exchange(comm, 1) == 0
        assert L.pft_comm_splits(comm) == 1
        got = gpu_run(dims, x0, tile=2, pair=pair, **kw)
    finally:
        L.pft_comm_set_current(None)
        P.comm_destroy(comm)
    assert got["path"] == 1 and got["pairs"] == (1 if pair else 0)
    # ipc: stage 5 publishes for itself (deferred partials); RCCL: the all-reduce reads the accumulator
    assert got["route"] == (1 if transport == "ipc" else 0), got["route"]
    return got


@pytest.mark.parametrize("pair", [0, 2], ids=["stages", "pairs"])
@pytest.mark.parametrize("dims", [(30, 30, 12), (18, 12, 8)])
def test_three_slabs_loopback(dims, pair):
    """three slabs of one GPU: the boundary launches add to the error norm, and the maximum of one
    rank must win on all (pft_comm_eps_publish / pft_comm_allreduce_eps)"""
    for name, tgt in pick(dims, _slab_targets(dims, 3)).items():
        ok, ref = cpu_probe(dims, tgt)
        assert ok, (name, tgt)
        try:
            run_loopback(dims, probe_state(dims, tgt), ref, pair=pair)
        except AssertionError as e:
            raise AssertionError(f"target {name} {tgt}: {e}") from e


@pytest.mark.parametrize("pair", [0, 2], ids=["stages", "pairs"])
@pytest.mark.parametrize("transport", ["rccl", "ipc"])
def test_self_exchange(transport, pair):
    """one rank exchanging with itself: the split launches (boundary planes first) of a slab between
    neighbours, the error norm through RCCL's all-reduce or the ipc host round"""
    dims = (30, 30, 12)
    n3 = dims[2]
    cells = [(j, i) for j in _spread(30)[:4] for i in _spread(30)[:4]]
    classes = {f"plane{k}": [(k, j, i) for j, i in cells] for k in (0, 1, n3 // 2, n3 - 2, n3 - 1)}
    for name, tgt in pick(dims, classes).items():
        ok, ref = cpu_probe(dims, tgt)
        assert ok, (name, tgt)
        try:
            run_self_exchange(transport, dims, probe_state(dims, tgt), ref, pair=pair)
        except AssertionError as e:
            raise AssertionError(f"target {name} {tgt}: {e}") from e


# ---- multipliers and delta mode on the device ---------------------------------------------------

FLAVOURS = {"cache": dict(tile=0, recompute=False), "fusedauto": dict(tile=2, pair=0),
            "pairs": dict(tile=2, pair=2), "gated": dict(tile=2, pair=0, gate=1)}


@pytest.mark.parametrize("name,flavour", [(n, f) for n in "abc" for f in FLAVOURS if (n, f) != ("b", "gated")])
def test_epsctl_reference_runs(name, flavour):
    """the reference's own runs with DELTA_LOCAL and per-variable multipliers (tests/golden/epsctl);
    the gated flavour takes the DELTA_LOCAL runs (a) and (c), which gate_decide restates"""
    meta, A = O.load_case("epsctl")
    Pm, info = O.params_from_meta(meta)
    run = meta["runs"][name]
    kw = dict(FLAVOURS[flavour])
    L = P.lib()
    L.pft_solver_set_option(P.PFT_OPT_PAIR, kw.pop("pair", 1))
    L.pft_solver_set_option(P.PFT_OPT_GATE, kw.pop("gate", 0))
    sim = None
    try:
        sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                           initial=A["ic"], tau=run["h0"], t0=run["t0"], tau_min=info["tau_min"], delta=info["delta"],
                           chunk_mult=run["mult"], delta_mode=P.DELTA_LOCAL if run["delta_local"] else P.DELTA_GLOBAL,
                           **kw)
        rc = sim.solve(meta["T"])
        st = sim.stats()
        got = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, rc)
        x = sim.interior()
        kind = sim.tile_geometry()[5][0]
    finally:
        if sim is not None:
            sim.close()
        L.pft_solver_set_option(P.PFT_OPT_GATE, 0)
        L.pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    ref = run["traj"][0]
    assert got == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
    assert np.array_equal(x, A[f"{name}_state0"])
    assert st.path == 1 and st.pairs == (1 if flavour == "pairs" else 0)
    assert kind == (0 if flavour == "cache" else 2)
    if flavour == "gated":
        assert st.gated_steps > 0


def test_epsctl_multipliers_within_a_variable_take_the_staged_path():
    """run (d): x1 on even planes, x2.5 on odd ones -- canonical_chunks() refuses, libpft's own
    device RHS runs under run_staged with flat_combine_kernel's per-chunk table"""
    meta, A = O.load_case("epsctl")
    Pm, info = O.params_from_meta(meta)
    run = meta["runs"]["d"]
    cm = np.ones((3, info["n3"], info["n2"]))
    cm[:, 1::2, :] = run["mult_odd_planes"]
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       initial=A["ic"], tau=run["h0"], t0=run["t0"], tau_min=info["tau_min"], delta=info["delta"],
                       chunk_mult=cm)
    try:
        rc = sim.solve(meta["T"])
        path = sim.stats().path
        got = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, rc)
        x = sim.interior()
    finally:
        sim.close()
    ref = run["traj"][0]
    assert path == 2
    assert got == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
    assert np.array_equal(x, A["d_state0"])


@pytest.mark.parametrize("name", ["a", "c"])
def test_epsctl_delta_local_on_the_staged_path(name):
    """the reference's DELTA_LOCAL runs (a) and (c) under run_staged -- an identity DDLBF_Rearrange
    keeps the solve off the fused path (hybrid2.c:726-729): the controller's local scaling, and the
    NEXTFINISH hand-over that ends the solve at T, on the host-staged loop"""
    meta, A = O.load_case("epsctl")
    Pm, info = O.params_from_meta(meta)
    run = meta["runs"][name]
    assert run["delta_local"]
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       initial=A["ic"], tau=run["h0"], t0=run["t0"], tau_min=info["tau_min"], delta=info["delta"],
                       chunk_mult=run["mult"], delta_mode=P.DELTA_LOCAL)

    @P.REARRANGE_FN
    def same(n):
        return n

    sim.system.DDLBF_Rearrange = C.cast(same, C.c_void_p).value
    try:
        rc = sim.solve(meta["T"])
        path = sim.stats().path
        got = (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, rc)
        x = sim.interior()
    finally:
        sim.close()
    ref = run["traj"][0]
    assert path == 2
    assert got == (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
    assert np.array_equal(x, A[f"{name}_state0"])


ROUTES = {
    "cache": ((17, 9, 13), dict(tile=0, recompute=False), {"kind": 0, "route": 0}),
    "fused_deferred": ((66, 38, 21), dict(tile=2, pair=0), {"kind": 2, "pairs": 0, "route": 1}),
    "fused_arrival": ((66, 38, 21), dict(tile=2, pair=0, publish=False), {"kind": 2, "pairs": 0, "route": 0}),
    "pair": ((66, 38, 21), dict(tile=2, pair=2), {"pairs": 1, "route": 1}),
    "gated": ((30, 30, 24), dict(tile=2, pair=0, gate=1), {"pairs": 0}),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_probe_with_multipliers_and_delta_local(route):
    """multipliers (0.25, 3, 7) reach em0/em1/em2 of the route's kernel and DELTA_LOCAL its decision"""
    dims, kw, claim = ROUTES[route]
    steps = GATE_STEPS if route == "gated" else STEPS
    tgt = pick(dims, _some(plane_classes(dims), ("cornerYX",)), MULT, True)["cornerYX"]
    ok, ref = cpu_probe(dims, tgt, MULT, True)
    assert ok
    plain = cpu_probe(dims, tgt)[1]
    assert (ref[0], ref[1]) != (plain[0], plain[1])          # the multipliers and the mode are seen
    if steps != STEPS:
        ref = cpu_probe(dims, tgt, MULT, True, steps=steps)[1]
    got = gpu_run(dims, probe_state(dims, tgt), mult=MULT, delta_local=True, steps=steps, **kw)
    same_as_oracle(got, ref)
    for key, want in claim.items():
        assert got[key] == want, (key, got[key], want)
    if route == "gated":
        assert got["gated"] > 0


@pytest.mark.parametrize("route", ["loopback", "loopback_pairs", "selfx_rccl", "selfx_ipc"])
def test_probe_with_multipliers_and_delta_local_between_slabs(route):
    dims = (30, 30, 12)
    tgt = pick(dims, {"rank1_last": _slab_targets(dims, 3)["rank1_last"]}, MULT, True)["rank1_last"]
    ok, ref = cpu_probe(dims, tgt, MULT, True)
    assert ok
    plain = cpu_probe(dims, tgt)[1]
    assert (ref[0], ref[1]) != (plain[0], plain[1])
    x0 = probe_state(dims, tgt)
    if route.startswith("loopback"):
        run_loopback(dims, x0, ref, pair=2 if route.endswith("pairs") else 0, mult=MULT, delta_local=True)
    else:
        run_self_exchange(route.split("_")[1], dims, x0, ref, mult=MULT, delta_local=True)


# ---- the non-finite flag: the same routes, separate words -----------------------------------------

NAN_T = 36.0


def _giveup_rows(t, h, T):
    """hybrid2.c:493-503, :626-646 with every attempt non-finite: h /= 10 until h/(T-t) < 1e-11"""
    attempts = 0
    while True:
        attempts += 1
        if h / (T - t) < 1e-11:
            return attempts
        h /= 10


SLAB_ROUTES = ["loopback", "loopback_pairs", "selfx_rccl", "selfx_ipc"]
SLAB_DIMS = (30, 30, 12)          # one rank exchanging with itself
LOOP_NAN_DIMS = (18, 12, 36)      # three slabs of 12 planes: taller than a NaN travels in an attempt


@functools.lru_cache(maxsize=None)
def nan_planes(dims, cell):
    """the planes that hold a non-finite value after the first accepted step of the oracle
    (handle_NAN(0)) from the probe state with a NaN in u at `cell`: the stages carry a NaN one plane
    further each, so these are the planes whose error values are non-finite in an attempt, at any h"""
    Pm, _ = _g20()
    x0 = probe_state(dims, (0, 0, 0))
    x0[0][cell] = np.nan
    for attempts in range(1, 9):
        ref = O.solve_ex(_info(dims), Pm, 0, x0, 0.0, 1.0, [1e9], max_steps_total=attempts)[0]
        if ref[2] == 1:
            return tuple(k for k in range(dims[2]) if not np.isfinite(ref[5][:, k]).all())
    raise AssertionError("the oracle accepted no step")


def _route_dims(route):
    if route in ROUTES:
        return ROUTES[route][0]
    return LOOP_NAN_DIMS if route.startswith("loopback") else SLAB_DIMS


def _nan_cells(route):
    """{name: the cell (k, j, i) that holds the NaN}.  One slab: the plane's far corner.  Three
    slabs: the first plane of rank 0, the middle of rank 1 and the last plane of rank 2, and the CPU
    oracle must confirm that the non-finite planes stay inside that rank: the other two ranks have
    finite error values only and give up only if that one rank's flag reaches them.  One rank
    exchanging with itself: the first, an inner and the last plane (a single flag word; the boundary
    launch's flag cannot be told from the interior's, whose planes next to it are non-finite too)"""
    n1, n2, n3 = dims = _route_dims(route)
    if route in ROUTES:
        return {"cornerYX": (n3 // 2, n2 - 1, n1 - 1)}
    j, i = n2 // 2, n1 // 2
    if not route.startswith("loopback"):
        return {"first": (0, j, i), "inner": (n3 // 2, j, i), "last": (n3 - 1, j, i)}
    cells = {}
    for r, name in enumerate(("rank0_first", "rank1_middle", "rank2_last")):
        m, f = O.decompose(n3, 3, r)
        cell = ((f, f + m // 2, f + m - 1)[r], j, i)
        bad = nan_planes(dims, cell)
        assert bad and cell[0] in bad and all(f <= k < f + m for k in bad), (name, cell, bad, (f, m))
        cells[name] = cell
    return cells


def _nan_run(route, x0, **kw):
    """(every rank's gpu_run, the joined state) on a route of ROUTES or SLAB_ROUTES, which each
    run asserts it took"""
    if route in ROUTES:
        dims, rkw, claim = ROUTES[route]
        got = gpu_run(dims, x0, **dict(rkw, **kw))
        for key, want in claim.items():
            assert got[key] == want, (key, got[key], want)
        return [got], got["x"]
    if route.startswith("loopback"):
        outs = loopback_outs(LOOP_NAN_DIMS, x0, pair=2 if route.endswith("pairs") else 0, **kw)
        return outs, np.concatenate([o["x"] for o in outs], axis=1)
    got = self_exchange_out(route.split("_")[1], SLAB_DIMS, x0, **kw)
    return [got], got["x"]


@pytest.mark.parametrize("route", list(ROUTES) + SLAB_ROUTES)
def test_nan_flag_gives_up(route):
    """RK_MPI_SA_handle_NAN(1) and one NaN in u: every attempt is non-finite, so every rank divides h
    by 10 until it gives up with -4 and leaves the state alone.  A route that lost the flag would
    accept a step (the NaN never wins the maximum) and return 0.  Over three slabs only one rank has
    non-finite error values (_nan_cells), so a maximum over ranks that lost that rank's flag would
    let the other two go on.  Inside one slab (the self-exchange) a boundary launch's flag cannot
    be isolated: the interior planes next to it are non-finite in the same attempt.

    The gated flavour: gate_decide's d_nan branch makes the device skip every attempt, as the host
    does; no step is accepted, so gated_steps stays 0 and the host would discard a pre-enqueued step
    whatever the device decided -- the case pins the host's rows and the untouched state with
    gating on, not the device's branch (test_nan_never_wins_the_maximum[gated] has the flag raised
    beside kept gated steps)."""
    dims = _route_dims(route)
    for name, cell in _nan_cells(route).items():
        x0 = probe_state(dims, (0, 0, 0))
        x0[0][cell] = np.nan
        outs, x = _nan_run(route, x0, handle_nan=1, steps=0, final=NAN_T)
        for o in outs:
            assert o["rc"] == -4 and o["nan"] == 1, (name, o["rc"], o["nan"])
            assert o["rec"] == (0.0.hex(), 1.0.hex(), 0, _giveup_rows(0.0, 1.0, NAN_T)), (name, o["rec"])
            assert o["gated"] == 0
        assert np.array_equal(x, x0, equal_nan=True), name


@pytest.mark.parametrize("route", list(ROUTES) + SLAB_ROUTES)
def test_nan_never_wins_the_maximum(route):
    """RK_MPI_SA_handle_NAN(0): e > eps is false for a NaN (hybrid2.c:522), the finite cells decide,
    on every rank alike; the gated flavour must keep gated steps with the flag raised (d_nan 0)"""
    dims = _route_dims(route)
    steps = GATE_STEPS if route == "gated" else STEPS
    Pm, _ = _g20()
    for name, cell in _nan_cells(route).items():
        x0 = probe_state(dims, (0, 0, 0))
        x0[0][cell] = np.nan
        ref = O.solve_ex(_info(dims), Pm, 0, x0, 0.0, 1.0, [1e9], max_steps_total=steps)[0]
        assert ref[6][0][0] > 0.0 and np.isfinite(ref[6][0][0])
        outs, x = _nan_run(route, x0, handle_nan=0, steps=steps)
        for o in outs:
            assert o["rc"] == ref[4] and o["rec"] == (ref[0].hex(), ref[1].hex(), ref[2], ref[3]), (name, o["rec"])
            assert o["nan"] == 0
            if route == "gated":
                print(name, cell, "gated steps", o["gated"], "of", steps)
                assert o["gated"] > 0
        assert np.array_equal(x, ref[5], equal_nan=True), name
