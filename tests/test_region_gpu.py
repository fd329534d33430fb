"""f11 on the GPU: region_kernel (pft_slab_export_region_be, pft_slab_region_export) against the host
twin and numpy, word for word, on every selection of tests/_region.py -- also with the workgroups
capped so that the grid-stride loop iterates; Simulation.region against interior(); region files from
the resident state against save_snapshot(region=) of the downloaded state byte for byte, synchronous
and in the background; one region file from three loopback slabs and from two ipc processes; and
run_series with named regions."""
import ctypes as C
import filecmp
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import _diag as D
import _multi as M
import _oracle as O
import _region as R
import _snap as S
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
X, XN = P.PFT_BUF_X, P.PFT_BUF_XN
KEEP = P.PFT_SOLVE_KEEP_DEVICE
ALL = slice(None)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


# ---- 1. slab level ---------------------------------------------------------------------------

# the shapes of the f7 tests: 7x5x3 odd rows, below one wave; 64x8x2; 33x31x9 odd, several
# workgroups; 50x50x4
GRIDS = [(7, 5, 3), (64, 8, 2), (33, 31, 9), (50, 50, 4)]


def check_slab(n1, n2, n3):
    """every selection from X and from XN (the other buffer holds other words), ghost planes
    poisoned: through device memory at a 16-byte and at an 8-byte boundary and through the pinned
    buffer by both host links; each equals the host twin and numpy.  Returns the number of images
    compared."""
    g = D.grid(n1, n2, n3)
    slab = R.Slab(n1, n2, n3)
    done = 0
    try:
        for which, other, seed in ((X, XN, 81), (XN, X, 82)):
            a, b = S.random_words(n1, n2, n3, seed), S.random_words(n1, n2, n3, seed + 10)
            w = D.padded(a)
            slab.upload(which, w)
            slab.upload(other, D.padded(b))
            for name, sel in R.selections(n1, n2, n3):
                r = P.region(*sel, g)
                loc = R.local_region(g, r)
                want = R.be_words(S.np_image(a[(ALL,) + R.as_index(sel)]))
                assert np.array_equal(R.be_words(R.host_image(g, r, w)), want), name
                for how, got in (("dev16", slab.region_device(which, loc)), ("dev8", slab.region_device(which, loc, offset=8)),
                                 ("direct", slab.region_pinned(which, loc, 0)), ("staged", slab.region_pinned(which, loc, 1))):
                    assert np.array_equal(R.be_words(got), want), (name, how, which)
                    done += 1
            # the f7 image is untouched by all this
            assert slab.export_device(other) == S.np_image(b)
    finally:
        slab.close()
    return done


@pytest.mark.parametrize("n1,n2,n3", GRIDS)
def test_slab_region_image_equals_host_twin_and_numpy(n1, n2, n3):
    assert check_slab(n1, n2, n3) == 2 * 4 * len(R.selections(n1, n2, n3))


@pytest.mark.parametrize("wgs", [1, 3])
def test_grid_stride_loop_iterates(wgs):
    """33x31x9 in a fresh process with PFT_REGION_WGS=1 (and 3): 256 (768) lanes walk images of up
    to 9 207 words per field, a step that is no multiple of any row"""
    env = dict(os.environ, PFT_REGION_WGS=str(wgs))
    p = subprocess.run([sys.executable, os.path.join(HERE, "_region_wgs_worker.py"), "33", "31", "9"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-3000:]
    assert out.strip().splitlines()[-1] == "ok %d" % (2 * 4 * len(R.selections(33, 31, 9)))


def test_slab_entries_refuse_what_leaves_the_interior():
    """a region past the slab's interior is refused before any launch; a share of no planes moves
    nothing and succeeds"""
    slab = R.Slab(7, 5, 3)
    try:
        L, dev, img = slab.L, C.c_void_p(), C.c_void_p()
        assert L.pft_dev_alloc(C.byref(dev), 4096) == 0
        for t in (((0, 0, 0), (8, 1, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 4), (1, 1, 1)), ((0, 3, 0), (1, 2, 1), (1, 2, 1)),
                  ((-1, 0, 0), (1, 1, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1), (0, 1, 1)), ((0, 0, 0), (0, 1, 1), (1, 1, 1)),
                  ((0, 0, 3), (1, 1, 1), (1, 1, 1)), ((0, 0, 1), (1, 1, 2), (1, 1, 2))):
            r = P.pft_region(*t)
            assert L.pft_slab_export_region_be(slab.s, X, C.byref(r), dev) == -2, t
            assert L.pft_slab_region_export(slab.s, X, C.byref(r), 0, C.byref(img)) == -2, t
        ok = P.pft_region((0, 0, 0), (7, 5, 3), (1, 1, 1))
        assert L.pft_slab_export_region_be(slab.s, X, C.byref(ok), C.c_void_p(dev.value + 4)) == -2
        assert L.pft_slab_export_region_be(slab.s, 99, C.byref(ok), dev) == -2
        none = P.pft_region((1, 1, 0), (3, 2, 0), (2, 2, 5))
        assert L.pft_slab_region_image_bytes(C.byref(none)) == 0
        assert L.pft_slab_export_region_be(slab.s, X, C.byref(none), dev) == 0
        assert L.pft_slab_region_export(slab.s, X, C.byref(none), 1, C.byref(img)) == 0
        L.pft_dev_free(dev)
    finally:
        slab.close()


# ---- 2. solver level -------------------------------------------------------------------------

def _g20(mode=0, **kw):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    kw.setdefault("tau", 1.0)
    if "icond_file" not in kw:
        kw.setdefault("initial", A[f"traj_m{mode}_ic"])
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        tau_min=info["tau_min"], delta=info["delta"], **kw)


def _info(sim, final, snapshot=1, total=4, comment="f11"):
    return P.snapshot_info(sim.t, sim.h, final, sim.system.delta, sim.grid.calc_mode, snapshot=snapshot,
                           total_snapshots=total, comment=comment)


def test_no_resident_state_refuses_and_creates_nothing(tmp_path):
    """a host IC and no solve yet: -3, RuntimeError from the Python entries, no file; a bad region is
    -2 once a state is resident, and creates nothing either"""
    sim = _g20()
    try:
        path = str(tmp_path / "early.ncd")
        inf = _info(sim, 360.0)
        r = P.region(ALL, 5, ALL, sim.grid)
        L = sim.lib
        assert L.pft_solver_snapshot_region_write(os.fsencode(path), P._dp(sim.params), C.byref(inf), C.byref(r), 0) == -3
        assert L.pft_solver_region(C.byref(r), P._dp(np.zeros(3 * 20 * 10))) == -3
        with pytest.raises(RuntimeError, match="resident"):
            sim.snapshot_device(path, inf, region=(ALL, 5, ALL))
        with pytest.raises(RuntimeError, match="resident"):
            sim.region((ALL, 5, ALL))
        assert not os.path.exists(path)
        sim.solve_ex(36.0, 0, KEEP)
        bad = P.pft_region((0, 0, 0), (10, 10, 21), (1, 1, 1))
        assert L.pft_solver_snapshot_region_write(os.fsencode(path), P._dp(sim.params), C.byref(inf), C.byref(bad), 0) == -2
        assert L.pft_solver_region(C.byref(bad), P._dp(np.zeros(3 * 21 * 100))) == -2
        assert not os.path.exists(path)
    finally:
        sim.close()


def test_simulation_region_equals_interior():
    """g20 after the solve to 36 s: Simulation.region(sel) from the resident state equals
    interior()[:, sel] of the downloaded one, and where="host" the same"""
    _, A = O.load_case("g20")
    sim = _g20()
    try:
        sim.solve_ex(36.0, 0, KEEP)
        got = {name: sim.region(sel) for name, sel in R.selections(10, 10, 20)}
        sim.download()
        a = sim.interior()
        assert np.array_equal(a, A["traj_m0_state0"])
        for name, sel in R.selections(10, 10, 20):
            want = a[(ALL,) + R.as_index(sel)]
            assert got[name].shape == want.shape and got[name].dtype == np.float64, name
            assert np.array_equal(S.words(got[name]), S.words(want)), name
            assert np.array_equal(S.words(sim.region(sel, where="host")), S.words(want)), name
    finally:
        sim.close()


def test_device_region_file_equals_host_file(tmp_path):
    """region files from the resident state are byte for byte what save_snapshot(region=) writes from
    the downloaded state, as CDF-1 and with CDF-2 forced, by both host links"""
    sim = _g20()
    pairs = []
    try:
        sim.solve_ex(36.0, 0, KEEP)
        inf = _info(sim, 360.0)
        for name, sel in R.selections(10, 10, 20):
            for version, link in ((0, None), (2, "direct"), (1, "staged")):
                dev = str(tmp_path / f"dev.{name}.{version}.ncd")
                sim.snapshot_device(dev, inf, region=sel, version=version, link=link)
                pairs.append((dev, name, sel, version))
        sim.download()
        for dev, name, sel, version in pairs:
            host = str(tmp_path / f"host.{name}.{version}.ncd")
            P.save_snapshot(sim, host, inf, region=sel, version=version)
            assert filecmp.cmp(dev, host, shallow=False), (name, version)
            assert open(dev, "rb").read(4) == (b"CDF\x02" if version == 2 else b"CDF\x01")
        # and the variables are the selection of the state
        a = sim.interior()
        for dev, name, sel, version in pairs[::3]:
            r = P.region(*sel, sim.grid)
            rg = R.ranges(dev, sim.grid, r)
            back = C.create_string_buffer(3 * rg.bytes)
            assert sim.lib.pft_snapshot_read_image(os.fsencode(dev), C.byref(rg), back) == 0
            assert np.array_equal(R.be_words(back.raw), R.be_words(S.np_image(a[(ALL,) + R.as_index(sel)]))), name
    finally:
        sim.close()


def test_async_region_snapshot_is_a_snapshot_not_a_view(tmp_path):
    """snapshot_device(region=, wait=False) at 36 s and a solve to 360 s at once: after
    snapshot_wait() the files hold the state of 36 s -- two regions through the one pinned buffer"""
    sim = _g20()
    try:
        sim.solve_ex(36.0, 0, KEEP)
        inf = _info(sim, 360.0)
        sim.download()
        sels = {"xz": (ALL, 5, ALL), "half": (slice(0, None, 2), slice(1, None, 2), slice(0, None, 2))}
        for name, sel in sels.items():
            P.save_snapshot(sim, str(tmp_path / f"host.{name}.ncd"), inf, region=sel)
        for name, sel in sels.items():
            sim.snapshot_device(str(tmp_path / f"dev.{name}.ncd"), inf, region=sel, wait=False)
        sim.solve_ex(360.0, 0, KEEP | P.PFT_SOLVE_REUSE_DEVICE)
        sim.snapshot_wait()
        assert sim.t == 360.0
        for name in sels:
            assert filecmp.cmp(tmp_path / f"dev.{name}.ncd", tmp_path / f"host.{name}.ncd", shallow=False), name
    finally:
        sim.close()


# ---- 3. decomposition ------------------------------------------------------------------------

def test_loopback_slabs_write_one_region_file(tmp_path):
    """7x5x7 on 3 loopback slabs (3, 2, 2 planes) with the four k selections -- one plane per rank,
    rank 0 only, ranks 0 and 2, rank 1 only -- and a strided j and i: the shared file's variables are
    the gathered interior's selection, and the ranks' Simulation.region shares tile it"""
    a = D.random_state(7, 5, 7, 91)
    a[2] = np.abs(a[2])
    Pm = O.params_from_meta(O.load_case("g20")[0])[0]
    first = str(tmp_path / "first.ncd")
    inf = P.snapshot_info(36.0, 0.5, 72.0, 1e-3, 0, snapshot=3, total_snapshots=9, comment="slabs")
    g = D.grid(7, 5, 7)
    g.L1, g.L2, g.L3 = 0.03, 0.03, 0.06
    S.write_host(first, g, Pm, inf, D.padded(a, poison=False))
    sels = [(ks, slice(1, None, 2), slice(0, None, 3)) for ks in R.K_SELECTIONS]

    def make(r):
        return P.Simulation(7, 5, 7, (0.03, 0.03, 0.06), 0, Pm, nprocs=3, rank=r, icond_file=first)

    def run(sim):
        shares = []
        for n, sel in enumerate(sels):
            sim.snapshot_device(str(tmp_path / f"region.{n}.ncd"), inf, region=sel, wait=False)
            shares.append((sim.region_share(sel)[1], sim.region(sel)))
        sim.snapshot_wait()
        return shares

    out = M.loopback_run(3, make, run)
    for n, sel in enumerate(sels):
        want = a[(ALL,) + R.as_index(sel)]
        assert [o[n][0] for o in out] == R.K_OWNERS[n]
        assert np.array_equal(S.words(np.concatenate([o[n][1] for o in out], axis=1)), S.words(want))
        path = str(tmp_path / f"region.{n}.ncd")
        r = P.region(*sel, g)
        rg = R.ranges(path, g, r)
        back = C.create_string_buffer(3 * rg.bytes)
        assert P.lib().pft_snapshot_read_image(os.fsencode(path), C.byref(rg), back) == 0
        assert np.array_equal(R.be_words(back.raw), R.be_words(S.np_image(want))), n
        # byte for byte the host path's file of the whole state
        host = str(tmp_path / f"host.{n}.ncd")
        assert P.lib().pft_snapshot_write_region(os.fsencode(host), C.byref(g), C.byref(r), P._dp(Pm), C.byref(inf),
                                                 P._dp(D.padded(a)), 0) == 0
        assert filecmp.cmp(path, host, shallow=False), n


def test_two_ipc_processes_write_one_region_file(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_region_worker.py) read the golden state at 36 s,
    solve to 360 s and write region datasets from their resident slabs of 10 planes: a strided
    selection across the slab boundary and one that rank 1 alone owns (rank 0 writes its header);
    byte for byte the single slab's files"""
    meta, A = O.load_case("g20")
    ref0 = meta["traj_m0"][0]
    t, h = float.fromhex(ref0[0]), float.fromhex(ref0[1])
    start = str(tmp_path / "start.ncd")
    w = _g20(initial=A["traj_m0_state0"], init_solver=False)
    P.save_snapshot(w, start, P.snapshot_info(t, h, 360.0, w.system.delta, 0, snapshot=1, total_snapshots=4))
    w.close()
    regions = {"across": [[1, 20, 3], [0, 10, 2], [1, 10, 1]], "upper": [[15, 18, 1], [3, 4, 1], [0, 10, 3]]}
    one = _g20(icond_file=start, t0=t, tau=h)
    try:
        one.solve_ex(360.0, 0, KEEP | P.PFT_SOLVE_REUSE_DEVICE)
        inf = P.snapshot_info(one.t, one.h, 360.0, one.system.delta, 0, snapshot=2, total_snapshots=4, comment="ipc")
        whole = {}
        for name, triples in regions.items():
            sel = tuple(slice(*v) for v in triples)
            one.snapshot_device(str(tmp_path / f"single.{name}.ncd"), inf, region=sel)
            whole[name] = one.region(sel)
        one.download()
        assert np.array_equal(one.interior(), A["traj_m0_state1"])
    finally:
        one.close()
    spec = {"nranks": 2, "shm": f"/pft_region_{os.getpid()}_{uuid.uuid4().hex[:12]}", "icond_file": start, "t0": t,
            "tau": h, "T": 360.0, "regions": regions, "out": str(tmp_path / "two"), "res": str(tmp_path / "rank")}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_region_worker.py"), str(path), str(r)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
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
    res = [json.load(open(f"{spec['res']}.{r}.json")) for r in range(2)]
    assert [res[r]["regions"]["across"]["share"] for r in range(2)] == [[0, 3, 1], [3, 4, 0]]
    assert [res[r]["regions"]["upper"]["share"][1] for r in range(2)] == [0, 3]
    for name in regions:
        assert filecmp.cmp(f"{spec['out']}.{name}.ncd", tmp_path / f"single.{name}.ncd", shallow=False), name
        parts = [np.frombuffer(bytes.fromhex(res[r]["regions"][name]["words"]), np.uint64).reshape(res[r]["regions"][name]["shape"])
                 for r in range(2)]
        assert np.array_equal(np.concatenate(parts, axis=1), S.words(whole[name])), name


# ---- 4. the series ---------------------------------------------------------------------------

def test_run_series_writes_named_regions(tmp_path):
    """g20 to 36 s in 5 snapshots with two named regions and region_every=2, files from the resident
    state in the background: region files exist at snapshots 0, 2 and 4 only; each variable is that
    selection of the full dataset of the same run; the rows are those of a run without regions=;
    with snapshot_full=False on the host route the same region files appear and no full one"""
    regions = {"xz": (ALL, 5, ALL), "front": (slice(12, 20), slice(0, None, 3), slice(1, None, 2))}
    runs = {}
    for tag, kw in (("a", dict(snapshot_where="device", snapshot_async=True, regions=regions, region_every=2)),
                    ("b", dict(snapshot_where="host", regions=regions, region_every=2, snapshot_full=False)),
                    ("c", dict(snapshot_where="device", snapshot_async=True))):
        sim = _g20()
        try:
            (tmp_path / tag).mkdir()
            runs[tag] = sim.run_series(36.0, 5, snapshot_path=str(tmp_path / tag / "image"), comment="f11", **kw)
            grid = sim.grid
        finally:
            sim.close()
    assert [r["snapshot"] for r in runs["a"]] == list(range(5)) and runs["a"][-1]["t"] == 36.0
    assert runs["a"] == runs["c"] and runs["b"] == runs["c"]
    for s in range(5):
        full = tmp_path / "a" / ("image.%03d.ncd" % s)
        assert full.exists() and not (tmp_path / "b" / full.name).exists()
        assert filecmp.cmp(full, tmp_path / "c" / full.name, shallow=False)
        state = np.frombuffer(S.file_image(str(full), grid), ">u8").reshape(3, 20, 10, 10)
        for name, sel in regions.items():
            f = tmp_path / "a" / ("image.%s.%03d.ncd" % (name, s))
            assert f.exists() == (s % 2 == 0), (name, s)
            assert (tmp_path / "b" / f.name).exists() == (s % 2 == 0), (name, s)
            if s % 2:
                continue
            assert filecmp.cmp(f, tmp_path / "b" / f.name, shallow=False), (name, s)
            r = P.region(*sel, grid)
            rg = R.ranges(str(f), grid, r)
            back = C.create_string_buffer(3 * rg.bytes)
            assert P.lib().pft_snapshot_read_image(os.fsencode(str(f)), C.byref(rg), back) == 0
            want = np.ascontiguousarray(state[(ALL,) + R.as_index(sel)])
            assert np.array_equal(R.be_words(back.raw), want.reshape(-1)), (name, s)
            info = P.read_snapshot_info(str(f))[3]
            assert (info.snapshot, info.total_snapshots, info.t) == (s, 5, runs["a"][s]["t"])
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == ["image.%03d.ncd" % s for s in range(5)]
