"""f5 on the GPU: the diagnostics kernel (pft_slab_diag) against pft_diag_host and numpy field for
field -- counts and doubles by == -- on shapes that take every path of the kernel (an odd plane
smaller than a wave, one plane, several workgroups per plane, several planes per workgroup, more
planes than the LDS window), with single cells swept over the plane boundaries and poisoned ghost
planes; pft_solver_diag / Simulation.diagnostics / run_series on one slab, on loopback slabs, in two
ipc processes and from a Service_Callback."""
import ctypes as C
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
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


class SlabDesc(C.Structure):
    """include/pft_hip.h pft_slab_desc"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("n3", C.c_int), ("has_below", C.c_int),
                ("has_above", C.c_int), ("calc_mode", C.c_int), ("gl_static", C.c_int),
                ("eps_mult", C.c_double * 3)]


class Slab:
    """a bare pft_slab (no model, no solver): the diagnostics read the buffers only"""

    def __init__(self, n1, n2, n3):
        L = P.lib()
        L.pft_slab_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(SlabDesc), C.c_void_p]
        L.pft_slab_upload_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.pft_slab_destroy.argtypes = [C.c_void_p]
        self.L, self.n3 = L, n3
        d = SlabDesc(n1, n2, n3, 0, 0, 0, 0, (C.c_double * 3)(1.0, 1.0, 1.0))
        consts = (C.c_double * 64)(*([1.0] * 64))     # pft_consts: doubles only, unused here
        self.s = C.c_void_p()
        rc = L.pft_slab_create(C.byref(self.s), C.byref(d), consts)
        assert rc == 0, (rc, L.pft_hip_last_error())

    def upload(self, which, w):
        assert self.L.pft_slab_upload_host(self.s, which, P._dp(w)) == 0

    def diag(self, which, opts=None):
        d = P.pft_diag()
        planes = (C.c_longlong * self.n3)()
        o = None if opts is None else C.byref(P.pft_diag_opts(*opts))
        rc = self.L.pft_slab_diag(self.s, which, o, C.byref(d), planes)
        assert rc == 0, (rc, self.L.pft_hip_last_error())
        return D.rec_of(d), np.array(planes[:], dtype=np.int64)

    def close(self):
        self.L.pft_slab_destroy(self.s)


PFT_BUF_X, PFT_BUF_XN = 0, 1


def _check_state(slab, a, opts=None, which=PFT_BUF_X):
    """upload a (ghosts poisoned), then device == host twin == numpy"""
    n3, n2, n1 = a.shape[1:]
    w = D.padded(a)
    slab.upload(which, w)
    got, planes = slab.diag(which, opts)
    host, host_planes = D.host_diag(D.grid(n1, n2, n3), w, opts)
    want, want_planes = D.np_diag(a, *(opts or (0.5, 0.5)))
    D.assert_same(got, host, "device against pft_diag_host")
    D.assert_same(got, want, "device against numpy")
    assert np.array_equal(planes, host_planes) and np.array_equal(planes, want_planes)
    assert planes.sum() == got["ice"]
    return got, planes


def _special(a, seed):
    """NaN, +-Inf and signed zeros sprinkled into a copy of a"""
    a = a.copy()
    r = np.random.default_rng(seed)
    flat = a.reshape(3, -1)
    n = flat.shape[1]
    for q in range(3):
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            flat[q, r.integers(0, n, size=max(1, n // 40))] = v
    return a


# (n1, n2, n3, PFT_DIAG_WGS); a workgroup takes 2048 elements per iteration, a wave 512 of them.
# 7x5x3 an odd plane smaller than a wave, an odd run (a lone last element); 1x1x2 the smallest grid
# pft_grid_init accepts, 1x1x1 and 3x2x1 one plane (slab level only); 10x10x20 one workgroup, 18x12x30
# four; 50x50x100 123 workgroups, each inside one plane or across a plane boundary; 13x11x40 capped at
# 2 workgroups (and uncapped: 3): 20 planes per workgroup, the plane (143) no divisor of anything;
# 3x1x200 in one workgroup: 200 planes, past the 64-plane LDS window, and 3x1x2000 in three
SHAPES = [(7, 5, 3, 0), (1, 1, 2, 0), (1, 1, 1, 0), (3, 2, 1, 0), (10, 10, 20, 0), (18, 12, 30, 0),
          (50, 50, 100, 0), (13, 11, 40, 2), (13, 11, 40, 0), (13, 11, 9, 0), (3, 1, 200, 0), (3, 1, 2000, 0)]


@pytest.mark.parametrize("n1,n2,n3,wgs", SHAPES)
def test_slab_diag_equals_host_and_numpy(n1, n2, n3, wgs, monkeypatch):
    if wgs:
        monkeypatch.setenv("PFT_DIAG_WGS", str(wgs))
    slab = Slab(n1, n2, n3)
    try:
        a = D.random_state(n1, n2, n3, 11)
        got, _ = _check_state(slab, a)
        assert got["cells"] == n1 * n2 * n3
        _check_state(slab, a, opts=(0.7, 0.25))
        _check_state(slab, _special(a, 12))
        _check_state(slab, np.full_like(a, np.nan))
        z = np.zeros_like(a)
        z[2] = 1.0
        got, planes = _check_state(slab, z)         # no ice, no pore
        assert (got["ice"], got["pore"], got["ice_u_maxabs"]) == (0, 0, 0.0) and not planes.any()
    finally:
        slab.close()


def test_slab_diag_golden_and_ic():
    """the golden g20 states and the ragged fixture's; the IC at 50x50x100: 8 720 ice cells"""
    _, A = O.load_case("g20")
    slab = Slab(10, 10, 20)
    try:
        for key, ice in (("traj_m0_state0", 56), ("traj_m0_state2", 96), ("traj_m1_state2", 68), ("traj_m2_ic", 0)):
            got, planes = _check_state(slab, A[key])
            assert got["ice"] == ice
        got, planes = _check_state(slab, A["traj_m0_state0"])
        assert got["ice_u_maxabs"] == 275.68668582453085 and (planes[17], planes[18]) == (24, 32)
    finally:
        slab.close()
    slab = Slab(18, 12, 30)
    try:
        _check_state(slab, O.load_case("ragged")[1]["state"])
    finally:
        slab.close()
    base, Pm, info = M.full_size_case(100, 0)
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       beads=O.beads(), init_solver=False)
    a = sim.interior()
    sim.close()
    slab = Slab(50, 50, 100)
    try:
        got, _ = _check_state(slab, a)
        assert (got["ice"], got["pore"]) == (8720, 105796)
    finally:
        slab.close()


@pytest.mark.parametrize("n1,n2,n3", [(7, 5, 3), (10, 10, 20)])
def test_position_sweep(n1, n2, n3):
    """a single extreme u, or a single ice cell, at the first cell, the last cell, the last cell
    of a plane and the first cell of the next one; the device ghost planes hold poison"""
    plane = n1 * n2
    cells = [0, n3 * plane - 1, plane - 1, plane, (n3 - 1) * plane - 1, (n3 - 1) * plane]
    base = np.zeros((3, n3, n2, n1))
    base[0] = 1.0 + np.arange(n3 * plane).reshape(n3, n2, n1) / (n3 * plane)     # 1 <= u < 2
    base[2] = 1.0
    slab = Slab(n1, n2, n3)
    try:
        for c in cells:
            k = c // plane
            a = base.copy()
            a[0].reshape(-1)[c] = 1e6
            got, _ = _check_state(slab, a)
            assert got["u_max"] == 1e6 and got["ice"] == 0
            a = base.copy()
            a[0].reshape(-1)[c] = -1e6
            got, _ = _check_state(slab, a)
            assert got["u_min"] == -1e6
            a = base.copy()
            a[1].reshape(-1)[c] = 1.0
            got, planes = _check_state(slab, a)
            assert got["ice"] == 1 and planes[k] == 1 and got["ice_u_maxabs"] == base[0].reshape(-1)[c]
            assert got["p_max"] == 1.0
    finally:
        slab.close()


def test_no_accumulator_carries_over():
    """X, then XN holding another state: each call returns its buffer's own numbers"""
    slab = Slab(10, 10, 20)
    try:
        a, b = D.random_state(10, 10, 20, 21), D.random_state(10, 10, 20, 22)
        b[0] *= 0.5          # smaller maxima than a's: a stale maximum would show
        b[1, :10] = 0.0      # fewer ice cells
        slab.upload(PFT_BUF_X, D.padded(a))
        slab.upload(PFT_BUF_XN, D.padded(b))
        ra, pa = slab.diag(PFT_BUF_X)
        rb, pb = slab.diag(PFT_BUF_XN)
        ra2, pa2 = slab.diag(PFT_BUF_X)
        D.assert_same(ra, D.np_diag(a)[0])
        D.assert_same(rb, D.np_diag(b)[0])
        D.assert_same(ra2, ra)
        assert np.array_equal(pa, D.np_diag(a)[1]) and np.array_equal(pb, D.np_diag(b)[1])
        assert np.array_equal(pa2, pa) and rb["ice"] < ra["ice"] and rb["u_max"] < ra["u_max"]
    finally:
        slab.close()


# ---- solver level --------------------------------------------------------------------------

def _g20_sim(mode, tile=2, nprocs=1, rank=0, **kw):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        nprocs=nprocs, rank=rank, initial=A[f"traj_m{mode}_ic"], tau=1.0,
                        tau_min=info["tau_min"], delta=info["delta"], tile=tile, **kw)


def _row_diag(row):
    return {k: row[k] for k in D.FIELDS}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("pair", [0, 2])
def test_run_series_reproduces_golden(mode, pair, tmp_path):
    """the driver's loop to the golden snapshot times: the reference's (t, h, steps, steps_total,
    rc) rows, each with the diagnostics of the golden state -- with one launch per stage and with
    the pair kernels; the snapshot files hold the golden states"""
    meta, A = O.load_case("g20")
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _g20_sim(mode)
        assert P.lib().pft_solver_diag(None, C.byref(P.pft_diag()), None, None) == -3   # host IC, no solve yet
        with pytest.raises(RuntimeError, match="resident"):
            sim.diagnostics()
        rows = sim.run_series(times=meta["traj_times"], snapshot_path=str(tmp_path / "snap") if pair == 0 else None,
                              comment="g20")
        pairs = sim.stats().pairs
        last = sim.diagnostics(per_plane=True)
        sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    assert pairs == (1 if pair else 0)
    assert [r["snapshot"] for r in rows] == [0, 1, 2, 3] and rows[0]["rc"] is None and rows[0]["t"] == 0.0
    D.assert_same(_row_diag(rows[0]), D.np_diag(A[f"traj_m{mode}_ic"])[0], "snapshot 0")
    for i, r in enumerate(rows[1:]):
        ref = meta[f"traj_m{mode}"][i]
        assert (r["t"].hex(), r["h"].hex(), r["steps"], r["steps_total"], r["rc"]) == \
            (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
        want, _ = D.np_diag(A[f"traj_m{mode}_state{i}"])
        D.assert_same(_row_diag(r), want, f"snapshot {i + 1}")
        assert r["ice_fraction"] == want["ice"] / 2000
    assert np.array_equal(last["ice_per_plane"], D.np_diag(A[f"traj_m{mode}_state2"])[1])
    if pair == 0:
        probe = _g20_sim(mode, init_solver=False)
        for s in range(4):
            path = "%s.%03d.ncd" % (tmp_path / "snap", s)
            n1, n2, n3, info, _ = P.read_snapshot_info(path)
            assert (info.snapshot, info.total_snapshots, info.t) == (s, 4, rows[s]["t"])
            P.load_snapshot(probe, path)
            assert np.array_equal(probe.interior(), A[f"traj_m{mode}_ic" if s == 0 else f"traj_m{mode}_state{s - 1}"])
        probe.close()


def test_device_ic_diagnostics():
    """after the device IC at 50x50x100: the published first line, 8 720 of 250 000"""
    base, Pm, info = M.full_size_case(100, 0)
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       beads=O.beads(), tau=1.0, tau_min=info["tau_min"], delta=info["delta"], device_ic=True)
    try:
        d = sim.diagnostics(per_plane=True)
        h = sim.diagnostics(where="host", per_plane=True)
        rows = sim.run_series(times=[])
    finally:
        sim.close()
    assert (d["cells"], d["ice"], d["pore"]) == (250000, 8720, 105796) and d["ice_fraction"] == 0.03488
    D.assert_same(d, h)
    assert np.array_equal(d["ice_per_plane"], h["ice_per_plane"])
    assert len(rows) == 1 and rows[0]["ice"] == 8720


def _series_on_slabs(make_sim, nprocs, times):
    def run(sim):
        rows = sim.run_series(times=times)
        return rows, sim.diagnostics(per_plane=True)
    return M.loopback_run(nprocs, lambda r: make_sim(nprocs, r), run)


@pytest.mark.parametrize("case", ["g20", "ragged"])
def test_loopback_slabs_equal_one_slab(case):
    """3 loopback slabs: the global record on every rank is the single slab's, the ranks'
    ice_per_plane side by side are its array (snapshot 0 from the host arrays, then a solve)"""
    if case == "g20":
        T = 36.0

        def make(nprocs, rank):
            return _g20_sim(0, nprocs=nprocs, rank=rank)
    else:
        meta, A = O.load_case("ragged")
        Pm, info = O.params_from_meta(meta)
        state = A["state"].copy()
        state[1, 8:19, 3:9, 4:11] = 1.0        # ice across the slab interfaces (rows 10 and 20)
        T = meta["step_large"]["T"]

        def make(nprocs, rank):
            return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                                nprocs=nprocs, rank=rank, initial=state, tau=meta["step_large"]["h0"],
                                tau_min=info["tau_min"], delta=info["delta"], t0=meta["step_large"]["t0"], tile=2)
    one = make(1, 0)
    rows1 = one.run_series(times=[T])
    d1 = one.diagnostics(per_plane=True)
    one.download()
    x1 = one.interior()
    one.close()
    D.assert_same(_row_diag(rows1[1]), D.np_diag(x1)[0])
    assert rows1[1]["ice"] > 0
    out = _series_on_slabs(make, 3, [T])
    for rows, d in out:
        for a, b in zip(rows, rows1):
            assert a == b
        D.assert_same(d, d1)
    assert [d["first_row"] for _, d in out] == [P.decompose(len(d1["ice_per_plane"]), 3, r)[1] for r in range(3)]
    assert np.array_equal(np.concatenate([d["ice_per_plane"] for _, d in out]), d1["ice_per_plane"])
    local = [d["local"] for _, d in out]
    assert sum(r["ice"] for r in local) == d1["ice"] and sum(r["cells"] for r in local) == d1["cells"]


def test_two_ipc_processes(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_diag_worker.py): both ranks report the
    golden state's global record; their planes side by side are the whole grid's"""
    meta, A = O.load_case("g20")
    spec = {"nranks": 2, "shm": f"/pft_diag_{os.getpid()}_{uuid.uuid4().hex[:12]}", "out": str(tmp_path / "rank"),
            "times": [meta["traj_times"][0]]}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_diag_worker.py"), str(path), str(r)], env=env,
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
    res = [json.load(open(f"{spec['out']}.{r}.json")) for r in range(2)]
    want0, _ = D.np_diag(A["traj_m0_ic"])
    want1, planes1 = D.np_diag(A["traj_m0_state0"])
    ref = meta["traj_m0"][0]
    for r in res:
        D.assert_same(r["rows"][0], want0, "snapshot 0")
        D.assert_same(r["rows"][1], want1, "snapshot 1")
        D.assert_same(r["diag"], want1)
        row = r["rows"][1]
        assert (float(row["t"]).hex(), float(row["h"]).hex(), row["steps"], row["steps_total"], row["rc"]) == \
            (float.fromhex(ref[0]).hex(), float.fromhex(ref[1]).hex(), ref[2], ref[3], ref[4])
    assert [r["first_row"] for r in res] == [0, 10]
    assert np.array_equal(np.concatenate([r["ice_per_plane"] for r in res]), planes1)


def test_diag_inside_a_service_callback():
    """at the 25th accepted step: pft_solver_diag describes the state pft_solver_download gives in
    the same callback (tests/golden/ctl cb_break_state0)"""
    _, A = O.load_case("ctl")
    sim = _g20_sim(0, tile=32)
    got = []

    @P.SERVICE_FN
    def cb(final, s):
        if s.contents.steps == 25:
            d, planes = P.pft_diag(), (C.c_longlong * 20)()
            rc = sim.lib.pft_solver_diag(None, C.byref(d), None, planes)
            assert sim.lib.pft_solver_download(s) == 0
            got.append((rc, D.rec_of(d), np.array(planes[:], dtype=np.int64), sim.interior()))
        return 0

    sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
    sim.solve(36.0)
    sim.close()
    assert len(got) == 1
    rc, d, planes, x = got[0]
    assert rc == 0 and np.array_equal(x, A["cb_break_state0"])
    want, want_planes = D.np_diag(x)
    D.assert_same(d, want)
    assert np.array_equal(planes, want_planes)
