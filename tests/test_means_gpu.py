"""f6 on the GPU: the means kernels (pft_slab_means) against pft_means_host word for word and
against exact rational arithmetic (fractions.Fraction sums rounded once) by ==, on shapes that take
every path -- an odd plane with misaligned planes, a plane smaller than a wave, several workgroups
per plane, fewer workgroups than planes -- with fields that keep a wave on its register path and
fields that force the per-lane LDS atomics; pft_solver_means / Simulation.means / run_series on one
slab, on loopback slabs, in two ipc processes and from a Service_Callback."""
import ctypes as C
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import _diag as D
import _means as Mn
import _multi as M
import _oracle as O
import porousfreezethaw_amd as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PFT_BUF_X, PFT_BUF_XN = 0, 1


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


def _check_state(slab, a, opts=None, which=PFT_BUF_X):
    """upload a (ghost planes poisoned), then device words == host twin's words, for the slab and
    for every plane, and the values == the Fraction results"""
    n3, n2, n1 = a.shape[1:]
    w = D.padded(a)
    slab.upload(which, w)
    total, planes = slab.means(which, opts)
    host, host_planes = Mn.host_means(D.grid(n1, n2, n3), w, opts)
    Mn.assert_words(total, host, "device against pft_means_host")
    for k in range(n3):
        Mn.assert_words(planes[k], host_planes[k], f"plane {k}: device against pft_means_host")
    alone, _ = slab.means(which, opts, per_plane=False)
    Mn.assert_words(alone, host, "without per_plane")
    want = Mn.ref_means(a, *(opts or (0.5, 0.5)))
    got = Mn.record_dict(total, planes)
    Mn.assert_scalars(got, want, "device against Fraction")
    Mn.assert_profiles(got, want, "device against Fraction")
    return total, planes


# (n1, n2, n3, PFT_DIAG_WGS); a workgroup takes 2048 elements per iteration, a wave 512 of them.
# 13x11x9: an odd plane (143), every second plane starts on an odd multiple of 8 bytes; 3x1x200: a
# plane smaller than a wave, 200 planes; 120x60x4: 7200-element planes cut into 4 segments, the
# last one short; 40x40x8 with 1 and 3 workgroups: a workgroup takes several planes in turn, and
# uncapped; 50x50x3: whole 16-byte iterations inside a segment and ragged ends
SHAPES = [(13, 11, 9, 0), (3, 1, 200, 0), (120, 60, 4, 0), (40, 40, 8, 1), (40, 40, 8, 3), (40, 40, 8, 0),
          (50, 50, 3, 0)]


@pytest.mark.parametrize("n1,n2,n3,wgs", SHAPES)
def test_slab_means_equals_host_and_fraction(n1, n2, n3, wgs, monkeypatch):
    if wgs:
        monkeypatch.setenv("PFT_DIAG_WGS", str(wgs))
    slab = Mn.Slab(n1, n2, n3)
    try:
        a = D.random_state(n1, n2, n3, 61)
        total, _ = _check_state(slab, a)
        assert total.n[0] == n1 * n2 * n3
        _check_state(slab, a, opts=(0.7, 0.25))
        _check_state(slab, Mn.wide_state(n1, n2, n3, 62))           # the per-lane path, c changing
        _check_state(slab, Mn.special(a, 63))
        _check_state(slab, Mn.special(Mn.wide_state(n1, n2, n3, 64), 65))
        total, _ = _check_state(slab, np.full_like(a, np.nan))
        assert not any(total.words())
    finally:
        slab.close()


def test_uniform_path_equals_forced_slow_path():
    """u in [256, 512) and p in [0.5, 1) keep every lane at one word index; one outlier per wave
    iteration (512 elements), put where the field is zero, sends that iteration through the
    per-slot path.  Both are the host twin's words, and their difference is exactly the
    outliers' own digits."""
    n1, n2, n3 = 64, 48, 5
    r = np.random.default_rng(71)
    a = np.empty((3, n3, n2, n1))
    a[0] = r.uniform(256.0, 512.0, size=(n3, n2, n1))
    a[1] = r.uniform(0.5, 1.0, size=(n3, n2, n1))
    a[2] = r.choice([0.0, 1.0], size=(n3, n2, n1))
    flat = a.reshape(3, -1)
    n = flat.shape[1]
    spots = np.arange(37, n, 512)                 # one per wave iteration
    flat[0, spots] = 0.0
    flat[1, spots] = 0.0
    b = a.copy()
    fb = b.reshape(3, -1)
    out_u = np.ldexp(r.uniform(1.0, 2.0, size=spots.size), r.integers(-900, 900, size=spots.size).astype(np.int32))
    out_p = -np.ldexp(r.uniform(1.0, 2.0, size=spots.size), r.integers(-900, -40, size=spots.size).astype(np.int32))
    fb[0, spots] = out_u
    fb[1, spots] = out_p                          # negative: not ice
    slab = Mn.Slab(n1, n2, n3)
    try:
        ta, _ = _check_state(slab, a)
        tb, _ = _check_state(slab, b)
    finally:
        slab.close()
    assert [j for j, w in enumerate(ta.sum[0].w) if w] == [32, 33]      # u never left its window
    diff_u, diff_p = P.pft_xsum(), P.pft_xsum()
    for x in out_u.tolist():
        P.lib().pft_xsum_add(C.byref(diff_u), x)
    for x in out_p.tolist():
        P.lib().pft_xsum_add(C.byref(diff_p), x)
    assert [tb.sum[0].w[j] - ta.sum[0].w[j] for j in range(66)] == list(diff_u.w)
    assert [tb.sum[1].w[j] - ta.sum[1].w[j] for j in range(66)] == list(diff_p.w)
    assert list(tb.sum[2].w) == list(ta.sum[2].w)                        # the outliers' cells are no ice
    assert list(tb.n) == list(ta.n)


def test_no_accumulator_carries_over():
    """X, then XN holding another state, then X again: each call returns its buffer's own words"""
    slab = Mn.Slab(10, 10, 20)
    try:
        a, b = D.random_state(10, 10, 20, 81), Mn.wide_state(10, 10, 20, 82)
        slab.upload(PFT_BUF_X, D.padded(a))
        slab.upload(PFT_BUF_XN, D.padded(b))
        ha, _ = Mn.host_means(D.grid(10, 10, 20), D.padded(a))
        hb, _ = Mn.host_means(D.grid(10, 10, 20), D.padded(b))
        ra, pa = slab.means(PFT_BUF_X)
        rb, pb = slab.means(PFT_BUF_XN)
        ra2, pa2 = slab.means(PFT_BUF_X)
        Mn.assert_words(ra, ha, "X")
        Mn.assert_words(rb, hb, "XN after X")
        Mn.assert_words(ra2, ha, "X again")
        assert ra.words() != rb.words()
        for k in range(20):
            Mn.assert_words(pa2[k], pa[k], f"plane {k}")
    finally:
        slab.close()


# ---- solver level --------------------------------------------------------------------------

def _g20_sim(mode, tile=2, nprocs=1, rank=0, **kw):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        nprocs=nprocs, rank=rank, initial=A[f"traj_m{mode}_ic"], tau=1.0,
                        tau_min=info["tau_min"], delta=info["delta"], tile=tile, **kw)


TODAYS_KEYS = {"snapshot", "t", "h", "steps", "steps_total", "rc", "ice_fraction"} | set(D.FIELDS)


@pytest.mark.parametrize("pair", [0, 2])
def test_run_series_means_reproduce_golden(pair, tmp_path):
    """the driver's loop to the golden snapshot times with means=True: every row carries the
    Fraction results of the golden state, with one launch per stage and with the pair kernels;
    with the default the rows have exactly the keys they had"""
    meta, A = O.load_case("g20")
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _g20_sim(0)
        assert P.lib().pft_solver_means(None, C.byref(P.pft_means()), None, None) == -3   # host IC, no solve yet
        with pytest.raises(RuntimeError, match="resident"):
            sim.means()
        rows = sim.run_series(times=meta["traj_times"], means=True)
        pairs = sim.stats().pairs
        last = sim.means(per_plane=True)
        sim.download()
        host = sim.means(where="host", per_plane=True)
        sim.close()
        sim = _g20_sim(0)
        plain = sim.run_series(times=meta["traj_times"][:1])
        sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    assert pairs == (1 if pair else 0)
    assert [r["snapshot"] for r in rows] == [0, 1, 2, 3]
    states = [A["traj_m0_ic"]] + [A[f"traj_m0_state{i}"] for i in range(3)]
    for r, a in zip(rows, states):
        Mn.assert_scalars(r, Mn.ref_means(a, per_plane=False), f"snapshot {r['snapshot']}")
        assert set(r) == TODAYS_KEYS | set(Mn.SCALARS)
    want = Mn.ref_means(states[3])
    Mn.assert_scalars(last, want, "means() after the series")
    Mn.assert_profiles(last, want, "means() after the series")
    Mn.assert_scalars(host, want, "where='host'")
    Mn.assert_profiles(host, want, "where='host'")
    Mn.assert_words(last["record"], host["record"], "device against host")
    assert last["first_row"] == 0 and states[3][0].min() < last["u_mean"] < states[3][0].max()
    for r, q in zip(plain, rows):
        assert set(r) == TODAYS_KEYS
        assert all(r[k] == q[k] for k in TODAYS_KEYS)
    path = tmp_path / "u_mean.txt"
    P.write_series_txt(rows, str(path), key="u_mean")
    assert path.read_text() == "".join("%.15g \n" % r["u_mean"] for r in rows)


@pytest.mark.parametrize("case", ["g20", "ragged"])
def test_loopback_slabs_equal_one_slab(case):
    """3 loopback slabs (g20: 20 rows cut unevenly; the ragged fixture with ice across the slab
    interfaces): the global record on every rank is the single slab's word for word, the ranks'
    plane records side by side are its planes'"""
    if case == "g20":
        T = 36.0
        info = {"n3": 20}

        def make(nprocs, rank):
            return _g20_sim(0, nprocs=nprocs, rank=rank)
    else:
        meta, A = O.load_case("ragged")
        Pm, info = O.params_from_meta(meta)
        state = A["state"].copy()
        state[1, 8:19, 3:9, 4:11] = 1.0
        T = meta["step_large"]["T"]

        def make(nprocs, rank):
            return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                                nprocs=nprocs, rank=rank, initial=state, tau=meta["step_large"]["h0"],
                                tau_min=info["tau_min"], delta=info["delta"], t0=meta["step_large"]["t0"], tile=2)

    def run(sim):
        rows = sim.run_series(times=[T], means=True)
        d = sim.means(per_plane=True)
        return rows, d, d["record"].words(), [m.words() for m in d["plane_records"]]

    one = make(1, 0)
    rows1, d1, words1, planes1 = run(one)
    one.download()
    x1 = one.interior()
    one.close()
    want = Mn.ref_means(x1)
    Mn.assert_scalars(rows1[1], want, "one slab")
    Mn.assert_profiles(d1, want, "one slab")
    assert d1["ice_u_n"] > 0
    out = M.loopback_run(3, lambda r: make(3, r), run)
    for rows, d, words, _ in out:
        for a, b in zip(rows, rows1):
            assert set(a) == set(b) and all(Mn.same(a[k], b[k]) for k in a)
        assert words == words1
        Mn.assert_scalars(d, d1, "loopback rank")
    assert [d["first_row"] for _, d, _, _ in out] == [P.decompose(info["n3"], 3, r)[1] for r in range(3)]
    assert sum((pl for _, _, _, pl in out), []) == planes1
    assert sum(d["local"]["u_n"] for _, d, _, _ in out) == d1["u_n"]


def test_two_ipc_processes(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_means_worker.py): both ranks report the
    golden state's global record; their plane records side by side are the whole grid's"""
    meta, A = O.load_case("g20")
    spec = {"nranks": 2, "shm": f"/pft_means_{os.getpid()}_{uuid.uuid4().hex[:12]}", "out": str(tmp_path / "rank"),
            "times": [meta["traj_times"][0]]}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_means_worker.py"), str(path), str(r)], env=env,
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
    a = A["traj_m0_state0"]
    want0, want1 = Mn.ref_means(A["traj_m0_ic"], per_plane=False), Mn.ref_means(a)
    host, host_planes = Mn.host_means(D.grid(10, 10, 20), D.padded(a))
    for r in res:
        Mn.assert_scalars(r["rows"][0], want0, "snapshot 0")
        Mn.assert_scalars(r["rows"][1], want1, "snapshot 1")
        assert r["words"] == host.words()
    assert [r["first_row"] for r in res] == [0, 10]
    assert res[0]["plane_words"] + res[1]["plane_words"] == [m.words() for m in host_planes]
    got = {k + "_profile": res[0]["profiles"][k + "_profile"] + res[1]["profiles"][k + "_profile"] for k in Mn.KEYS}
    Mn.assert_profiles(got, want1, "the ranks' profiles side by side")
    assert res[0]["local"]["u_n"] + res[1]["local"]["u_n"] == 2000


def test_means_inside_a_service_callback():
    """at the 25th accepted step on one rank: pft_solver_means returns 0 and describes the state
    pft_solver_download gives in the same callback (tests/golden/ctl cb_break_state0)"""
    _, A = O.load_case("ctl")
    sim = _g20_sim(0, tile=32)
    got = []

    @P.SERVICE_FN
    def cb(final, s):
        if s.contents.steps == 25:
            m, planes = P.pft_means(), (P.pft_means * 20)()
            rc = sim.lib.pft_solver_means(None, C.byref(m), None, planes)
            assert sim.lib.pft_solver_download(s) == 0
            got.append((rc, Mn.record_dict(m, planes), sim.interior()))
        return 0

    sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
    sim.solve(36.0)
    sim.close()
    assert len(got) == 1
    rc, d, x = got[0]
    assert rc == 0 and np.array_equal(x, A["cb_break_state0"])
    want = Mn.ref_means(x)
    Mn.assert_scalars(d, want)
    Mn.assert_profiles(d, want)
