"""f12 on the GPU: the formula kernels (pft_slab_formulas) against pft_formula_host word for word and
against the independent reference (tests/_formula.py) by ==, on the shapes of tests/test_means_gpu.py
-- an odd plane with misaligned planes, a plane smaller than a wave, several segments per plane,
fewer workgroups than planes -- for all of the formula set in two calls, with fields that keep a
wave on its register path and fields that force the per-lane LDS atomics; the identities with
pft_slab_diag and pft_slab_means from the same upload; pft_solver_formulas / Simulation.formulas /
run_series / Case.run on one slab, on loopback slabs, in two ipc processes and from a
Service_Callback."""
import ctypes as C
import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import _diag as D
import _formula as Fm
import _means as Mn
import _multi as M
import _oracle as O
import _snap as S
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PFT_BUF_X, PFT_BUF_XN = 0, 1


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


class Slab(Mn.Slab):
    """tests/_means.py's bare slab with the f12 and f5 entries"""

    def __init__(self, n1, n2, n3):
        super().__init__(n1, n2, n3)
        self.grid = Fm.grid(n1, n2, n3)

    def formulas(self, which, formulas, per_plane=True):
        c = Fm.Compiled(self.grid, formulas)
        try:
            assert c.codes == [0] * len(c.names), c.codes
            n = len(c.names)
            total = (P.pft_fdiag * n)()
            planes = (P.pft_fdiag * (n * self.n3))() if per_plane else None
            rc = self.L.pft_slab_formulas(self.s, which, n, c.progs, total, planes)
            assert rc == 0, (rc, self.L.pft_hip_last_error())
        finally:
            c.free()
        split = None if planes is None else [[planes[f * self.n3 + k] for k in range(self.n3)] for f in range(n)]
        return c.names, total, split

    def diag(self, which):
        d = P.pft_diag()
        assert self.L.pft_slab_diag(self.s, which, None, C.byref(d), None) == 0
        return D.rec_of(d)


def _check_state(slab, tag, make, which=PFT_BUF_X):
    """upload the state (ghost planes poisoned), then for all of F in two calls: device words and
    counts == the host twin's, for the slab and for every plane, with and without per_plane, and
    the values == the independent reference; returns {name: record}"""
    a = make()
    n3, n2, n1 = a.shape[1:]
    w = D.padded(a)
    slab.upload(which, w)
    out = {}
    for formulas in Fm.CALLS:
        names, total, planes = slab.formulas(which, formulas)
        _, host, host_planes = Fm.host_formulas(slab.grid, w, formulas)
        _, alone, _ = slab.formulas(which, formulas, per_plane=False)
        want = Fm.cached_reference((tag, n1, n2, n3), formulas, lambda: a)
        for f, name in enumerate(names):
            Fm.assert_words(total[f], host[f], f"{tag} {name}: device against pft_formula_host")
            for k in range(n3):
                Fm.assert_words(planes[f][k], host_planes[f][k], f"{tag} {name} plane {k}: device against pft_formula_host")
            Fm.assert_words(alone[f], host[f], f"{tag} {name}: without per_plane")
            Fm.assert_dict(total[f].as_dict(), want[name][0], f"{tag} {name}: device against the reference")
            for k in range(n3):
                Fm.assert_dict(planes[f][k].as_dict(), want[name][1][k], f"{tag} {name} plane {k}: against the reference")
            out[name] = total[f]
    return out


def _check_identities(slab, tag, r, which=PFT_BUF_X):
    """f5 and f6 of the same upload as special cases of the formula set"""
    diag = slab.diag(which)
    means, _ = slab.means(which, per_plane=False)
    assert r["f1"].nonzero == diag["ice"] and r["f1"].as_dict()["sum"] == float(diag["ice"])
    assert r["f1"].as_dict()["mean"] == diag["ice"] / diag["cells"]                     # ice_fraction
    assert r["f2"].nonzero == diag["pore"]
    assert list(r["f3"].sum.w) == list(means.sum[0].w) and r["f3"].n == means.n[0]
    assert Mn.same(r["f3"].min, diag["u_min"]) and Mn.same(r["f3"].max, diag["u_max"])
    if tag != "special":
        assert Mn.same(r["f4"].maxabs, diag["ice_u_maxabs"])
        assert list(r["f4"].sum.w) == list(means.sum[2].w)


# the shapes of tests/test_means_gpu.py, for its reasons: (n1, n2, n3, PFT_DIAG_WGS)
SHAPES = [(13, 11, 9, 0), (3, 1, 200, 0), (120, 60, 4, 0), (40, 40, 8, 1), (40, 40, 8, 3), (50, 50, 3, 0)]


@pytest.mark.parametrize("n1,n2,n3,wgs", SHAPES)
def test_slab_formulas_equal_host_and_reference(n1, n2, n3, wgs, monkeypatch):
    if wgs:
        monkeypatch.setenv("PFT_DIAG_WGS", str(wgs))
    slab = Slab(n1, n2, n3)
    try:
        for tag, make in Fm.states(n1, n2, n3):
            r = _check_state(slab, tag, make)
            assert r["f3"].cells == n1 * n2 * n3
            _check_identities(slab, tag, r)
    finally:
        slab.close()


def test_not_device_exact_and_bad_programs_launch_nothing():
    """the four non-exact formulas compile to code 1; a residual program with an operator the device
    does not run, C or P among them, or a stack past the LDS column gets code 1 from the slab entry
    too, a malformed program, tables of another grid and more than 8 programs -2: before anything
    is launched (the out records stay as they were)"""
    slab = Slab(13, 11, 9)
    try:
        c = Fm.Compiled(slab.grid, Fm.NOT_EXACT)
        assert c.codes == [1, 1, 1, 1]
        c.free()
        out = (P.pft_fdiag * 9)()

        def raw(ops, args):
            ops, args = np.array(ops, dtype=np.int32), np.array(args, dtype=np.float64)
            pr = P.pft_ic_prog(len(ops), P._ip(ops), P._dp(args), 0, None, None, None, None, 0, 0)
            return slab.L.pft_slab_formulas(slab.s, PFT_BUF_X, 1, C.byref(pr), out, None)

        assert raw([101, 101, 2], [6, 7, 0]) == 0
        out[0].cells = -77                                  # a mark no refused call may touch
        assert raw([101, 100, 5], [6, 2, 0]) == 1           # u C 2: not device-exact
        assert raw([101, 100, 6], [6, 2, 0]) == 1           # u P 2
        assert raw([101, 42], [6, 0]) == 1                  # exp(u)
        assert raw([101, 100, 7], [6, 2, 0]) == 1           # u^2
        assert raw([101] * 17 + [2] * 16, [6] * 17 + [0] * 16) == 1         # a stack of 17
        assert raw([101, 16], [6, 0]) == -2 and raw([101, 49], [6, 0]) == -2     # no such operator
        assert raw([101] * 16 + [2] * 15, [6] * 16 + [0] * 15) == 0         # ... of 16
        out[0].cells = -77
        assert raw([101, 2], [6, 0]) == -2 and raw([101, 101], [6, 6]) == -2 and raw([101], [5]) == -2
        assert raw([102], [0]) == -2                        # no such table
        assert out[0].cells == -77
        other = Fm.Compiled(Fm.grid(12, 11, 9), {"a": "tanh(x)*u"})     # tables of another grid
        assert other.codes == [0]
        assert slab.L.pft_slab_formulas(slab.s, PFT_BUF_X, 1, other.progs, out, None) == -2
        other.free()
        nine = Fm.Compiled(slab.grid, {"a": "u"})
        progs = (P.pft_ic_prog * 9)(*([nine.progs[0]] * 9))
        assert slab.L.pft_slab_formulas(slab.s, PFT_BUF_X, 9, progs, out, None) == -2
        assert slab.L.pft_slab_formulas(slab.s, PFT_BUF_X, 8, progs, out, None) == 0
        nine.free()
    finally:
        slab.close()


def test_no_accumulator_carries_over():
    """X, then XN holding another state, then X again: each call returns its buffer's own words"""
    slab = Slab(10, 10, 20)
    try:
        a, b = D.random_state(10, 10, 20, 81), Mn.wide_state(10, 10, 20, 82)
        slab.upload(PFT_BUF_X, D.padded(a))
        slab.upload(PFT_BUF_XN, D.padded(b))
        for formulas in Fm.CALLS:
            _, ha, _ = Fm.host_formulas(slab.grid, D.padded(a), formulas)
            _, hb, _ = Fm.host_formulas(slab.grid, D.padded(b), formulas)
            names, ra, pa = slab.formulas(PFT_BUF_X, formulas)
            _, rb, _ = slab.formulas(PFT_BUF_XN, formulas)
            _, ra2, pa2 = slab.formulas(PFT_BUF_X, formulas)
            for f, name in enumerate(names):
                Fm.assert_words(ra[f], ha[f], f"{name}: X")
                Fm.assert_words(rb[f], hb[f], f"{name}: XN after X")
                Fm.assert_words(ra2[f], ha[f], f"{name}: X again")
                for k in range(20):
                    Fm.assert_words(pa2[f][k], pa[f][k], f"{name} plane {k}")
            if "f3" in names:
                assert ra[names.index("f3")].words() != rb[names.index("f3")].words()
        # one program after eight: the records past the first belong to no one
        _, one, _ = slab.formulas(PFT_BUF_X, {"f3": Fm.F["f3"]})
        Fm.assert_words(one[0], Fm.host_formulas(slab.grid, D.padded(a), {"f3": Fm.F["f3"]})[1][0], "one after eight")
    finally:
        slab.close()


# ---- solver level --------------------------------------------------------------------------

def _g20_sim(mode, tile=2, nprocs=1, rank=0, **kw):
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        nprocs=nprocs, rank=rank, initial=A[f"traj_m{mode}_ic"], tau=1.0,
                        tau_min=info["tau_min"], delta=info["delta"], tile=tile, **kw)


def _g20_variables():
    """the golden case's parameters and lengths as formula variables"""
    meta, _ = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    v = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
    v.update(L1=info["L1"], L2=info["L2"], L3=info["L3"])
    return v


SERIES = {"ice": Fm.F["f1"], "heat": Fm.F["f8"], "supercooled": Fm.F["f5"], "top_ice": Fm.F["f6"]}


@pytest.mark.parametrize("pair", [0, 2])
def test_run_series_formulas_on_golden(pair, tmp_path):
    """the driver's loop on golden g20 to t = 36 s with formulas=, with one launch per stage and with
    the pair kernels: the rows' t, h and step counts are those of a run without formulas, ice_mean
    is the row's ice_fraction at every snapshot, formula 8 equals the host route on the downloaded
    state; the non-exact formulas raise on the device and give the reference on the host"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _g20_sim(0)
        lens, ops, args = (np.array([1], dtype=np.int32), np.array([101], dtype=np.int32), np.array([6.0]))
        assert P.lib().pft_solver_formulas(1, P._ip(lens), P._ip(ops), P._dp(args), (P.pft_fdiag * 1)(), None, None) == -3
        with pytest.raises(RuntimeError, match="resident"):
            sim.formulas({"a": "u"})
        rows = sim.run_series(times=meta["traj_times"][:1], formulas=SERIES, variables=V)
        pairs = sim.stats().pairs
        dev = sim.formulas(SERIES, V, per_plane=True)
        with pytest.raises(ValueError, match="'e1'.*not device-exact"):
            sim.formulas({"f3": "u", **Fm.NOT_EXACT}, V)
        with pytest.raises(ValueError, match="'e3'"):
            sim.formulas({"e3": "u C 2"}, V)
        sim.download()
        host = sim.formulas(SERIES, V, where="host", per_plane=True)
        inexact = sim.formulas(Fm.NOT_EXACT, V, where="host")
        x = sim.interior()
        sim.close()
        sim = _g20_sim(0)
        plain = sim.run_series(times=meta["traj_times"][:1])
        sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    assert pairs == (1 if pair else 0)
    assert np.array_equal(x, A["traj_m0_state0"])
    assert [r["snapshot"] for r in rows] == [0, 1] and rows[1]["t"] == 36.0
    for r, q in zip(rows, plain):
        assert all(r[k] == q[k] for k in q)
        assert set(r) == set(q) | {n + "_" + k for n in SERIES for k in P.FORMULA_ROW_KEYS}
        assert r["ice_mean"] == r["ice_fraction"] and r["ice_nonzero"] == r["ice"] and r["ice_n"] == r["cells"]
    want = Fm.reference(SERIES, x, variables=V)
    ref0 = Fm.reference({"heat": SERIES["heat"]}, A["traj_m0_ic"], variables=V)["heat"][0]
    assert all(Mn.same(rows[0]["heat_" + k], ref0[k]) for k in P.FORMULA_ROW_KEYS)       # the host IC's first snapshot
    for name in SERIES:
        Fm.assert_words(dev[name]["record"], host[name]["record"], f"{name}: device against host")
        Fm.assert_dict(dev[name], want[name][0], name)
        assert [m.words() for m in dev[name]["plane_records"]] == [m.words() for m in host[name]["plane_records"]]
        assert all(Mn.same(rows[1][name + "_" + k], want[name][0][k]) for k in P.FORMULA_ROW_KEYS)
        assert dev[name]["first_row"] == 0 and dev[name]["local"] == {k: dev[name][k] for k in Fm.KEYS}
    assert rows[1]["heat_sum"] == host["heat"]["sum"] and rows[1]["heat_sum"] != 0.0
    ref = Fm.reference(Fm.NOT_EXACT, x, variables=V)
    for name in Fm.NOT_EXACT:
        Fm.assert_dict(inexact[name], ref[name][0], f"{name} on the host")
    path = tmp_path / "supercooled_mean.txt"
    P.write_series_txt(rows, str(path), key="supercooled_mean")
    assert path.read_text() == "".join("%.15g \n" % r["supercooled_mean"] for r in rows)


def test_case_run_formulas_with_a_params_variable(tmp_path):
    """Case.run(formulas=) compiles with the case's own evaluator: a variable of the parameter file
    appears in a formula; an undefined one ends the run before any work"""
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    lines = [f"{k} {v!r}" for k, v in zip(P.PARAM_NAMES, (float(x) for x in Pm))]
    lines += [f"L1 {info['L1']!r}", f"L2 {info['L2']!r}", f"L3 {info['L3']!r}", f"n1 {info['n1']}", f"n2 {info['n2']}",
              f"n3 {info['n3']}", "saved_files 2", "tau 1", "final_time 36", f"delta {info['delta']!r}",
              f"tau_min {info['tau_min']!r}", "my_threshold u_star + 1",
              'icond u = "u_star + 5*_z"', 'icond p = "_z < 0.3"', 'icond gl = "0"']
    case = FE.load_params(text="\n".join(lines) + "\n")
    with pytest.raises(FE.EvalError, match="nope"):
        case.run(formulas={"a": "u > nope"})
    rows = case.run(formulas={"warm": "u > my_threshold", "ice": "p>0.5"}, tile=2)
    thr = case.ev.value("my_threshold")
    sim = case.simulation(tile=2)
    try:
        ic = sim.interior()
    finally:
        sim.close()
    assert [r["snapshot"] for r in rows] == [0, 1]
    assert rows[0]["warm_nonzero"] == int((ic[0] > thr).sum()) > 0 and rows[0]["warm_n"] == ic[0].size
    assert all(r["ice_mean"] == r["ice_fraction"] for r in rows)
    assert 0 < rows[1]["warm_nonzero"] < ic[0].size


@pytest.mark.parametrize("case", ["7x5x7", "g20", "ragged"])
def test_loopback_slabs_equal_one_slab(case, tmp_path):
    """3 loopback slabs (7x5x7: slabs of 3 / 2 / 2 planes of 35 cells, less than a wave, every second
    plane on an odd multiple of 8 bytes, the state read from a dataset and reduced as it stands;
    g20: 7 / 6 / 7 rows; the ragged fixture, 18x12x30 with ice across the slab interfaces): every
    rank's global records are the single slab's word for word and its plane records side by side are
    the single slab's planes' -- formula 6's threshold plane lies inside one slab (7x5x7: k >= 4, in
    the middle slab's rows 3-4), formula 7's tables do not depend on the slab.  On 7x5x7 both also
    equal pft_formula_host and the independent reference of the whole state"""
    small = None
    if case == "7x5x7":
        T = None                                       # no solve: the state of the dataset itself
        Pm = O.params_from_meta(O.load_case("g20")[0])[0]
        V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
        V.update(L1=Fm.L[0], L2=Fm.L[1], L3=Fm.L[2])
        info = {"n3": 7}
        small = D.random_state(7, 5, 7, 91)
        small[2] = np.abs(small[2])
        small[1, :, 2, 3] = [1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.75]     # the disc's centre: ice on both sides of plane 4
        small[1, 3:5, 0, 0] = 1.0                                     # ... and outside the disc, in rows 3 and 4
        first = str(tmp_path / "first.ncd")
        inf = P.snapshot_info(36.0, 0.5, 72.0, 1e-3, 0, snapshot=3, total_snapshots=9, comment="slabs")
        S.write_host(first, Fm.grid(7, 5, 7), Pm, inf, D.padded(small, poison=False))

        def make(nprocs, rank):
            return P.Simulation(7, 5, 7, Fm.L, 0, Pm, nprocs=nprocs, rank=rank, icond_file=first)
    elif case == "g20":
        T, V = 36.0, _g20_variables()
        info = {"n3": 20}

        def make(nprocs, rank):
            return _g20_sim(0, nprocs=nprocs, rank=rank)
    else:
        meta, A = O.load_case("ragged")
        Pm, info = O.params_from_meta(meta)
        V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
        V.update(L1=info["L1"], L2=info["L2"], L3=info["L3"])
        state = A["state"].copy()
        state[1, 8:19, 3:9, 4:11] = 1.0
        T = meta["step_large"]["T"]

        def make(nprocs, rank):
            return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                                nprocs=nprocs, rank=rank, initial=state, tau=meta["step_large"]["h0"],
                                tau_min=info["tau_min"], delta=info["delta"], t0=meta["step_large"]["t0"], tile=2)

    def run(sim):
        rows = sim.run_series(times=[] if T is None else [T], formulas=Fm.CALLS[1], variables=V)
        out = {}
        for call in Fm.CALLS:
            for name, d in sim.formulas(call, V, per_plane=True).items():
                out[name] = (d["record"].words(), [m.words() for m in d["plane_records"]], d["first_row"], d["local"]["cells"])
        return rows, out

    one = make(1, 0)
    rows1, out1 = run(one)
    one.close()
    assert out1["f6"][0][2] > 0 and out1["f7"][0][2] > 0          # some ice in the upper half and in the disc
    if small is not None:
        assert 0 < out1["f6"][0][2] < out1["f1"][0][2] and 0 < out1["f7"][0][2] < out1["f1"][0][2]
        w = D.padded(small)
        for call in Fm.CALLS:
            names, host, host_planes = Fm.host_formulas(Fm.grid(7, 5, 7), w, call, variables=V)
            want = Fm.reference(call, small, variables=V)
            for f, name in enumerate(names):
                assert out1[name][0] == host[f].words(), name
                assert out1[name][1] == [m.words() for m in host_planes[f]], name
                Fm.assert_dict(host[f].as_dict(), want[name][0], name)
    res = M.loopback_run(3, lambda r: make(3, r), run)
    for rows, out in res:
        for a, b in zip(rows, rows1):
            assert set(a) == set(b) and all(Mn.same(a[k], b[k]) for k in a)
        for name in Fm.F:
            assert out[name][0] == out1[name][0], name
    for name in Fm.F:
        assert sum((out[name][1] for _, out in res), []) == out1[name][1], name
        assert [out[name][2] for _, out in res] == [P.decompose(info["n3"], 3, r)[1] for r in range(3)]
        assert sum(out[name][3] for _, out in res) == out1[name][0][0]


def test_two_ipc_processes(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_formula_worker.py): both ranks report the
    golden state's global records; their plane records side by side are the whole grid's"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    spec = {"nranks": 2, "shm": f"/pft_formula_{os.getpid()}_{uuid.uuid4().hex[:12]}", "out": str(tmp_path / "rank"),
            "times": [meta["traj_times"][0]], "formulas": Fm.CALLS[0], "variables": V}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_formula_worker.py"), str(path), str(r)], env=env,
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
    g = D.grid(10, 10, 20)
    meta_info = O.params_from_meta(meta)[1]
    g.L1, g.L2, g.L3 = meta_info["L1"], meta_info["L2"], meta_info["L3"]
    names, host, host_planes = Fm.host_formulas(g, D.padded(a), Fm.CALLS[0], variables=V)
    want = Fm.reference(Fm.CALLS[0], a, variables=V)
    assert [r["first_row"] for r in res] == [0, 10] and res[0]["not_exact"] == res[1]["not_exact"] == "ValueError"
    for f, name in enumerate(names):
        for r in res:
            assert r["words"][name] == host[f].words(), name
            assert all(Mn.same(r["rows"][1][name + "_" + k], want[name][0][k]) for k in P.FORMULA_ROW_KEYS)
        assert res[0]["plane_words"][name] + res[1]["plane_words"][name] == [m.words() for m in host_planes[f]]
        assert res[0]["local_cells"][name] + res[1]["local_cells"][name] == 2000


def test_formulas_inside_a_service_callback():
    """at the 25th accepted step on one rank: pft_solver_formulas returns 0 and describes the state
    pft_solver_download gives in the same callback (tests/golden/ctl cb_break_state0)"""
    _, A = O.load_case("ctl")
    V = _g20_variables()
    sim = _g20_sim(0, tile=32)
    names, lens, ops, args = P.formula_programs(Fm.CALLS[0], V)
    got = []

    @P.SERVICE_FN
    def cb(final, s):
        if s.contents.steps == 25:
            total, planes = (P.pft_fdiag * len(names))(), (P.pft_fdiag * (len(names) * 20))()
            rc = sim.lib.pft_solver_formulas(len(names), P._ip(lens), P._ip(ops), P._dp(args), total, None, planes)
            assert sim.lib.pft_solver_download(s) == 0
            got.append((rc, [t.words() for t in total], [m.words() for m in planes], sim.interior()))
        return 0

    sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
    sim.solve(36.0)
    g = P.pft_grid.from_buffer_copy(sim.grid)
    sim.close()
    assert len(got) == 1
    rc, words, plane_words, x = got[0]
    assert rc == 0 and np.array_equal(x, A["cb_break_state0"])
    _, host, host_planes = Fm.host_formulas(g, D.padded(x), Fm.CALLS[0], variables=V)
    assert words == [h.words() for h in host]
    assert plane_words == [m.words() for row in host_planes for m in row]


def test_two_ranks_refuse_inside_a_service_callback():
    """with two ranks a Service_Callback's pft_solver_formulas returns -2 (another rank's callback
    need not make the same call)"""
    V = _g20_variables()
    names, lens, ops, args = P.formula_programs({"a": "u"}, V)

    def run(sim):
        codes = []

        @P.SERVICE_FN
        def cb(final, s):
            if not codes:
                codes.append(sim.lib.pft_solver_formulas(1, P._ip(lens), P._ip(ops), P._dp(args), (P.pft_fdiag * 1)(),
                                                         None, None))
            return 0

        sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
        sim.solve(36.0)
        return codes

    out = M.loopback_run(2, lambda r: _g20_sim(0, nprocs=2, rank=r), run)
    assert out == [[-2], [-2]]
