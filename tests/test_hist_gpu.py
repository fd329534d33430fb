"""f13 on the GPU: the histogram kernels (pft_slab_hist) against pft_hist_host and against numpy
(tests/_hist.py) by == on integers, on the shapes of tests/test_means_gpu.py -- an odd plane with
misaligned planes, a plane smaller than a wave, several segments per plane, fewer workgroups than
planes -- on states that keep a wave on its aggregated path, states that force the per-lane adds
and a state that holds every edge and its neighbours; pft_solver_hist / Simulation.histogram /
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
import _hist as H
import _means as Mn
import _multi as M
import _oracle as O
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
    """tests/_means.py's bare slab with the f13 entry"""

    def __init__(self, n1, n2, n3):
        super().__init__(n1, n2, n3)
        self.grid = Fm.grid(n1, n2, n3)

    def hist(self, which, formula, edges, mask, per_plane=True):
        names = {"f": formula} if mask is None else {"f": formula, "m": mask}
        c = Fm.Compiled(self.grid, names)
        try:
            assert c.codes == [0] * len(c.names), c.codes
            edges = np.ascontiguousarray(edges, dtype=np.float64)
            nbins = edges.size - 1
            head, counts = P.pft_hist_head(), (C.c_longlong * nbins)()
            ph = (P.pft_hist_head * self.n3)() if per_plane else None
            pc = (C.c_longlong * (self.n3 * nbins))() if per_plane else None
            rc = self.L.pft_slab_hist(self.s, which, C.byref(c.progs[0]), None if mask is None else C.byref(c.progs[1]),
                                      nbins, P._dp(edges), C.byref(head), counts, ph, pc)
            assert rc == 0, (rc, self.L.pft_hip_last_error())
        finally:
            c.free()
        return H.rows_of(head, counts, ph, pc, self.n3, nbins)


def _check_state(slab, tag, make, extra, which=PFT_BUF_X):
    """upload the state (ghost planes poisoned), then for every spec: the device rows == the host
    twin's == numpy's, for the slab and every plane, with and without per_plane"""
    a = make()
    w = D.padded(a)
    slab.upload(which, w)
    sp = H.specs(a) + extra
    want = H.reference(sp, a)
    out = {}
    for name, f, edges, m in sp:
        got = slab.hist(which, f, edges, m)
        H.assert_all(got, H.host_hist(slab.grid, w, f, edges, m), f"{tag} {name}: device against pft_hist_host")
        H.assert_all(got, want[name], f"{tag} {name}: device against numpy")
        alone = slab.hist(which, f, edges, m, per_plane=False)
        assert alone[1] is None
        H.assert_rows(alone[0], want[name][0], f"{tag} {name}: without per_plane")
        out[name] = got[0]
    return out


# the shapes of tests/test_means_gpu.py, for its reasons: (n1, n2, n3, PFT_DIAG_WGS)
SHAPES = [(13, 11, 9, 0), (3, 1, 200, 0), (120, 60, 4, 0), (40, 40, 8, 1), (40, 40, 8, 3), (50, 50, 3, 0)]


@pytest.mark.parametrize("n1,n2,n3,wgs", SHAPES)
def test_slab_hist_equals_host_and_numpy(n1, n2, n3, wgs, monkeypatch):
    if wgs:
        monkeypatch.setenv("PFT_DIAG_WGS", str(wgs))
    cells = n1 * n2 * n3
    slab = Slab(n1, n2, n3)
    try:
        for tag, make, extra in H.states(n1, n2, n3):
            r = _check_state(slab, tag, make, extra)
            assert r["u64"][0]["cells"] == cells
            if tag == "one_bin":
                # every cell in one bin: the aggregated path alone
                assert r["u64"][1].max() == cells and r["u1"][1].tolist() == [cells] and r["p1024"][1][0] == cells
            if tag == "ramp" and cells >= 1024:
                # every lane of a wave in another bin: the per-lane path alone
                c = r["ramp1024"][1]
                assert c.min() >= 1 and c.max() - c.min() <= 1 and c.sum() == cells
    finally:
        slab.close()


def test_no_state_carries_over():
    """1024 bins and then 3 bins give the rows of 3 bins alone; X, then XN holding another state,
    then X again: each call returns its buffer's own rows"""
    slab = Slab(10, 10, 20)
    try:
        a, b = D.random_state(10, 10, 20, 81), H.ramp_state(10, 10, 20)
        slab.upload(PFT_BUF_X, D.padded(a))
        slab.upload(PFT_BUF_XN, D.padded(b))
        three = P.hist_edges([200.0, 270.0, 280.0, 340.0])
        alone = slab.hist(PFT_BUF_X, "u", three, None)
        big = slab.hist(PFT_BUF_X, "p", P.hist_edges(1024, (0.0, 1.0)), H.SUPERCOOLED)
        assert big[0][0]["selected"] > 0
        H.assert_all(slab.hist(PFT_BUF_X, "u", three, None), alone, "3 bins after 1024")
        H.assert_all(alone, H.host_hist(slab.grid, D.padded(a), "u", three, None), "3 bins")
        xa = slab.hist(PFT_BUF_X, *H.RAMP[1:])
        xb = slab.hist(PFT_BUF_XN, *H.RAMP[1:])
        xa2 = slab.hist(PFT_BUF_X, *H.RAMP[1:])
        H.assert_all(xa, H.host_hist(slab.grid, D.padded(a), *H.RAMP[1:]), "X")
        H.assert_all(xb, H.host_hist(slab.grid, D.padded(b), *H.RAMP[1:]), "XN after X")
        H.assert_all(xa2, xa, "X again")
        assert xa[0][1].tolist() != xb[0][1].tolist()
    finally:
        slab.close()


def test_refusals_launch_nothing():
    """a value or mask that is not device-exact answers 1, a bad program or bad edges -2, before
    anything is launched (the outputs stay as they were)"""
    slab = Slab(13, 11, 9)
    try:
        slab.upload(PFT_BUF_X, D.padded(D.random_state(13, 11, 9, 5)))
        e = P.hist_edges(4, (0.0, 400.0))
        head, counts = P.pft_hist_head(), (C.c_longlong * 4)()

        def prog(ops, args):
            ops, args = np.array(ops, dtype=np.int32), np.array(args, dtype=np.float64)
            return P.pft_ic_prog(len(ops), P._ip(ops), P._dp(args), 0, None, None, None, None, 0, 0), (ops, args)

        def call(value, mask=None, nbins=4, edges=e, hd=head):
            v = prog(*value)
            m = None if mask is None else prog(*mask)
            return slab.L.pft_slab_hist(slab.s, PFT_BUF_X, C.byref(v[0]), None if m is None else C.byref(m[0]), nbins,
                                        None if edges is None else P._dp(np.ascontiguousarray(edges, dtype=np.float64)),
                                        None if hd is None else C.byref(hd), counts, None, None)

        u, exp_u, bad = ([101], [6]), ([101, 42], [6, 0]), ([101, 2], [6, 0])
        assert call(u) == 0 and head.cells == 13 * 11 * 9 and head.selected == head.cells
        head.cells = -77                                    # a mark no refused call may touch
        assert call(exp_u) == 1 and call(u, exp_u) == 1     # exp(u) as the value, as the mask
        assert call(([101, 100, 5], [6, 2, 0])) == 1 and call(u, ([101, 100, 7], [6, 2, 0])) == 1      # u C 2; mask u^2
        assert call(([101] * 17 + [2] * 16, [6] * 17 + [0] * 16)) == 1                                  # a stack of 17
        assert call(bad) == -2 and call(u, bad) == -2 and call(([102], [0])) == -2 and call(([101], [5])) == -2
        for edges in H_BAD_EDGES:
            assert call(u, nbins=len(edges) - 1, edges=edges) == -2, edges
        assert call(u, nbins=0) == -2 and call(u, nbins=1025, edges=np.linspace(0.0, 1.0, 1026)) == -2
        assert call(u, edges=None) == -2 and call(u, hd=None) == -2
        assert slab.L.pft_slab_hist(slab.s, 7, C.byref(prog(*u)[0]), None, 4, P._dp(e), C.byref(head), counts, None, None) == -2
        other = Fm.Compiled(Fm.grid(12, 11, 9), {"a": "tanh(x)*u"})     # tables of another grid
        assert other.codes == [0]
        assert slab.L.pft_slab_hist(slab.s, PFT_BUF_X, other.progs, None, 4, P._dp(e), C.byref(head), counts, None, None) == -2
        other.free()
        assert head.cells == -77
        assert call(u) == 0 and head.cells == 13 * 11 * 9
    finally:
        slab.close()


H_BAD_EDGES = [[0.0, 0.0, 1.0], [0.0, -0.0], [-0.0, 0.0], [0.0, np.nan], [0.0, np.inf], [-np.inf, 0.0], [1.0, 0.0]]


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


SERIES = {"temp": {"formula": "u", "bins": 64, "range": (250.0, 300.0)},
          "phase": {"formula": "p", "bins": 1024, "range": (0.0, 1.0)},
          "supercooling": {"formula": "(u-u_star)*(1-gl)", "bins": [-40.0, -10.0, -1.0, 0.0, 1e-3, 5.0, 10.0, 40.0],
                           "mask": "p<0.5 and gl<0.5"},
          "upper": {"formula": "u", "bins": 16, "range": (200.0, 340.0), "mask": "z>L3/2"}}


def _series_specs():
    return [(name, s["formula"], P.hist_edges(s["bins"], s.get("range")), s.get("mask")) for name, s in SERIES.items()]


def _assert_row(row, want, what):
    for name, (head, counts) in want.items():
        assert row[name].dtype == np.int64 and (row[name] == counts).all(), f"{what} {name}"
        assert all(row[name + "_" + k] == head[k] for k in P.HIST_ROW_KEYS), f"{what} {name}"


@pytest.mark.parametrize("pair", [0, 2])
def test_run_series_histograms_on_golden(pair, tmp_path):
    """the driver's loop on golden g20 to t = 36 s with histograms=, with one launch per stage and
    with the pair kernels: every other row key is that of a run without histograms, the counts are
    numpy's on the golden states; Simulation.histogram on one slab, device against host route; -3 and
    RuntimeError without a resident state; the not device-exact formulas raise"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _g20_sim(0)
        (vops, vargs), _ = H.programs("u", None, V)
        e = P.hist_edges(4, (0.0, 400.0))
        assert P.lib().pft_solver_hist(1, P._ip(vops), P._dp(vargs), 0, None, None, 4, P._dp(e), C.byref(P.pft_hist_head()),
                                       (C.c_longlong * 4)(), None, None, None, None) == -3
        with pytest.raises(RuntimeError, match="resident"):
            sim.histogram("u", 4, (0.0, 400.0))
        rows = sim.run_series(times=meta["traj_times"][:1], histograms=SERIES, variables=V)
        pairs = sim.stats().pairs
        dev = {n: sim.histogram(s["formula"], s["bins"], s.get("range"), mask=s.get("mask"), variables=V, per_plane=True)
               for n, s in SERIES.items()}
        flat = sim.histogram("u", 64, (250.0, 300.0))
        with pytest.raises(ValueError, match="'exp\\(u-u_star\\)'.*not device-exact"):
            sim.histogram("exp(u-u_star)", 4, (0.0, 1.0), variables=V)
        with pytest.raises(ValueError, match="'u C 2'.*not device-exact"):
            sim.histogram("u", 4, (0.0, 1.0), mask="u C 2", variables=V)
        sim.download()
        host = {n: sim.histogram(s["formula"], s["bins"], s.get("range"), mask=s.get("mask"), variables=V, where="host",
                                 per_plane=True) for n, s in SERIES.items()}
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
    new = {k for n in SERIES for k in [n] + [n + "_" + s for s in P.HIST_ROW_KEYS]}
    for r, q in zip(rows, plain):
        assert all(r[k] == q[k] for k in q)
        assert set(r) == set(q) | new
    sp = _series_specs()
    want0 = H.reference(sp, A["traj_m0_ic"], variables=V)
    want1 = H.reference(sp, x, variables=V)
    _assert_row(rows[0], {n: w[0] for n, w in want0.items()}, "snapshot 0 (the host IC)")
    _assert_row(rows[1], {n: w[0] for n, w in want1.items()}, "snapshot 1")
    for name in SERIES:
        H.assert_rows(H.as_rows(dev[name]), want1[name][0], f"{name}: device against numpy")
        H.assert_rows(H.as_rows(host[name]), want1[name][0], f"{name}: host route against numpy")
        for (hd, c), (gh, gc), (hh, hc) in zip(want1[name][1], H.planes_of(dev[name]), H.planes_of(host[name])):
            assert (gc == c).all() and (hc == c).all()
            assert all(gh[k] == hd[k] == hh[k] for k in P.HIST_ROW_KEYS)
        assert dev[name]["first_row"] == 0 and H.as_rows(dev[name]["local"])[0] == H.as_rows(dev[name])[0]
        assert (dev[name]["edges"] == sp[[s[0] for s in sp].index(name)][2]).all()
    assert (flat["counts"] == dev["temp"]["counts"]).all() and "counts_per_plane" not in flat
    assert rows[1]["temp"].sum() + rows[1]["temp_under"] + rows[1]["temp_over"] == rows[1]["cells"]
    path = tmp_path / "temp.txt"
    P.write_hist_txt(rows, str(path), "temp")
    assert path.read_text() == "".join(" ".join(str(int(c)) for c in r["temp"]) + "\n" for r in rows)
    lo, hi = P.hist_quantile(dev["temp"], 0.5)
    med = np.sort(x[0].ravel())[(x[0].size + 1) // 2 - 1]           # the ceil(N / 2)-th smallest
    assert lo <= med <= hi


def test_case_run_histograms_with_a_params_variable():
    """Case.run(histograms=) compiles with the case's own evaluator: a variable of the parameter
    file appears in a formula, in a mask and nowhere else; an undefined one ends the run before any
    work"""
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    lines = [f"{k} {v!r}" for k, v in zip(P.PARAM_NAMES, (float(x) for x in Pm))]
    lines += [f"L1 {info['L1']!r}", f"L2 {info['L2']!r}", f"L3 {info['L3']!r}", f"n1 {info['n1']}", f"n2 {info['n2']}",
              f"n3 {info['n3']}", "saved_files 2", "tau 1", "final_time 36", f"delta {info['delta']!r}",
              f"tau_min {info['tau_min']!r}", "my_threshold u_star + 1",
              'icond u = "u_star + 5*_z"', 'icond p = "_z < 0.3"', 'icond gl = "0"']
    case = FE.load_params(text="\n".join(lines) + "\n")
    with pytest.raises(FE.EvalError, match="nope"):
        case.run(histograms={"a": {"formula": "u - nope", "bins": 4, "range": (0.0, 1.0)}})
    with pytest.raises(ValueError):
        case.run(histograms={"a": {"formula": "u", "bins": [1.0, 1.0]}})
    rows = case.run(histograms={"warm": {"formula": "u - my_threshold", "bins": 8, "range": (-1.0, 4.0),
                                         "mask": "u > my_threshold"}}, tile=2)
    thr = case.ev.value("my_threshold")
    sim = case.simulation(tile=2)
    try:
        ic = sim.interior()
    finally:
        sim.close()
    assert [r["snapshot"] for r in rows] == [0, 1]
    sel = ic[0] > thr
    want = H.np_rows(ic[0] - thr, sel, np.linspace(-1.0, 4.0, 9))
    assert (rows[0]["warm"] == want[1]).all() and rows[0]["warm_selected"] == want[0]["selected"] == int(sel.sum()) > 0
    assert rows[0]["warm_under"] == 0 and rows[0]["warm"].sum() == rows[0]["warm_selected"]
    assert 0 < rows[1]["warm_selected"] < ic[0].size


@pytest.mark.parametrize("case", ["7x5x7", "g20", "ragged"])
def test_loopback_slabs_equal_one_slab(case, tmp_path):
    """3 loopback slabs (7x5x7: slabs of 3 / 2 / 2 planes of 35 cells, the state read from a dataset
    and counted as it stands; g20: 7 / 6 / 7 rows; the ragged fixture, 18x12x30): every rank's global
    rows are the single slab's and its planes' rows side by side are the single slab's planes'.  On
    7x5x7 both also equal pft_hist_host and numpy of the whole state"""
    import _snap as S
    small = None
    if case == "7x5x7":
        T = None                                       # no solve: the state of the dataset itself
        Pm = O.params_from_meta(O.load_case("g20")[0])[0]
        V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
        V.update(L1=Fm.L[0], L2=Fm.L[1], L3=Fm.L[2])
        info = {"n3": 7}
        small = H.edges_state(7, 5, 7)
        small[2] = np.abs(small[2])
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

    series = dict(SERIES, uedges={"formula": "u", "bins": H.IRREGULAR})

    def run(sim):
        rows = sim.run_series(times=[] if T is None else [T], histograms={"upper": SERIES["upper"]}, variables=V)
        out = {}
        for n, s in series.items():
            d = sim.histogram(s["formula"], s["bins"], s.get("range"), mask=s.get("mask"), variables=V, per_plane=True)
            out[n] = (H.as_rows(d), H.planes_of(d), d["first_row"], d["local"]["cells"])
        return rows, out

    def plain(rows_pair):
        return [list(rows_pair[0].values()), rows_pair[1].tolist()]

    one = make(1, 0)
    rows1, out1 = run(one)
    one.close()
    assert 0 < out1["upper"][0][0]["selected"] < out1["upper"][0][0]["cells"]
    if small is not None:
        w = D.padded(small)
        sp = [(n, s["formula"], P.hist_edges(s["bins"], s.get("range")), s.get("mask")) for n, s in series.items()]
        want = H.reference(sp, small, variables=V)
        for name, f, edges, m in sp:
            host = H.host_hist(Fm.grid(7, 5, 7), w, f, edges, m, variables=V)
            H.assert_all(host, want[name], f"{name}: host twin against numpy")
            H.assert_rows(out1[name][0], want[name][0], f"{name}: one slab against numpy")
            for (gh, gc), (hd, c) in zip(out1[name][1], want[name][1]):
                assert (gc == c).all() and all(gh[k] == hd[k] for k in P.HIST_ROW_KEYS), name
    res = M.loopback_run(3, lambda r: make(3, r), run)
    for rows, out in res:
        for a, b in zip(rows, rows1):
            assert set(a) == set(b)
            assert all((a[k] == b[k]).all() if isinstance(a[k], np.ndarray) else Mn.same(a[k], b[k]) for k in a)
        for name in series:
            assert plain(out[name][0]) == plain(out1[name][0]), name
    for name in series:
        side = sum((out[name][1] for _, out in res), [])
        assert [[list(h.values()), c.tolist()] for h, c in side] == [[list(h.values()), c.tolist()] for h, c in out1[name][1]]
        assert [out[name][2] for _, out in res] == [P.decompose(info["n3"], 3, r)[1] for r in range(3)]
        assert sum(out[name][3] for _, out in res) == out1[name][0][0]["cells"]


def test_two_ipc_processes(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_hist_worker.py): both ranks report the golden
    state's global rows, their planes' rows side by side are the whole grid's; edges that differ
    between the two ranks answer -2 on both, a formula that is not device-exact raises on both, and
    the next call works"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    hist = {"formula": "(u-u_star)*(1-gl)", "bins": 1024, "range": [-40.0, 40.0], "mask": "p<0.5 and gl<0.5"}
    spec = {"nranks": 2, "shm": f"/pft_hist_{os.getpid()}_{uuid.uuid4().hex[:12]}", "out": str(tmp_path / "rank"),
            "times": [meta["traj_times"][0]], "hist": hist, "variables": V}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_hist_worker.py"), str(path), str(r)], env=env,
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
    edges = P.hist_edges(1024, (-40.0, 40.0))
    sp = [("h", hist["formula"], edges, hist["mask"])]
    (head, counts), planes = H.reference(sp, a, variables=V)["h"]
    head0, counts0 = H.reference(sp, A["traj_m0_ic"], variables=V)["h"][0]
    assert head["selected"] > 0
    assert [r["hist"]["first_row"] for r in res] == [0, 10]
    assert [r["differ"] for r in res] == [-2, -2] and [r["not_exact"] for r in res] == ["ValueError"] * 2
    for r in res:
        for got in (r["hist"], r["after"]):
            assert got["counts"] == counts.tolist() and all(got[k] == head[k] for k in H.HEAD_KEYS)
        for row, (hd, c) in zip(r["rows"], ((head0, counts0), (head, counts))):       # the host IC, then the device
            assert row["sc"] == c.tolist() and all(row["sc_" + k] == hd[k] for k in P.HIST_ROW_KEYS)
    side = res[0]["hist"]["counts_per_plane"] + res[1]["hist"]["counts_per_plane"]
    assert side == [c.tolist() for _, c in planes]
    for k in P.HIST_ROW_KEYS:
        assert res[0]["hist"][k + "_per_plane"] + res[1]["hist"][k + "_per_plane"] == [h[k] for h, _ in planes]
    assert res[0]["local"]["cells"] + res[1]["local"]["cells"] == 2000


def test_hist_inside_a_service_callback():
    """at the 25th accepted step on one rank: pft_solver_hist returns 0 and describes the state
    pft_solver_download gives in the same callback (tests/golden/ctl cb_break_state0)"""
    _, A = O.load_case("ctl")
    V = _g20_variables()
    sim = _g20_sim(0, tile=32)
    (vops, vargs), (mops, margs) = H.programs("u", "p<0.5 and gl<0.5", V)
    edges = P.hist_edges(64, (250.0, 300.0))
    got = []

    @P.SERVICE_FN
    def cb(final, s):
        if s.contents.steps == 25:
            head, counts = P.pft_hist_head(), (C.c_longlong * 64)()
            ph, pc = (P.pft_hist_head * 20)(), (C.c_longlong * (20 * 64))()
            rc = sim.lib.pft_solver_hist(len(vops), P._ip(vops), P._dp(vargs), len(mops), P._ip(mops), P._dp(margs), 64,
                                         P._dp(edges), C.byref(head), counts, None, None, ph, pc)
            assert sim.lib.pft_solver_download(s) == 0
            got.append((rc, H.rows_of(head, counts, ph, pc, 20, 64), sim.interior()))
        return 0

    sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
    sim.solve(36.0)
    g = P.pft_grid.from_buffer_copy(sim.grid)
    sim.close()
    assert len(got) == 1
    rc, rows, x = got[0]
    assert rc == 0 and np.array_equal(x, A["cb_break_state0"])
    H.assert_all(rows, H.host_hist(g, D.padded(x), "u", edges, "p<0.5 and gl<0.5", variables=V), "in the callback")
    H.assert_all(rows, H.reference([("h", "u", edges, "p<0.5 and gl<0.5")], x, variables=V)["h"], "against numpy")


def test_two_ranks_refuse_inside_a_service_callback():
    """with two ranks a Service_Callback's pft_solver_hist returns -2 (another rank's callback need
    not make the same call)"""
    V = _g20_variables()
    (vops, vargs), _ = H.programs("u", None, V)
    edges = P.hist_edges(4, (0.0, 400.0))

    def run(sim):
        codes = []

        @P.SERVICE_FN
        def cb(final, s):
            if not codes:
                codes.append(sim.lib.pft_solver_hist(len(vops), P._ip(vops), P._dp(vargs), 0, None, None, 4, P._dp(edges),
                                                     C.byref(P.pft_hist_head()), (C.c_longlong * 4)(), None, None, None, None))
            return 0

        sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
        sim.solve(36.0)
        return codes

    out = M.loopback_run(2, lambda r: _g20_sim(0, nprocs=2, rank=r), run)
    assert out == [[-2], [-2]]
