"""f15 on the GPU: the map kernel (pft_slab_map) against pft_map_host and against numpy (tests/_map.py)
by == on integers and on the bits of the doubles, for every axis -- on shapes with an odd row and an
odd plane (the 8-byte loads, the alignment alternating with k), rows shorter and longer than a
wave's window, lines cut into sub-chunks and into chunks of several workgroups, fewer workgroups than
items; a first / last sweep; pft_solver_map / Simulation.project / run_series / Case.run on one slab,
on loopback slabs, in two ipc processes and from a Service_Callback."""
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
import _map as Mp
import _means as Mn
import _multi as M
import _oracle as O
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PFT_BUF_X, PFT_BUF_XN = 0, 1
AXES = (0, 1, 2)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


class Slab(Mn.Slab):
    """tests/_means.py's bare slab with the f15 entry"""

    def __init__(self, n1, n2, n3):
        super().__init__(n1, n2, n3)
        self.grid = Fm.grid(n1, n2, n3)

    def map(self, which, formula, mask, axis):
        names = {"f": formula} if mask is None else {"f": formula, "m": mask}
        c = Fm.Compiled(self.grid, names)
        try:
            assert c.codes == [0] * len(c.names), c.codes
            rows, cols = Mp.dims(self.grid, axis)
            out = np.empty(rows * cols, dtype=P.MAP_DTYPE)
            rc = self.L.pft_slab_map(self.s, which, C.byref(c.progs[0]), None if mask is None else C.byref(c.progs[1]), axis,
                                     P._map_ptr(out))
            assert rc == 0, (rc, self.L.pft_hip_last_error())
        finally:
            c.free()
        return Mp.as_dict(out, cols)


# (n1, n2, n3, PFT_DIAG_WGS).  The issue's shapes, and two of this file's for the cut of a line into
# chunks of several workgroups, which a thread's floor of 16 cells keeps the others from: (40, 6, 70)
# along z (120 pairs: 128 x 2 threads, chunks of 32 planes), (130, 70, 2) along y (65 pairs: 128 x 2
# threads, chunks of 32 rows)
SHAPES = [(13, 11, 9, 0), (3, 1, 200, 0), (1, 7, 5, 0), (120, 60, 4, 0), (50, 50, 3, 0), (33, 31, 9, 0),
          (40, 40, 8, 1), (40, 40, 8, 3), (40, 6, 70, 0), (130, 70, 2, 0)]


@pytest.mark.parametrize("n1,n2,n3,wgs", SHAPES)
def test_slab_map_equals_host_and_numpy(n1, n2, n3, wgs, monkeypatch):
    """device == host twin == numpy on bit patterns, a dense state and a random one, for every axis,
    from X and from XN; with PFT_DIAG_WGS (read when the slab is made) one or three workgroups take
    every item in turn"""
    if wgs:
        monkeypatch.setenv("PFT_DIAG_WGS", str(wgs))
    slab = Slab(n1, n2, n3)
    try:
        for q, (tag, make) in enumerate(Mp.states(n1, n2, n3)):
            a = make()
            w = D.padded(a)
            which = PFT_BUF_XN if q == 1 else PFT_BUF_X
            slab.upload(which, w)
            for name, f, m in Mp.SPECS + (Mp.COORD_SPECS if tag == "random" else []):
                for axis in AXES:
                    what = f"{tag} {name} axis {axis}"
                    got = slab.map(which, f, m, axis)
                    Mp.assert_map(got, Mp.host_map(slab.grid, w, f, m, axis), what + ": device against pft_map_host")
                    if (name, f, m) in Mp.SPECS or n1 * n2 * n3 <= 1500:
                        Mp.assert_map(got, Mp.reference(f, m, a, axis), what + ": device against numpy")
    finally:
        slab.close()


@pytest.mark.parametrize("axis", AXES)
def test_first_last_sweep(axis):
    """one non-zero cell moved through every position of a line at (13, 11, 9): first == last == its
    position at that pixel and -1 at every other; then two cells: first and last apart"""
    n1, n2, n3 = 13, 11, 9
    slab = Slab(n1, n2, n3)
    try:
        length = (n3, n2, n1)[axis]
        line = [(4, 6), (5, 7), (3, 8)][axis]            # the pixel (row, column) of the map
        for pos in list(range(length)) + [None]:
            a = np.zeros((3, n3, n2, n1))
            v = np.moveaxis(a[0], axis, 0)
            if pos is None:
                v[1][line], v[length - 2][line] = -2.5, np.nan
                want = (1, length - 2)
            else:
                v[pos][line] = 7.0
                want = (pos, pos)
            slab.upload(PFT_BUF_X, D.padded(a))
            got = slab.map(PFT_BUF_X, "u", None, axis)
            assert (got["first"][line], got["last"][line]) == want, pos
            rest = np.ones(got["first"].shape, dtype=bool)
            rest[line] = False
            assert (got["first"][rest] == -1).all() and (got["last"][rest] == -1).all() and not got["nonzero"][rest].any()
            assert got["nonzero"][line] == (1 if pos is not None else 2) and (got["selected"] == length).all()
            Mp.assert_map(got, Mp.reference("u", None, a, axis), f"pos {pos}")
    finally:
        slab.close()


def test_no_state_carries_over():
    """two different formulas in turn, then the first again; another axis and another buffer between"""
    slab = Slab(10, 10, 20)
    try:
        a, b = D.random_state(10, 10, 20, 81), Mp.dense_state(10, 10, 20, 82)
        slab.upload(PFT_BUF_X, D.padded(a))
        slab.upload(PFT_BUF_XN, D.padded(b))
        first = slab.map(PFT_BUF_X, "u", Mp.ICE, 0)
        other = slab.map(PFT_BUF_X, Mp.ICE, None, 0)
        Mp.assert_map(slab.map(PFT_BUF_X, "u", Mp.ICE, 0), first, "the first again")
        Mp.assert_map(first, Mp.reference("u", Mp.ICE, a, 0), "the first")
        Mp.assert_map(other, Mp.reference(Mp.ICE, None, a, 0), "the second")
        for axis in (2, 1, 0):
            Mp.assert_map(slab.map(PFT_BUF_XN, "u", Mp.ICE, axis), Mp.reference("u", Mp.ICE, b, axis), f"XN, axis {axis}")
            Mp.assert_map(slab.map(PFT_BUF_X, "u", Mp.ICE, axis), Mp.reference("u", Mp.ICE, a, axis), f"X, axis {axis}")
    finally:
        slab.close()


def test_refusals_launch_nothing():
    """a value or mask that is not device-exact answers 1, a bad program, axis or buffer -2, before
    anything is launched (the output stays as it was)"""
    slab = Slab(13, 11, 9)
    try:
        slab.upload(PFT_BUF_X, D.padded(D.random_state(13, 11, 9, 5)))
        out = np.zeros(13 * 11, dtype=P.MAP_DTYPE)

        def prog(ops, args):
            ops, args = np.array(ops, dtype=np.int32), np.array(args, dtype=np.float64)
            return P.pft_ic_prog(len(ops), P._ip(ops), P._dp(args), 0, None, None, None, None, 0, 0), (ops, args)

        def call(value, mask=None, axis=0, o=out, buf=PFT_BUF_X):
            v = prog(*value)
            m = None if mask is None else prog(*mask)
            return slab.L.pft_slab_map(slab.s, buf, C.byref(v[0]), None if m is None else C.byref(m[0]), axis,
                                       None if o is None else P._map_ptr(o))

        u, exp_u, bad = ([101], [6]), ([101, 42], [6, 0]), ([101, 2], [6, 0])
        assert call(u) == 0 and (out["selected"] == 9).all()
        out["selected"] = -77                               # a mark no refused call may touch
        assert call(exp_u) == 1 and call(u, exp_u) == 1     # exp(u), a libm function, as the value, as the mask
        assert call(([101, 100, 5], [6, 2, 0])) == 1 and call(u, ([101, 100, 7], [6, 2, 0])) == 1      # u C 2; mask u^2 (pow)
        assert call(([101, 100, 7], [6, 2, 0])) == 1                                                    # u^2 as the value
        assert call(([101] * 17 + [2] * 16, [6] * 17 + [0] * 16)) == 1                                  # a stack of 17
        assert call(bad) == -2 and call(u, bad) == -2 and call(([102], [0])) == -2 and call(([101], [5])) == -2
        assert call(u, axis=3) == -2 and call(u, axis=-1) == -2 and call(u, o=None) == -2 and call(u, buf=7) == -2
        other = Fm.Compiled(Fm.grid(12, 11, 9), {"a": "tanh(x)*u"})     # tables of another grid
        assert other.codes == [0]
        assert slab.L.pft_slab_map(slab.s, PFT_BUF_X, other.progs, None, 0, P._map_ptr(out)) == -2
        other.free()
        assert (out["selected"] == -77).all()
        assert call(u, axis=2) == 0 and (out["selected"][:9 * 11] == 13).all()
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


SERIES = {"front": {"formula": "p>0.5", "axis": 0},
          "warm_y": {"formula": "u", "axis": 1, "mask": "p>0.5"},
          "cold_x": {"formula": "u_star-u", "axis": 2, "mask": "p<0.5 and gl<0.5"}}


def _want(a, V, series=SERIES):
    return {n: Mp.reference(s["formula"], s.get("mask"), a, s["axis"], variables=V) for n, s in series.items()}


def _arrays(d):
    return {k: np.asarray(d[k], dtype=np.float64 if k in ("min", "max") else np.int64) for k in Mp.KEYS}


@pytest.mark.parametrize("pair", [0, 2])
def test_run_series_maps_on_golden(pair, tmp_path):
    """the driver's loop on golden g20 to t = 36 s with maps=, with one launch per stage and with the
    pair kernels: every other row key is that of a run without maps, the maps are numpy's and the host
    twin's on the golden states and are written beside the snapshots; -3 and RuntimeError without a
    resident state; the not device-exact formulas raise"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, pair)
    try:
        sim = _g20_sim(0)
        (vops, vargs), _ = Mp.programs("u", None, V)
        local = np.empty(10 * 10, dtype=P.MAP_DTYPE)
        assert P.lib().pft_solver_map(1, P._ip(vops), P._dp(vargs), 0, None, None, 0, None, P._map_ptr(local)) == -3
        with pytest.raises(RuntimeError, match="resident"):
            sim.project("u", 0)
        rows = sim.run_series(times=meta["traj_times"][:1], maps=SERIES, variables=V, snapshot_path=str(tmp_path / "s"))
        pairs = sim.stats().pairs
        dev = {n: sim.project(s["formula"], s["axis"], mask=s.get("mask"), variables=V) for n, s in SERIES.items()}
        with pytest.raises(ValueError, match="'exp\\(u-u_star\\)'.*not device-exact"):
            sim.project("exp(u-u_star)", 0, variables=V)
        with pytest.raises(ValueError, match="'u\\^2'.*not device-exact"):
            sim.project("u", 1, mask="u^2", variables=V)
        assert P.lib().pft_solver_map(1, P._ip(vops), P._dp(vargs), 0, None, None, 3, None, P._map_ptr(local)) == -2
        sim.download()
        host = {n: sim.project(s["formula"], s["axis"], mask=s.get("mask"), variables=V, where="host") for n, s in SERIES.items()}
        x = sim.interior()
        sim.close()
        sim = _g20_sim(0)
        plain = sim.run_series(times=meta["traj_times"][:1], snapshot_path=str(tmp_path / "p"))
        sim.close()
    finally:
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
    assert pairs == (1 if pair else 0)
    assert np.array_equal(x, A["traj_m0_state0"])
    assert [r["snapshot"] for r in rows] == [0, 1] and rows[1]["t"] == 36.0
    for r, q in zip(rows, plain):
        assert all(r[k] == q[k] for k in q)
        assert set(r) == set(q) | set(SERIES)
    want0, want1 = _want(A["traj_m0_ic"], V), _want(x, V)
    for name, s in SERIES.items():
        Mp.assert_map(rows[0][name], want0[name], f"snapshot 0 (the host IC) {name}")
        Mp.assert_map(rows[1][name], want1[name], f"snapshot 1 {name}")
        Mp.assert_map(dev[name], want1[name], f"{name}: device against numpy")
        Mp.assert_map(host[name], want1[name], f"{name}: host route against numpy")
        assert dev[name]["axis"] == s["axis"] and dev[name]["rows"] == (0, 20)
        for snap in (0, 1):
            f = np.load(str(tmp_path / f"s.{name}.{snap:03d}.npz"))
            Mp.assert_map(f, rows[snap][name], f"{name}: the file of snapshot {snap}")
            assert int(f["axis"]) == s["axis"] and f["rows"].tolist() == [0, 20]
    assert rows[1]["front"]["nonzero"].sum() == rows[1]["ice"]          # the ice thickness sums to f5's ice count
    every = _g20_sim(0)
    try:
        skipped = every.run_series(times=meta["traj_times"][:1], maps={"front": SERIES["front"]}, variables=V, map_every=2)
    finally:
        every.close()
    assert "front" in skipped[0] and "front" not in skipped[1]


def test_case_run_maps_with_a_params_variable():
    """Case.run(maps=) compiles with the case's own evaluator: a variable of the parameter file appears
    in a formula and in a mask; an undefined one ends the run before any work"""
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    lines = [f"{k} {v!r}" for k, v in zip(P.PARAM_NAMES, (float(x) for x in Pm))]
    lines += [f"L1 {info['L1']!r}", f"L2 {info['L2']!r}", f"L3 {info['L3']!r}", f"n1 {info['n1']}", f"n2 {info['n2']}",
              f"n3 {info['n3']}", "saved_files 2", "tau 1", "final_time 36", f"delta {info['delta']!r}",
              f"tau_min {info['tau_min']!r}", "my_threshold u_star + 1",
              'icond u = "u_star + 5*_z"', 'icond p = "_z < 0.3"', 'icond gl = "0"']
    case = FE.load_params(text="\n".join(lines) + "\n")
    with pytest.raises(FE.EvalError, match="nope"):
        case.run(maps={"a": {"formula": "u - nope", "axis": 0}})
    with pytest.raises(ValueError, match="axis"):
        case.run(maps={"a": {"formula": "u", "axis": 5}})
    rows = case.run(maps={"warm": {"formula": "u - my_threshold", "axis": 0, "mask": "u > my_threshold"}}, tile=2)
    thr = case.ev.value("my_threshold")
    sim = case.simulation(tile=2)
    try:
        ic = sim.interior()
    finally:
        sim.close()
    assert [r["snapshot"] for r in rows] == [0, 1]
    Mp.assert_map(rows[0]["warm"], Mp.np_map(ic[0] - thr, ic[0] > thr, 0), "snapshot 0")
    assert 0 < int(rows[1]["warm"]["selected"].sum()) < ic[0].size


@pytest.mark.parametrize("case", ["7x5x7", "g20", "ragged"])
def test_loopback_slabs_equal_one_slab(case, tmp_path):
    """3 loopback slabs (7x5x7: slabs of 3 / 2 / 2 planes, the state read from a dataset and mapped as
    it stands; g20: 7 / 6 / 7 rows; the ragged fixture, 18x12x30): every rank's global map is the
    single slab's for every axis, and the ranks' shares are its rows (axes 1, 2) or combine to it (0).
    On 7x5x7 both also equal pft_map_host and numpy of the whole state"""
    import _snap as S
    small = None
    if case == "7x5x7":
        T = None                                       # no solve: the state of the dataset itself
        Pm = O.params_from_meta(O.load_case("g20")[0])[0]
        V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
        V.update(L1=Fm.L[0], L2=Fm.L[1], L3=Fm.L[2])
        n3 = 7
        small = Mp.pattern_state(7, 5, 7, 33)
        small[2] = np.abs(np.nan_to_num(small[2], nan=0.5, posinf=1.0, neginf=0.0))
        first = str(tmp_path / "first.ncd")
        inf = P.snapshot_info(36.0, 0.5, 72.0, 1e-3, 0, snapshot=3, total_snapshots=9, comment="slabs")
        S.write_host(first, Fm.grid(7, 5, 7), Pm, inf, D.padded(small, poison=False))

        def make(nprocs, rank):
            return P.Simulation(7, 5, 7, Fm.L, 0, Pm, nprocs=nprocs, rank=rank, icond_file=first)
    elif case == "g20":
        T, V, n3 = 36.0, _g20_variables(), 20

        def make(nprocs, rank):
            return _g20_sim(0, nprocs=nprocs, rank=rank)
    else:
        meta, A = O.load_case("ragged")
        Pm, info = O.params_from_meta(meta)
        V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
        V.update(L1=info["L1"], L2=info["L2"], L3=info["L3"])
        state = A["state"].copy()
        state[1, 8:19, 3:9, 4:11] = 1.0
        T, n3 = meta["step_large"]["T"], info["n3"]

        def make(nprocs, rank):
            return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                                nprocs=nprocs, rank=rank, initial=state, tau=meta["step_large"]["h0"],
                                tau_min=info["tau_min"], delta=info["delta"], t0=meta["step_large"]["t0"], tile=2)

    series = {f"{n}{axis}": dict(s, axis=axis) for n, s in SERIES.items() for axis in AXES}
    series["upper1"] = {"formula": "u", "axis": 1, "mask": "z>L3/2"}

    def run(sim):
        rows = sim.run_series(times=[] if T is None else [T], maps={"front": SERIES["front"]}, variables=V)
        both = {n: sim.project(s["formula"], s["axis"], mask=s.get("mask"), variables=V) for n, s in series.items()}
        share = {n: sim.project(s["formula"], s["axis"], mask=s.get("mask"), variables=V, combine=False)
                 for n, s in series.items()}
        return rows, both, share

    one = make(1, 0)
    rows1, both1, share1 = run(one)
    one.close()
    assert 0 < int(both1["upper1"]["selected"].sum()) < both1["upper1"]["selected"].size * both1["upper1"]["selected"].max()
    if small is not None:
        w = D.padded(small)
        for n, s in series.items():
            host = Mp.host_map(Fm.grid(7, 5, 7), w, s["formula"], s.get("mask"), s["axis"], variables=V)
            want = Mp.reference(s["formula"], s.get("mask"), small, s["axis"], variables=V)
            Mp.assert_map(host, want, f"{n}: host twin against numpy")
            Mp.assert_map(both1[n], want, f"{n}: one slab against numpy")
    res = M.loopback_run(3, lambda r: make(3, r), run)
    places = [P.decompose(n3, 3, r) for r in range(3)]
    for r, (rows, both, share) in enumerate(res):
        for a, b in zip(rows, rows1):
            assert set(a) == set(b)
            Mp.assert_map(a["front"], b["front"], f"rank {r}: run_series")
        for n, s in series.items():
            Mp.assert_map(both[n], both1[n], f"rank {r} {n}: global")
            assert both[n]["rows"] == (0, n3) and share[n]["rows"] == (places[r][1], places[r][0])
    neutral = P.pft_map_px()
    P.lib().pft_map_init(C.byref(neutral))
    for n, s in series.items():
        if s["axis"]:
            for k in Mp.KEYS:
                side = np.concatenate([share[n][k] for _, _, share in res])
                assert np.array_equal(side.view(np.int64), both1[n][k].view(np.int64)), (n, k)
            continue
        acc = None
        for _, _, share in res[::-1]:
            rec = np.zeros(share[n]["selected"].size, dtype=P.MAP_DTYPE)
            for k in Mp.KEYS:
                rec[k] = share[n][k].ravel()
            if acc is None:
                acc = rec
            else:
                assert P.lib().pft_map_combine(acc.size, P._map_ptr(acc), P._map_ptr(rec)) == 0
        Mp.assert_map(Mp.as_dict(acc, both1[n]["selected"].shape[1]), both1[n], f"{n}: the shares combined")


def test_two_ipc_processes(tmp_path):
    """2 processes over the ipc transport (tests/_ipc_map_worker.py): both ranks report the golden
    state's global maps for every axis, their shares are its rows or combine to it; an axis that
    differs between the two ranks answers -2 on both, a formula that is not device-exact raises on
    both, and the next call works"""
    meta, A = O.load_case("g20")
    V = _g20_variables()
    spec = {"nranks": 2, "shm": f"/pft_map_{os.getpid()}_{uuid.uuid4().hex[:12]}", "out": str(tmp_path / "rank"),
            "times": [meta["traj_times"][0]], "maps": SERIES, "variables": V}
    path = tmp_path / "spec.json"
    path.write_text(json.dumps(spec))
    env = dict(os.environ, PFT_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ipc_map_worker.py"), str(path), str(r)], env=env,
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
    want0, want1 = _want(A["traj_m0_ic"], V), _want(A["traj_m0_state0"], V)
    assert [r["differ"] for r in res] == [-2, -2] and [r["not_exact"] for r in res] == ["ValueError"] * 2
    print("wall time of the combined calls, seconds:", [r["wall"] for r in res])
    for q, r in enumerate(res):
        for name in SERIES:
            Mp.assert_map(_arrays(r["rows"][0][name]), want0[name], f"rank {q} {name}: snapshot 0 (the host IC)")
            Mp.assert_map(_arrays(r["rows"][1][name]), want1[name], f"rank {q} {name}: snapshot 1")
            Mp.assert_map(_arrays(r["both"][name]), want1[name], f"rank {q} {name}: global")
            assert r["both"][name]["rows"] == [0, 20] and r["share"][name]["rows"] == [10 * q, 10]
        Mp.assert_map(_arrays(r["after"]), want1["front"], f"rank {q}: after the refusals")
    for name, s in SERIES.items():
        if s["axis"]:
            for k in Mp.KEYS:
                side = np.concatenate([_arrays(r["share"][name])[k] for r in res])
                assert np.array_equal(side.view(np.int64), np.ascontiguousarray(want1[name][k]).view(np.int64)), (name, k)
        else:
            recs = []
            for r in res:
                d = _arrays(r["share"][name])
                rec = np.zeros(d["selected"].size, dtype=P.MAP_DTYPE)
                for k in Mp.KEYS:
                    rec[k] = d[k].ravel()
                recs.append(rec)
            assert P.lib().pft_map_combine(recs[0].size, P._map_ptr(recs[0]), P._map_ptr(recs[1])) == 0
            Mp.assert_map(Mp.as_dict(recs[0], 10), want1[name], f"{name}: the shares combined")


def test_map_inside_a_service_callback():
    """at the 25th accepted step on one rank: pft_solver_map returns 0 and describes the state
    pft_solver_download gives in the same callback (tests/golden/ctl cb_break_state0)"""
    _, A = O.load_case("ctl")
    V = _g20_variables()
    sim = _g20_sim(0, tile=32)
    (vops, vargs), (mops, margs) = Mp.programs("u", "p<0.5 and gl<0.5", V)
    got = []

    @P.SERVICE_FN
    def cb(final, s):
        if s.contents.steps == 25:
            for axis in AXES:
                rows, cols = [(10, 10), (20, 10), (20, 10)][axis]
                local, glob = np.empty(rows * cols, dtype=P.MAP_DTYPE), np.empty(rows * cols, dtype=P.MAP_DTYPE)
                rc = sim.lib.pft_solver_map(len(vops), P._ip(vops), P._dp(vargs), len(mops), P._ip(mops), P._dp(margs), axis,
                                            P._map_ptr(glob), P._map_ptr(local))
                got.append((axis, rc, Mp.as_dict(local, cols), Mp.as_dict(glob, cols)))
            assert sim.lib.pft_solver_download(s) == 0
            got.append(sim.interior())
        return 0

    sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
    sim.solve(36.0)
    g = P.pft_grid.from_buffer_copy(sim.grid)
    sim.close()
    assert len(got) == 4
    x = got[3]
    assert np.array_equal(x, A["cb_break_state0"])
    for axis, rc, local, glob in got[:3]:
        assert rc == 0
        Mp.assert_map(local, Mp.host_map(g, D.padded(x), "u", "p<0.5 and gl<0.5", axis, variables=V), f"in the callback, axis {axis}")
        Mp.assert_map(local, Mp.reference("u", "p<0.5 and gl<0.5", x, axis, variables=V), f"against numpy, axis {axis}")
        Mp.assert_map(glob, local, "global == local on one rank")


def test_two_ranks_refuse_inside_a_service_callback():
    """with two ranks a Service_Callback's pft_solver_map returns -2 (another rank's callback need not
    make the same call)"""
    V = _g20_variables()
    (vops, vargs), _ = Mp.programs("u", None, V)

    def run(sim):
        codes = []

        @P.SERVICE_FN
        def cb(final, s):
            if not codes:
                local = np.empty(10 * 10, dtype=P.MAP_DTYPE)
                codes.append(sim.lib.pft_solver_map(len(vops), P._ip(vops), P._dp(vargs), 0, None, None, 0, None,
                                                    P._map_ptr(local)))
            return 0

        sim.system.Service_Callback = C.cast(cb, C.c_void_p).value
        sim.solve(36.0)
        return codes

    out = M.loopback_run(2, lambda r: _g20_sim(0, nprocs=2, rank=r), run)
    assert out == [[-2], [-2]]
