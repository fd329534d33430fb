"""The freeze-to-thaw switch of the top temperature (equation.c:96-111,175-183: top_temp1 while
t < phase_switch_time, top_temp2 from it on), decided once per right-hand side at that stage's own
time t, t + h/3, t + h/3, t + h/2, t + h.  libpft takes that decision in a stage launch
(run_stage), for both stages of a pair launch (run_pair: T_topA, T_topB), on the device for a gated
launch (gate_scalars), in the host model (bcond_setup), and keeps its result in the speculative
stage 1 at t + h and in the K1 carried from one pft_solve_ex call into the next.

1. tests/golden/gthaw, the reference's own g20 trajectory with the switch at 100 s, to t = 36, 360
   and 720 s on every route: t, h, both step counters, the return code and the fields bit for bit.
2. The straddle matrix on 66 x 38 x 21 (partial pair and fused tiles; four slabs hold 6/5/5/5
   planes): default Params, default IC with beads, tau = 1, 12 attempted steps, with
   phase_switch_time placed relative to the stage times of attempted step STEP[mode] -- between
   them, on them, and one double after them (where `<` and `<=`, or a stage time that is off by a
   bit, give another answer) -- against the CPU oracle.  The oracle alone first shows that each
   placement matters: the results differ pairwise.
"""
import functools

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P
from _loopback import run_slabs

pytestmark = pytest.mark.gpu

# kernel flavours, as tests/test_gpu_parity.py: (tile option, recompute stage inputs)
FLAVOURS = {"cache": (0, False), "fused32": (32, True), "fused16": (16, True), "default": (1, True),
            "fusedauto": (2, True)}
# a route: (flavour, PFT_OPT_PAIR, PFT_OPT_GATE); PFT_OPT_PAIR 1 is the library's default (by slab
# size), 2 forces the pair kernels, 0 turns them off
ROUTES = {name: (name, 1, 0) for name in FLAVOURS}
ROUTES["pairs"] = ("fusedauto", 2, 0)
ROUTES["gate"] = ("fusedauto", 0, 1)        # gated steps need the fused kernel and one launch per stage
NOPAIRS = ("fusedauto", 0, 0)

PST = O.PARAM_NAMES.index("phase_switch_time")
KEEP, REUSE = P.PFT_SOLVE_KEEP_DEVICE, P.PFT_SOLVE_REUSE_DEVICE


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


class routed:
    """the calling host thread's PFT_OPT_PAIR and PFT_OPT_GATE set for a route, the defaults after"""

    def __init__(self, route):
        self.pair, self.gate = route[1], route[2]

    def __enter__(self):
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, self.pair)
        P.lib().pft_solver_set_option(P.PFT_OPT_GATE, self.gate)

    def __exit__(self, *exc):
        P.lib().pft_solver_set_option(P.PFT_OPT_PAIR, 1)
        P.lib().pft_solver_set_option(P.PFT_OPT_GATE, 0)


def make_sim(info, Pm, mode, route, **kw):
    tile, recompute = FLAVOURS[route[0]]
    kw.setdefault("tau", 1.0)
    return P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), mode, Pm,
                        tau_min=info["tau_min"], delta=info["delta"], tile=tile, recompute=recompute, **kw)


def rec(sim, rc):
    return (sim.t.hex(), sim.h.hex(), sim.system.steps, sim.system.steps_total, rc)


def check_route_stats(st, route, gated):
    """the run took the route it was meant to take"""
    assert st.path == 1
    if route[1] == 2:
        assert st.pairs == 1
    if route[1] == 0 or route[2]:
        assert st.pairs == 0
    if route[2]:
        assert gated > 0


# ---- 1. the reference's trajectory across the switch (tests/golden/gthaw) ------------------------

@functools.lru_cache(maxsize=None)
def gthaw():
    meta, A = O.load_case("gthaw")
    Pm, info = O.params_from_meta(meta)
    assert Pm[PST] == 100.0
    for a in A.values():
        a.setflags(write=False)
    return meta, A, Pm, info


def golden_rows(meta, mode):
    return [(float.fromhex(r[0]).hex(), float.fromhex(r[1]).hex(), r[2], r[3], r[4]) for r in meta[f"traj_m{mode}"]]


GTHAW_RUNS = [(r, m) for r in list(FLAVOURS) + ["pairs", "gate"] for m in (0, 1)] + \
             [(r, 2) for r in ("default", "fusedauto", "pairs")]


@pytest.mark.parametrize("route,mode", GTHAW_RUNS)
def test_gthaw_trajectory_bitwise(route, mode):
    """RK_MPI_SA_solve to 36, 360 and 720 s: 93, 518 and 901 attempted steps in mode 0, the switch
    inside the second call"""
    meta, A, Pm, info = gthaw()
    rt = ROUTES[route]
    with routed(rt):
        sim = make_sim(info, Pm, mode, rt, initial=A[f"traj_m{mode}_ic"])
        try:
            gated = 0
            for i, T in enumerate(meta["traj_times"]):
                rc = sim.solve(T)
                assert rec(sim, rc) == golden_rows(meta, mode)[i]
                assert np.array_equal(sim.interior(), A[f"traj_m{mode}_state{i}"])
                gated += sim.stats().gated_steps
            check_route_stats(sim.stats(), rt, gated)
        finally:
            sim.close()


def slab_runs(info, Pm, mode, route, nprocs, initial, calls):
    """nprocs loopback slabs on `route`; calls: [(final time, step cap)]; per rank the record and
    interior after each call, and the pair flag"""
    def body(r):
        P.lib().pft_solver_set_option(P.PFT_OPT_GATE, route[2])
        sim = make_sim(info, Pm, mode, route, nprocs=nprocs, rank=r, initial=initial)
        try:
            res = []
            for T, cap in calls:
                rc = sim.solve_ex(T, cap, 0) if cap else sim.solve(T)
                res.append((rec(sim, rc), sim.interior()))
            return res, sim.stats().pairs
        finally:
            sim.close()

    return run_slabs(nprocs, body, pair=route[1])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("route", ["pairs", "nopairs"])
@pytest.mark.parametrize("nprocs", [2, 3])
def test_gthaw_loopback_slabs_bitwise(nprocs, route, mode):
    """20 planes on 2 and 3 slabs (7/7/6): only the top rank holds the Dirichlet planes, and with the
    pair kernels between slabs its stage A runs on the ghost planes below them"""
    meta, A, Pm, info = gthaw()
    rt = ROUTES["pairs"] if route == "pairs" else NOPAIRS
    out = slab_runs(info, Pm, mode, rt, nprocs, A[f"traj_m{mode}_ic"], [(T, 0) for T in meta["traj_times"]])
    assert all(o[1] == (1 if route == "pairs" else 0) for o in out)
    for i in range(len(meta["traj_times"])):
        for o in out:
            assert o[0][i][0] == golden_rows(meta, mode)[i]
        assert np.array_equal(np.concatenate([o[0][i][1] for o in out], axis=1), A[f"traj_m{mode}_state{i}"])


def test_gthaw_run_series_ice_rows():
    """Simulation.run_series over the three times with the device diagnostics: the rows are the
    golden's, each row's ice count that of the golden state -- it falls in the thaw"""
    meta, A, Pm, info = gthaw()
    sim = make_sim(info, Pm, 0, ROUTES["default"], initial=A["traj_m0_ic"])
    try:
        rows = sim.run_series(times=meta["traj_times"])
    finally:
        sim.close()
    assert len(rows) == 4
    assert rows[0]["ice"] == int((A["traj_m0_ic"][1] > 0.5).sum())
    for i, row in enumerate(rows[1:]):
        got = (float(row["t"]).hex(), float(row["h"]).hex(), row["steps"], row["steps_total"], row["rc"])
        assert got == golden_rows(meta, 0)[i]
        assert row["ice"] == int((A[f"traj_m0_state{i}"][1] > 0.5).sum()), i
        assert row["cells"] == A["traj_m0_ic"][1].size
    assert rows[1]["ice"] > rows[3]["ice"] > 0


@pytest.mark.parametrize("route", ["default", "pairs"])
def test_gthaw_restart_in_the_thaw(route, tmp_path):
    """gthaw to 360 s, snapshot_device to a file, a fresh Simulation(icond_file=) with t, tau and the
    parameters (phase_switch_time among them) from the dataset, solved to 720 s: the golden's third
    state and counters, as test_snapshot_restart_continues_trajectory has it for the freeze"""
    meta, A, Pm, info = gthaw()
    T1, T2 = meta["traj_times"][1:]
    path = str(tmp_path / "image.002.ncd")
    rt = ROUTES[route]
    with routed(rt):
        sim = make_sim(info, Pm, 0, rt, initial=A["traj_m0_ic"])
        try:
            for i, T in enumerate(meta["traj_times"][:2]):
                assert sim.solve_ex(T, 0, KEEP | (REUSE if i else 0)) == 0
            assert rec(sim, 0) == golden_rows(meta, 0)[1]
            sim.snapshot_device(path, P.snapshot_info(t=sim.t, tau=sim.h, final_time=T2, delta=info["delta"],
                                                      calc_mode=0, snapshot=2, total_snapshots=3,
                                                      comment="thaw restart"))
            s0, st0 = sim.system.steps, sim.system.steps_total
        finally:
            sim.close()
        n1, n2, n3, inf, prm = P.read_snapshot_info(path)
        assert np.array_equal(np.asarray(prm, dtype=np.float64), Pm)
        sim2 = P.Simulation(n1, n2, n3, (inf.L1, inf.L2, inf.L3), inf.calc_mode, prm, icond_file=path,
                            tau=inf.tau, t0=inf.t, tau_min=info["tau_min"], delta=inf.delta,
                            tile=FLAVOURS[rt[0]][0], recompute=FLAVOURS[rt[0]][1])
        try:
            assert np.array_equal(sim2.interior(), A["traj_m0_state1"])
            rc = sim2.solve(inf.final_time)
            ref = golden_rows(meta, 0)[2]
            assert (sim2.t.hex(), sim2.h.hex(), s0 + sim2.system.steps, st0 + sim2.system.steps_total, rc) == ref
            assert np.array_equal(sim2.interior(), A["traj_m0_state2"])
            check_route_stats(sim2.stats(), rt, 0)
        finally:
            sim2.close()


@pytest.mark.parametrize("route", ["default", "fusedauto", "cache"])
def test_device_rhs_at_the_switch(route):
    """f_generic_model01 (the host model's ghost fill, then a stage launch's T_top) on the gthaw IC
    at the last double before the switch, at it and at the first after it: the oracle's RHS each
    time; the first two differ, the last two are equal"""
    meta, A, Pm, info = gthaw()
    sim = make_sim(info, Pm, 0, ROUTES[route], initial=A["traj_m0_ic"], init_solver=False)
    try:
        K = []
        for t in (np.nextafter(100.0, 0.0), 100.0, np.nextafter(100.0, np.inf)):
            dw, _ = P.rhs(sim, float(t))
            K.append(dw.reshape((3,) + sim.N)[:, 2:-2, 2:-2, 2:-2].copy())
            assert np.array_equal(K[-1], O.rhs(info, Pm, 0, float(t), A["traj_m0_ic"])[0]), t
    finally:
        sim.close()
    assert not np.array_equal(K[0], K[1]) and np.array_equal(K[1], K[2])


# ---- 2. the straddle matrix ------------------------------------------------------------------------

DIMS = (66, 38, 21)
NSTEPS = 12
# the attempted step (1-based) whose stage times the switch is placed at, per calc_mode: step 8 is
# sensitive in all three (test_placements_matter_to_the_oracle); in mode 0 it starts at
# t = 0x1.0cacf2e414c08p-8 = 0.0040997 s with h = 0.0011913 s
STEP = {0: 8, 1: 8, 2: 8}

EIGHT = ["before", "in_t_h3", "at_h3", "in_h3_h2", "at_h2", "in_h2_h", "at_h", "after"]
NEXT = {"next_h3": "at_h3", "next_h2": "at_h2", "next_h": "at_h"}       # one double after a stage time
PLACEMENTS = EIGHT + list(NEXT)
MODE12_PLACEMENTS = ["in_h3_h2", "at_h2", "in_h2_h"]
SLAB_PLACEMENTS = ["in_h2_h", "at_h3"]


@functools.lru_cache(maxsize=None)
def straddle_base():
    """default Params (the g20 golden's), the grid, and the default IC with beads per calc_mode"""
    meta, _ = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    n1, n2, n3 = DIMS
    info = dict(info, n1=n1, n2=n2, n3=n3)
    ic = O.ic_default(info, Pm, O.beads())
    ic.setflags(write=False)
    Pm.setflags(write=False)
    return Pm, info, ic


@functools.lru_cache(maxsize=None)
def step_times(mode):
    """(t_n, h_n) before every attempted step n = 1 .. NSTEPS of the undisturbed run (the switch at
    5 h), from the oracle driven one attempted step at a time -- which equals the continuous run"""
    Pm, info, ic = straddle_base()
    res = O.solve(info, Pm, mode, ic, 0.0, 1.0, [1e9] * NSTEPS, max_steps_total=1)
    cont = O.solve(info, Pm, mode, ic, 0.0, 1.0, [1e9], max_steps_total=NSTEPS)[0]
    assert all(r[4] == 2 for r in res) and cont[4] == 2
    assert res[-1][:4] == cont[:4] and np.array_equal(res[-1][5], cont[5]), "stepwise != continuous"
    return [(0.0, 1.0)] + [(r[0], r[1]) for r in res[:-1]]


def placement(mode, name):
    """phase_switch_time for a placement, from (t, h) of attempted step STEP[mode] and the solver's
    own expressions for the stage times (hybrid2.c:355: h/3.0, h/2.0)"""
    t, h = step_times(mode)[STEP[mode] - 1]
    b3, b2, b1 = t + h / 3.0, t + h / 2.0, t + h
    assert t < b3 < b2 < b1
    if name in NEXT:
        return float(np.nextafter(placement(mode, NEXT[name]), np.inf))
    return {"before": float(np.nextafter(t, 0.0)), "in_t_h3": t + h / 6.0, "at_h3": b3, "in_h3_h2": 0.5 * (b3 + b2),
            "at_h2": b2, "in_h2_h": 0.5 * (b2 + b1), "at_h": b1, "after": b1 + h / 4.0}[name]


def params_with_switch(mode, name):
    Pm, _, _ = straddle_base()
    Pm = Pm.copy()
    Pm[PST] = placement(mode, name)
    return Pm


@functools.lru_cache(maxsize=None)
def oracle_result(mode, name):
    """the one-slab oracle's NSTEPS attempted steps with the switch at the placement"""
    _, info, ic = straddle_base()
    t, h, s, st, rc, x = O.solve(info, params_with_switch(mode, name), mode, ic, 0.0, 1.0, [1e9],
                                 max_steps_total=NSTEPS)[0]
    assert rc == 2 and st == NSTEPS
    x.setflags(write=False)
    return (t.hex(), h.hex(), s, st, rc), x


def differ(a, b):
    return a[0] != b[0] or not np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def assert_sensitive(mode):
    """on the oracle alone, before any device comparison: every placement changes the result"""
    names = EIGHT if mode == 0 else MODE12_PLACEMENTS
    vals = [placement(mode, n) for n in names]
    assert vals == sorted(vals) and len(set(vals)) == len(vals)
    res = {n: oracle_result(mode, n) for n in names}
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert differ(res[a], res[b]), f"mode {mode}: placements {a} and {b} give the same result"
    if mode == 0:
        for n, b in NEXT.items():
            assert placement(0, n) > placement(0, b)
            assert differ(oracle_result(0, n), oracle_result(0, b)), f"{b} and the next double give the same result"
    return True


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_placements_matter_to_the_oracle(mode):
    """the stepwise oracle equals the continuous one, and the placements give pairwise different
    results (mode 0: the eight of EIGHT, and each stage time against the next double)"""
    assert len(step_times(mode)) == NSTEPS
    assert assert_sensitive(mode)
    if mode == 0:
        # the 45 K jump is rejected at first: fewer accepted steps than attempted ones
        assert all(oracle_result(0, n)[0][2] < NSTEPS for n in EIGHT[1:7])


def device_run(mode, route, Pm, caps=(NSTEPS,)):
    """one slab on `route` through pft_solve_ex calls with the step caps `caps` (the state kept on
    the device between them when there are several); the final record, state and stats"""
    _, info, ic = straddle_base()
    with routed(route):
        sim = make_sim(info, Pm, mode, route, initial=ic)
        try:
            gated, launches = 0, []
            for i, cap in enumerate(caps):
                flags = 0 if len(caps) == 1 else (KEEP | (REUSE if i else 0))
                rc = sim.solve_ex(1e9, cap, flags)
                gated += sim.stats().gated_steps
                launches.append(sim.stats().kernel_launches)
            if len(caps) > 1:
                sim.download()
            check_route_stats(sim.stats(), route, gated)
            return rec(sim, rc), sim.interior(), launches
        finally:
            sim.close()


def assert_same(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", PLACEMENTS)
@pytest.mark.parametrize("route", ["cache", "fused32", "fusedauto", "default", "pairs", "gate"])
def test_straddle_mode0(route, name):
    assert assert_sensitive(0)
    assert_same(device_run(0, ROUTES[route], params_with_switch(0, name)), oracle_result(0, name))


@pytest.mark.parametrize("name", MODE12_PLACEMENTS)
@pytest.mark.parametrize("route", ["fusedauto", "pairs"])
@pytest.mark.parametrize("mode", [1, 2])
def test_straddle_modes_1_and_2(mode, route, name):
    """with that mode's own (t, h) of step STEP[mode]"""
    assert assert_sensitive(mode)
    assert_same(device_run(mode, ROUTES[route], params_with_switch(mode, name)), oracle_result(mode, name))


@pytest.mark.parametrize("name", SLAB_PLACEMENTS)
@pytest.mark.parametrize("route", ["pairs", "nopairs"])
@pytest.mark.parametrize("nprocs", [2, 4])
def test_straddle_loopback_slabs(nprocs, route, name):
    """two and four slabs (11/10 and 6/5/5/5 planes) against the one-slab oracle run"""
    assert assert_sensitive(0)
    _, info, ic = straddle_base()
    rt = ROUTES["pairs"] if route == "pairs" else NOPAIRS
    out = slab_runs(info, params_with_switch(0, name), 0, rt, nprocs, ic, [(1e9, NSTEPS)])
    want = oracle_result(0, name)
    assert all(o[1] == (1 if route == "pairs" else 0) for o in out)
    for o in out:
        assert o[0][0][0] == want[0]
    assert np.array_equal(np.concatenate([o[0][0][1] for o in out], axis=1), want[1])


@pytest.mark.parametrize("name", ["before", "in_h2_h"])
@pytest.mark.parametrize("caps", [(7, 1, 4), (8, 4)])
@pytest.mark.parametrize("route", ["default", "fusedauto", "pairs"])
def test_straddle_k1_carried_across_calls(route, caps, name):
    """pft_solve_ex with KEEP_DEVICE / REUSE_DEVICE and step caps 7, 1, 4: the second call is
    exactly the straddling attempt and starts from the K1 = f(t, x) the first call left on the
    device (with `before`, the first K1 of the thaw).  Caps 8, 4: the carried K1 follows the
    straddling attempt, accepted or rejected.  Both equal the continuous oracle run.  That K1 was
    carried shows in the one-attempt call's launches on the routes that always speculate: stages
    2-5 and the speculative stage 1 (fusedauto), or two pair launches and it (pairs), no stage 1"""
    assert STEP[0] == 8 and sum(caps) == NSTEPS
    assert assert_sensitive(0)
    got = device_run(0, ROUTES[route], params_with_switch(0, name), caps=caps)
    assert_same(got, oracle_result(0, name))
    if caps[1] == 1 and route != "default":
        assert got[2][1] == (3 if route == "pairs" else 5)
