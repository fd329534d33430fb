"""f15 on the CPU: the map record, its combine rule and its host twin (pft_map.h) against numpy
(tests/_map.py) for every axis, all by == on integers and on the bits of the doubles; the NaN, +-Inf
and signed-zero rules; Z-slabs; the refusals; the Python entries; make map-selftest."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _diag as D
import _formula as Fm
import _map as Mp
import _oracle as O
import porousfreezethaw_amd as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (0, 1, 2)


def _g20():
    meta, A = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    V = dict(zip(P.PARAM_NAMES, (float(x) for x in Pm)))
    V.update(L1=info["L1"], L2=info["L2"], L3=info["L3"])
    g = D.grid(info["n1"], info["n2"], info["n3"])
    g.L1, g.L2, g.L3 = info["L1"], info["L2"], info["L3"]
    return A, V, g


@pytest.mark.parametrize("state", ["traj_m0_ic", "traj_m0_state0"])
def test_host_twin_equals_numpy_on_golden_g20(state):
    """the three specs of the issue on the golden g20 states, for all three axes: counts == sum(axis),
    first / last == argmax-based indices with -1 where any() is false, extrema == np.max / np.min over
    the selected cells"""
    A, V, g = _g20()
    a = np.ascontiguousarray(A[state])
    w = D.padded(a)
    some = False
    for name, f, m in Mp.SPECS:
        for axis in AXES:
            got = Mp.host_map(g, w, f, m, axis, V)
            Mp.assert_map(got, Mp.reference(f, m, a, axis, variables=V), f"{state} {name} axis {axis}")
            assert got["selected"].shape == [(g.n2, g.n1), (g.n3, g.n1), (g.n3, g.n2)][axis]
            some = some or bool((got["first"] >= 0).any() and (got["first"] < 0).any())
    assert some                     # lines with and without a non-zero cell were both met
    ice = Mp.host_map(g, w, Mp.ICE, None, 0, V)
    # the front's height map and the ice thickness: the documented reading of the record
    assert (ice["nonzero"] == (a[1] > 0.5).sum(axis=0)).all() and int(ice["nonzero"].sum()) == int((a[1] > 0.5).sum())


@pytest.mark.parametrize("n1,n2,n3", [(13, 11, 9), (7, 5, 3), (1, 7, 5)])
def test_host_twin_equals_numpy_on_every_state(n1, n2, n3):
    """bit patterns, a dense state and a random one; formulas with coordinates against the node-by-node
    evaluator, so that x, y and z are each met on a kept and on the reduced axis"""
    g = Fm.grid(n1, n2, n3)
    for tag, make in Mp.states(n1, n2, n3):
        a = make()
        w = D.padded(a)
        for name, f, m in Mp.SPECS + (Mp.COORD_SPECS if tag == "random" else []):
            for axis in AXES:
                Mp.assert_map(Mp.host_map(g, w, f, m, axis), Mp.reference(f, m, a, axis), f"{tag} {name} axis {axis}")


def test_nan_inf_and_signed_zero_rules_on_planted_values():
    """with every ghost cell poisoned: a NaN counts as non-zero and as non-finite and wins no extremum,
    +-Inf win, -0.0 < +0.0, a line of NaN alone has no extremum, a NaN mask selects and a math error
    does not"""
    n1, n2, n3 = 6, 5, 4
    g = Fm.grid(n1, n2, n3)
    a = D.random_state(n1, n2, n3, 7)
    a[0] = 280.0 + np.arange(n1 * n2 * n3).reshape(n3, n2, n1)
    a[0][:, 1, 2] = [0.0, -0.0, np.nan, 5.0]          # along z at (j, i) = (1, 2)
    a[0][:, 2, 3] = [np.inf, 1.0, -np.inf, np.nan]
    a[0][:, 3, 4] = np.nan
    a[0][:, 4, 5] = [-0.0, -0.0, -0.0, -0.0]
    a[0][:, 0, 0] = [0.0, 0.0, 3.0, 0.0]
    w = D.padded(a)
    m = Mp.host_map(g, w, "u", None, 0)
    px = {k: m[k][1, 2] for k in Mp.KEYS}
    assert (px["selected"], px["nonzero"], px["nonfinite"], px["first"], px["last"]) == (4, 2, 1, 2, 3)
    assert px["min"] == 0 and np.signbit(px["min"]) and px["max"] == 5.0
    px = {k: m[k][2, 3] for k in Mp.KEYS}
    assert (px["nonzero"], px["nonfinite"], px["first"], px["last"]) == (4, 3, 0, 3)
    assert px["min"] == -np.inf and px["max"] == np.inf
    px = {k: m[k][3, 4] for k in Mp.KEYS}
    assert (px["selected"], px["nonzero"], px["nonfinite"]) == (4, 4, 4) and px["min"] == np.inf and px["max"] == -np.inf
    px = {k: m[k][4, 5] for k in Mp.KEYS}
    assert px["nonzero"] == 0 and px["first"] == px["last"] == -1 and np.signbit(px["min"]) and np.signbit(px["max"])
    px = {k: m[k][0, 0] for k in Mp.KEYS}
    assert (px["nonzero"], px["first"], px["last"]) == (1, 2, 2) and not np.signbit(px["min"]) and px["max"] == 3.0
    for axis in AXES:
        Mp.assert_map(Mp.host_map(g, w, "u", None, axis), Mp.reference("u", None, a, axis), f"planted, axis {axis}")
        # the mask u-u: NaN where u is NaN or +-Inf (selected), 0 elsewhere
        got = Mp.host_map(g, w, "p", "u-u", axis)
        Mp.assert_map(got, Mp.reference("p", "u-u", a, axis), f"NaN mask, axis {axis}")
        assert int(got["selected"].sum()) == int((~np.isfinite(a[0])).sum()) > 0
        # a math error in the mask selects nothing: every record neutral; in the value it is 0
        none = Mp.host_map(g, w, "u", "1/(gl-gl)", axis)
        assert not none["selected"].any() and (none["first"] == -1).all() and (none["last"] == -1).all()
        assert (none["min"] == np.inf).all() and (none["max"] == -np.inf).all()
        zero = Mp.host_map(g, w, "1/(gl-gl)", None, axis)
        assert not zero["nonzero"].any() and (zero["min"] == 0).all() and (zero["selected"] == (n3, n2, n1)[axis]).all()


def test_a_mask_that_selects_nothing_gives_neutral_records():
    g = Fm.grid(7, 5, 3)
    w = D.padded(D.random_state(7, 5, 3, 9))
    neutral = P.pft_map_px()
    P.lib().pft_map_init(C.byref(neutral))
    assert (neutral.selected, neutral.nonzero, neutral.nonfinite, neutral.first, neutral.last) == (0, 0, 0, -1, -1)
    assert neutral.min == np.inf and neutral.max == -np.inf and C.sizeof(P.pft_map_px) == 56 == P.MAP_DTYPE.itemsize
    for axis in AXES:
        got = Mp.host_map(g, w, "u", "p>2", axis)
        for k in Mp.KEYS:
            assert (got[k] == getattr(neutral, k)).all(), (axis, k)


@pytest.mark.parametrize("axis", AXES)
def test_combine_over_ragged_z_ranges_equals_one_slab(axis):
    """7 planes as slabs of 3 + 2 + 2: for axis 0 the slabs' partial maps combined in any order, for
    axes 1 and 2 their rows put together, are one slab's map; z enters a mask through first_row"""
    n1, n2, n3 = 6, 5, 7
    a = Mp.pattern_state(n1, n2, n3, 17)
    a[0][::2] = D.random_state(n1, n2, n3, 18)[0][::2]
    L = P.lib()
    whole = Fm.grid(n1, n2, n3)
    for f, m in (("u", Mp.ICE), ("u", "z>L3/3")):
        one = Mp.host_map(whole, D.padded(a), f, m, axis)
        Mp.assert_map(one, Mp.reference(f, m, a, axis), f"one slab, {m}")
        pieces = []
        for first, cnt in ((0, 3), (3, 2), (5, 2)):
            g = P.pft_grid.from_buffer_copy(whole)
            g.n3, g.first_row, g.total_n3 = cnt, first, n3
            pieces.append((first, cnt, Mp.host_map(g, D.padded(a[:, first:first + cnt]), f, m, axis)))
        if axis:
            for k in Mp.KEYS:
                assert np.array_equal(np.concatenate([p[2][k] for p in pieces]).view(np.int64), one[k].view(np.int64)), k
            continue
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            acc = np.zeros(n2 * n1, dtype=P.MAP_DTYPE)
            for q in range(acc.size):
                L.pft_map_init(C.byref(P.pft_map_px.from_buffer(acc, q * 56)))
            for s in order:
                rec = np.zeros(n2 * n1, dtype=P.MAP_DTYPE)
                for k in Mp.KEYS:
                    rec[k] = pieces[s][2][k].ravel()
                assert L.pft_map_combine(acc.size, P._map_ptr(acc), P._map_ptr(rec)) == 0
            Mp.assert_map(Mp.as_dict(acc, n1), one, f"order {order}")


def test_refusals():
    g = Fm.grid(7, 5, 3)
    w = D.padded(D.random_state(7, 5, 3, 9))
    L = P.lib()
    out = np.zeros(7 * 5, dtype=P.MAP_DTYPE)
    out["selected"] = -77                                  # a mark no refused call may touch
    # (the arrays outlive the programs that point into them)
    keep = [np.array(o, dtype=np.int32) for o in ([2], [101], [101])], [np.array(x) for x in ([6.0], [9.0], [6.0])]
    bad, inp, u = (Mp.hist_prog(keep[0][q], keep[1][q]) for q in range(3))
    empty = P.pft_hist_prog(0, P._ip(keep[0][2]), P._dp(keep[1][2]))

    def call(grid=g, x=w, value=u, mask=None, axis=0, o=out):
        return L.pft_map_host(None if grid is None else C.byref(grid), None if x is None else P._dp(x),
                              None if value is None else C.byref(value), None if mask is None else C.byref(mask), axis,
                              None if o is None else P._map_ptr(o))

    assert call(grid=None) == -2 and call(x=None) == -2 and call(value=None) == -2 and call(o=None) == -2
    assert call(value=bad) == -2 and call(mask=bad) == -2 and call(value=inp) == -2 and call(value=empty) == -2
    assert call(axis=3) == -2 and call(axis=-1) == -2
    none, huge = P.pft_grid.from_buffer_copy(g), P.pft_grid.from_buffer_copy(g)
    none.n3 = 0
    huge.n1, huge.n2, huge.n3 = 2048, 1024, 1024
    assert call(grid=none) == -2 and call(grid=huge) == -2
    r, c = C.c_int(), C.c_int()
    assert L.pft_map_dims(C.byref(g), 3, C.byref(r), C.byref(c)) == -2 and L.pft_map_dims(None, 0, C.byref(r), C.byref(c)) == -2
    assert L.pft_map_combine(1, None, P._map_ptr(out)) == -2 and L.pft_map_combine(-1, P._map_ptr(out), P._map_ptr(out)) == -2
    assert (out["selected"] == -77).all()
    assert call() == 0 and (out["selected"] == 3).all()


def test_python_entries_on_the_host():
    """Simulation.project(where="host") is the twin of self.x; bad arguments raise before any work"""
    A, V, g = _g20()
    meta, _ = O.load_case("g20")
    Pm, info = O.params_from_meta(meta)
    sim = P.Simulation(info["n1"], info["n2"], info["n3"], (info["L1"], info["L2"], info["L3"]), 0, Pm,
                       initial=A["traj_m0_state0"], init_solver=False)
    try:
        a = sim.interior()
        for axis in AXES:
            d = sim.project("u", axis, mask=Mp.ICE, variables=V, where="host")
            Mp.assert_map(d, Mp.reference("u", Mp.ICE, a, axis, variables=V), f"project, axis {axis}")
            assert d["axis"] == axis and d["rows"] == (0, info["n3"])
            assert d["selected"].dtype == d["first"].dtype == np.int64 and d["min"].dtype == np.float64
            e = sim.project("exp(u-u_star)", axis, variables=V, where="host", combine=False)     # every formula on the host
            assert np.isfinite(e["max"]).all() and (e["selected"] == a.shape[1 + axis]).all()
        for axis in (3, -1, 1.0, None, True):
            with pytest.raises(ValueError, match="axis"):
                sim.project("u", axis, where="host")
        with pytest.raises(ValueError, match="nope"):
            sim.project("u-nope", 0, where="host")
        with pytest.raises(RuntimeError, match="resident"):
            sim.project("u", 0)
        with pytest.raises(ValueError, match="where"):
            sim.project("u", 0, where="nowhere")
        with pytest.raises(ValueError, match="maps="):
            sim.run_series(times=[], maps={})
        with pytest.raises(ValueError, match="needs 'formula' and 'axis'"):
            sim.run_series(times=[], maps={"a": {"formula": "u"}})
        with pytest.raises(ValueError, match="unknown keys"):
            sim.run_series(times=[], maps={"a": {"formula": "u", "axis": 0, "bins": 3}})
        with pytest.raises(ValueError, match="collide"):
            sim.run_series(times=[], maps={"ice": {"formula": "u", "axis": 0}})
        with pytest.raises(ValueError, match="not device-exact"):
            sim.run_series(times=[], maps={"a": {"formula": "u^2", "axis": 0}})
    finally:
        sim.close()


def test_make_map_selftest_passes(tmp_path):
    """the stand-alone program over pft_map.c under AddressSanitizer and UBSan (CPU only)"""
    if shutil.which("make") is None or shutil.which("gcc") is None:
        pytest.fail("make and gcc are needed to build the selftest")
    r = subprocess.run(["make", "-C", os.path.join(REPO, "porousfreezethaw_amd"), "map-selftest", f"OBJ={tmp_path}"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "pft_map_selftest: ok" in r.stdout, r.stdout[-3000:]
