"""f12 on the CPU: the host twin pft_formula_host against the independent reference (tests/_formula.py:
frontend.Evaluator node by node, Fraction sums rounded once) by ==, the record's combine laws,
Z-slabs combined against one slab word for word, the identities with f5 (pft_diag_host) and f6
(pft_means_host), the compile outcomes of the device route, and every refusal of the Python
entries that needs no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import _diag as D
import _formula as Fm
import _means as Mn
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE

SHAPES = [(13, 11, 9), (7, 5, 3)]


def _states(n1, n2, n3):
    return Fm.states(n1, n2, n3) + [("wide-special", lambda: Mn.special(Mn.wide_state(n1, n2, n3, 64), 65))]


@pytest.mark.parametrize("n1,n2,n3", SHAPES)
def test_host_twin_equals_the_independent_reference(n1, n2, n3):
    g = Fm.grid(n1, n2, n3)
    for tag, make in _states(n1, n2, n3):
        a = make()
        w = D.padded(a)
        before = w.copy()
        # (the non-exact formulas on finite states only: Python's math.floor raises on +-Inf where C's
        # floor returns it, and the host evaluator takes exp(+Inf) for an overflow where Python's
        # math.exp returns +Inf, so for `u C 2` and `exp(u-u_star)` the Python evaluator is no
        # reference at an infinite u)
        for formulas in Fm.CALLS + ([Fm.NOT_EXACT] if "special" not in tag else []):
            want = Fm.cached_reference((tag, n1, n2, n3), formulas, lambda: a)
            names, total, planes = Fm.host_formulas(g, w, formulas)
            assert names == list(formulas)
            for f, name in enumerate(names):
                Fm.assert_dict(total[f].as_dict(), want[name][0], f"{tag} {name}")
                assert total[f].cells == total[f].n + total[f].nonfinite == n1 * n2 * n3
                for k in range(n3):
                    Fm.assert_dict(planes[f][k].as_dict(), want[name][1][k], f"{tag} {name} plane {k}")
                alone = Fm.host_formulas(g, w, {name: formulas[name]}, per_plane=False)[1][0]
                Fm.assert_words(alone, total[f], f"{tag} {name} alone, without per_plane")
        assert np.array_equal(w, before, equal_nan=True)          # nothing is written into the state


def test_math_errors_and_the_empty_cases():
    """sqrt(u-300) is 0 where u < 300 and 1/(gl-gl) is 0 everywhere: finite zeros that count"""
    a = D.random_state(13, 11, 9, 61)
    g = Fm.grid(13, 11, 9)
    _, total, _ = Fm.host_formulas(g, D.padded(a), {"s": Fm.F["f10"], "z": Fm.F["f11"], "nan": "u-u", "big": "u*1e308*1e308"})
    s, z = total[0].as_dict(), total[1].as_dict()
    assert s["n"] == s["cells"] == a[0].size and s["nonzero"] == int((a[0] > 300).sum()) and s["min"] == 0.0
    assert z == {"cells": a[0].size, "n": a[0].size, "nonzero": 0, "nonfinite": 0, "min": 0.0, "max": 0.0, "maxabs": 0.0,
                 "sum": 0.0, "mean": 0.0}
    nan = Fm.host_formulas(g, D.padded(np.full_like(a, np.nan)), {"nan": "u"})[1][0].as_dict()
    assert nan["n"] == 0 and nan["nonfinite"] == nan["nonzero"] == nan["cells"] and math.isnan(nan["mean"])
    assert nan["min"] == math.inf and nan["max"] == -math.inf and nan["maxabs"] == 0.0 and nan["sum"] == 0.0
    big = total[3].as_dict()
    assert big["n"] == 0 and big["max"] == big["min"] == big["maxabs"] == math.inf


def test_combine_laws():
    """associative and commutative bit for bit, the record of no cells neutral, -0.0 below +0.0"""
    g = Fm.grid(7, 5, 3)
    recs = []
    for seed, make in enumerate([lambda: D.random_state(7, 5, 3, 1), lambda: Mn.wide_state(7, 5, 3, 2),
                                 lambda: Mn.special(Mn.wide_state(7, 5, 3, 3), 4)]):
        recs += list(Fm.host_formulas(g, D.padded(make()), Fm.CALLS[0], per_plane=False)[1])

    def comb(x, y):
        out = P.pft_fdiag.from_buffer_copy(x)
        assert P.lib().pft_fdiag_combine(C.byref(out), C.byref(y)) == 0
        return out

    empty = P.pft_fdiag()
    P.lib().pft_fdiag_init(C.byref(empty))
    assert (empty.cells, empty.min, empty.max, empty.maxabs) == (0, math.inf, -math.inf, 0.0) and not any(empty.sum.w)
    for x in recs[:8]:
        Fm.assert_words(comb(x, empty), x, "neutral on the right")
        Fm.assert_words(comb(empty, x), x, "neutral on the left")
        for y in recs[8:16]:
            Fm.assert_words(comb(x, y), comb(y, x), "commutative")
            for z in recs[16:20]:
                Fm.assert_words(comb(comb(x, y), z), comb(x, comb(y, z)), "associative")
    lo, hi = P.pft_fdiag(), P.pft_fdiag()
    for r, v in ((lo, -0.0), (hi, 0.0)):
        P.lib().pft_fdiag_init(C.byref(r))
        r.cells = r.n = 1
        r.min = r.max = v
    for m in (comb(lo, hi), comb(hi, lo)):
        assert math.copysign(1.0, m.min) == -1.0 and math.copysign(1.0, m.max) == 1.0
    assert P.lib().pft_fdiag_combine(None, C.byref(lo)) == -2


@pytest.mark.parametrize("nprocs", [1, 2, 3])
def test_z_slabs_combine_to_one_slab(nprocs):
    """13x11x9 cut into 1-3 Z-slabs: the slabs' records combined are the single slab's words for every
    formula -- 6 (its threshold plane inside one slab) and 7 (tables independent of the slab) too --
    and the slabs' plane records side by side are its planes'"""
    n1, n2, n3 = 13, 11, 9
    for tag, make in Fm.states(n1, n2, n3):
        a = make()
        for formulas in Fm.CALLS:
            names, one, one_planes = Fm.host_formulas(Fm.grid(n1, n2, n3), D.padded(a), formulas)
            acc = (P.pft_fdiag * len(names))()
            for f in range(len(names)):
                P.lib().pft_fdiag_init(C.byref(acc[f]))
            side = [[] for _ in names]
            for r in range(nprocs):
                g = Fm.grid(n1, n2, n3, nprocs, r)
                part = np.ascontiguousarray(a[:, g.first_row:g.first_row + g.n3])
                _, tot, planes = Fm.host_formulas(g, D.padded(part), formulas)
                for f in range(len(names)):
                    P.lib().pft_fdiag_combine(C.byref(acc[f]), C.byref(tot[f]))
                    side[f] += planes[f]
            for f, name in enumerate(names):
                Fm.assert_words(acc[f], one[f], f"{tag} {name}: {nprocs} slabs")
                assert [m.words() for m in side[f]] == [m.words() for m in one_planes[f]]


def test_identities_with_diag_and_means():
    n1, n2, n3 = 13, 11, 9
    g = Fm.grid(n1, n2, n3)
    for tag, make in Fm.states(n1, n2, n3):
        a = make()
        w = D.padded(a)
        names, total, _ = Fm.host_formulas(g, w, Fm.CALLS[0], per_plane=False)
        r = {name: total[f] for f, name in enumerate(names)}
        diag, _ = D.host_diag(g, w)
        means, _ = Mn.host_means(g, w, per_plane=False)
        assert r["f1"].nonzero == diag["ice"] and r["f1"].as_dict()["sum"] == float(diag["ice"])
        assert r["f1"].as_dict()["mean"] == diag["ice"] / diag["cells"]
        assert r["f2"].nonzero == diag["pore"]
        assert list(r["f3"].sum.w) == list(means.sum[0].w) and r["f3"].n == means.n[0]
        assert Mn.same(r["f3"].min, diag["u_min"]) and Mn.same(r["f3"].max, diag["u_max"])
        if tag != "special":
            assert Mn.same(r["f4"].maxabs, diag["ice_u_maxabs"])
            assert list(r["f4"].sum.w) == list(means.sum[2].w)


def test_compile_outcomes():
    """pft_formula_compile: 0 for all of F, 1 for the four non-exact formulas; C and P are refused over
    a field and over several coordinates but folded over constants and one coordinate; the IC
    path's pft_ic_device_ok still takes them"""
    g = Fm.grid(13, 11, 9)
    for call in Fm.CALLS:
        c = Fm.Compiled(g, call)
        assert c.codes == [0] * len(call)
        c.free()
    c = Fm.Compiled(g, Fm.NOT_EXACT)
    assert c.codes == [1, 1, 1, 1]
    c.free()
    loops = {"a": "u P 2", "b": "(floor(_x*5)+3) C floor(_y*3)", "c": "5 C 2 + u", "d": "(floor(_x*5)+3) P 2 + p",
             "e": "(3 C 2)*gl"}
    c = Fm.Compiled(g, loops)
    assert c.codes == [1, 1, 0, 0, 0]
    assert all(o not in (5, 6) for pr, code in zip(c.progs, c.codes) if code == 0 for o in pr.op[:pr.n])
    c.free()
    names, lens, ops, args = P.formula_programs({"a": "u C 2"}, Fm.VARIABLES)
    assert P.lib().pft_ic_device_ok(C.byref(g), int(lens[0]), P._ip(ops), P._dp(args)) == 1
    pr = P.pft_ic_prog()
    long_ops = np.full(257, 100, dtype=np.int32)
    assert P.lib().pft_formula_compile(C.byref(g), 257, P._ip(long_ops), P._dp(np.zeros(257)), C.byref(pr)) == -2


def test_host_limits_and_bad_programs():
    g = Fm.grid(7, 5, 3)
    w = D.padded(D.random_state(7, 5, 3, 1))
    out = (P.pft_fdiag * 9)()
    one = (np.array([1], dtype=np.int32), np.array([100], dtype=np.int32), np.array([1.0]))

    def call(nprog, lens, ops, args, grid=g):
        return P.lib().pft_formula_host(C.byref(grid), P._dp(w), nprog, P._ip(lens), P._ip(ops), P._dp(args), out, None)

    assert call(1, *one) == 0 and out[0].nonzero == 105
    assert call(0, *one) == -2
    nine = (np.ones(9, dtype=np.int32), np.full(9, 100, dtype=np.int32), np.ones(9))
    assert call(9, *nine) == -2 and call(8, nine[0][:8].copy(), nine[1], nine[2]) == 0
    # 256 entries in all pass, 257 do not: "1 1 + 1 + ..." as two programs
    def chain(n):       # n entries (odd): 1, then (1 +) pairs
        return [100] + [100, 2] * ((n - 1) // 2)
    ops = np.array(chain(255) + chain(1), dtype=np.int32)
    assert call(2, np.array([255, 1], dtype=np.int32), ops, np.ones(256)) == 0 and out[0].max == 128.0
    ops = np.array(chain(255) + chain(3)[:2], dtype=np.int32)
    assert call(2, np.array([255, 2], dtype=np.int32), ops, np.ones(257)) == -2
    # bad programs: an unknown operator, a stack underflow, two values left, an input past gl
    for bad in ([100, 16], [2], [100, 100], [101]):
        args = np.full(len(bad), 9.0)
        assert call(1, np.array([len(bad)], dtype=np.int32), np.array(bad, dtype=np.int32), args) == -2
    huge = P.pft_grid()
    huge.n1, huge.n2, huge.n3, huge.total_n3, huge.nprocs = 2048, 1024, 1024, 1024, 1
    assert call(1, *one, grid=huge) == -2                         # 2^31 cells: refused before any read
    assert P.lib().pft_formula_host(C.byref(g), None, 1, P._ip(one[0]), P._ip(one[1]), P._dp(one[2]), out, None) == -2


def test_python_refusals_and_the_input_rule():
    with pytest.raises(ValueError, match="non-empty"):
        P.formula_programs({})
    with pytest.raises(ValueError, match="at most 8"):
        P.formula_programs({f"n{i}": "u" for i in range(9)})
    with pytest.raises(FE.EvalError, match="'bad'.*u_star"):
        P.formula_programs({"ok": "u", "bad": "u-u_star"})               # no variables given
    with pytest.raises(FE.EvalError, match="syntax"):
        P.formula_programs({"bad": "u +"})
    with pytest.raises(ValueError, match="more than 256"):
        P.formula_programs({"a": "+".join(["u"] * 100), "b": "+".join(["p"] * 100)})
    # the nine node inputs mean the node's own values whatever `variables` defines; an Evaluator
    # given as `variables` is read, not changed
    ev = FE.Evaluator()
    ev.define("u", 1e9)
    ev.define("u_star", 273.15)
    before = [list(e) for e in ev.ident]
    names, lens, ops, args = P.formula_programs({"a": "u-u_star"}, ev)
    assert [list(e) for e in ev.ident] == before
    assert list(ops) == [101, 100, 1] and list(args) == [6.0, 273.15, 0.0]
    assert list(P.formula_programs({"a": "u-u_star"}, {"u": 1e9, "u_star": 273.15})[2]) == [101, 100, 1]


def test_evaluator_sqrt_follows_the_reference_handler():
    """exp_all.cc's __sqrt__ refuses x < 0 and nothing else: a NaN goes through to sqrt (and comes back
    a NaN), as in pft_frontend.c; a negative argument is a domain error, -0.0 and +Inf are not"""
    ev = FE.Evaluator()
    for v, want in ((float("nan"), math.nan), (4.0, 2.0), (-0.0, -0.0), (math.inf, math.inf)):
        ev.define("v", v)
        assert Mn.same(ev.eval("sqrt(v)"), want)
    ev.define("v", -1e-300)
    with pytest.raises(FE.EvalError, match="domain"):
        ev.eval("sqrt(v)")
    # the emit-only compile: the program of a formula whose placeholder inputs have a math error
    ev.define("u", 0.5)
    assert ev.compile("sqrt(u-300)", ("u",), evaluate=False) == [(101, 0.0), (100, 300.0), (1, 0.0), (41, 0.0)]
    with pytest.raises(FE.EvalError):
        ev.compile("sqrt(u-300)", ("u",))


def test_simulation_formulas_host_route_and_refusals():
    """Simulation.formulas(where="host") needs no device: it accepts every formula, the non-exact
    ones too; where="device" without a resident state raises RuntimeError; bad arguments raise
    before any work"""
    base = Fm.VARIABLES
    a = D.random_state(10, 10, 20, 5)
    sim = P.Simulation(10, 10, 20, Fm.L, 0, P.params_array(base), initial=a, init_solver=False)
    try:
        got = sim.formulas({**Fm.CALLS[1], **Fm.NOT_EXACT}, variables=base, where="host", per_plane=True)
        want = Fm.reference({**Fm.CALLS[1], **Fm.NOT_EXACT}, a)
        for name, d in got.items():
            Fm.assert_dict(d, want[name][0], name)
            assert [Mn.same(float(x), y["mean"]) for x, y in zip(d[name + "_profile"], want[name][1])] == [True] * 20
            assert d["first_row"] == 0 and d["local"] == {k: d[k] for k in Fm.KEYS}
            assert len(d["plane_records"]) == 20 and d["record"].cells == 2000
        with pytest.raises(RuntimeError, match="resident"):
            sim.formulas({"a": "u"})
        with pytest.raises(ValueError, match="where"):
            sim.formulas({"a": "u"}, where="gpu")
        with pytest.raises(ValueError):
            sim.formulas({})
        with pytest.raises(FE.EvalError, match="nope"):
            sim.formulas({"a": "u*nope"}, where="host")
        with pytest.raises(ValueError, match="collide"):
            sim.run_series(times=[1.0], formulas={"ice": "p>0.5", "u": "u"})      # u_mean is means()' key
        with pytest.raises(ValueError, match="not device-exact"):
            sim.run_series(times=[1.0], formulas={"sq": "u^2"})
    finally:
        sim.close()
