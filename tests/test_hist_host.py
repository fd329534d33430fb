"""f13 on the CPU: the histogram record, its rule and its host twin (pft_hist.h) against
numpy.histogram with explicit edges on values from the independent evaluator of tests/_formula.py
(tests/_hist.py), all by == on integers; the refusals; Z-slabs; the identities with f12 and f5; the
Python entries."""
import ctypes as C

import numpy as np
import pytest

import _diag as D
import _formula as Fm
import _hist as H
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE

SHAPES = [(13, 11, 9), (7, 5, 3)]


def _bin(edges, v):
    e = np.ascontiguousarray(edges, dtype=np.float64)
    return P.lib().pft_hist_bin(e.size - 1, P._dp(e), float(v))


def test_bin_rule_is_numpy_histogram_on_the_edge_cases():
    """+-0.0 with an edge at 0.0, every edge, both neighbours of every edge, the last edge, +-Inf:
    pft_hist_bin names the bin numpy.histogram counts the value in (none: under / over); NaN is its
    own answer"""
    e = H.IRREGULAR
    vals = [0.0, -0.0, np.inf, -np.inf]
    for x in e:
        vals += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    for v in vals:
        c = np.histogram([v], bins=e)[0]
        b = _bin(e, v)
        if c.sum() == 0:
            assert b == (-1 if v < e[0] else -2) and (v < e[0] or v > e[-1]), v
        else:
            assert b == int(np.argmax(c)), (v, b)
    assert _bin(e, e[-1]) == 6 and _bin(e, -0.0) == 3 and _bin(e, np.nextafter(0.0, -1.0)) == 2
    assert _bin(e, np.nan) == -3 and _bin(e, np.inf) == -2 and _bin(e, -np.inf) == -1
    assert _bin([1.0, 2.0], 1.0) == 0 and _bin([1.0, 2.0], 2.0) == 0           # one bin: both edges inside
    big = np.linspace(0.0, 1024.0, 1025)
    assert [_bin(big, v) for v in (0.0, 0.5, 1023.0, 1023.999, 1024.0, 511.0)] == [0, 0, 1023, 1023, 1023, 511]


@pytest.mark.parametrize("n1,n2,n3", SHAPES)
def test_host_twin_equals_numpy(n1, n2, n3):
    """pft_hist_host of a padded array with poisoned ghosts == numpy for the slab and every plane, on
    every state and spec (1 and 1024 bins among them); the planes' rows sum to the slab's"""
    g = Fm.grid(n1, n2, n3)
    for tag, make, extra in H.states(n1, n2, n3):
        a = make()
        w = D.padded(a)
        sp = H.specs(a) + extra
        want = H.reference(sp, a)
        for name, f, edges, m in sp:
            got = H.host_hist(g, w, f, edges, m)
            H.assert_all(got, want[name], f"{tag} {name}")
            assert got[0][0]["cells"] == n1 * n2 * n3
            assert (sum(c for _, c in got[1]) == got[0][1]).all()
            for k in H.HEAD_KEYS:
                assert sum(h[k] for h, _ in got[1]) == got[0][0][k]
            alone = H.host_hist(g, w, f, edges, m, per_plane=False)
            H.assert_rows(alone[0], want[name][0], f"{tag} {name}: without per_plane")
        if tag == "one_bin":
            h, c = H.host_hist(g, w, "u", sp[0][2], None)[0]
            assert c.max() == h["cells"] == h["selected"]
        if tag == "ramp" and n1 * n2 * n3 >= 1024:
            c = H.host_hist(g, w, *H.RAMP[1:])[0][1]
            assert c.min() >= 1 and c.max() - c.min() <= 1


def test_edges_state_holds_what_it_promises():
    a = H.edges_state(7, 5, 3)
    u = a[0].ravel()
    for e in H.IRREGULAR:
        for v in (e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)):
            assert (u == v).any()
    assert np.isnan(u).any() and (u == np.inf).any() and (u == -np.inf).any()
    assert ((u == 0) & np.signbit(u)).any() and ((u == 0) & ~np.signbit(u)).any()
    got = H.host_hist(Fm.grid(7, 5, 3), D.padded(a), *H.EDGES[1:])[0]
    assert got[0]["nan"] == 1 and got[0]["under"] >= 2 and got[0]["over"] >= 2


def test_a_nan_mask_selects_and_a_math_error_does_not():
    a = Fm.states(13, 11, 9)[2][1]()                      # special: NaN and +-Inf in u
    g, w = Fm.grid(13, 11, 9), D.padded(a)
    e = P.hist_edges(8, (200.0, 340.0))
    nonfinite = int((~np.isfinite(a[0])).sum())
    assert nonfinite > 0
    (h, c), _ = H.host_hist(g, w, "p", e, "u-u")         # NaN where u is NaN or +-Inf, else 0
    assert h["selected"] == nonfinite and h["cells"] == a[0].size
    finite = D.padded(D.random_state(13, 11, 9, 61))     # gl finite: gl - gl is 0 at every cell
    (h, c), _ = H.host_hist(g, finite, "u", e, "1/(gl-gl)")   # a division by zero: 0, not selected
    assert h["selected"] == 0 and c.sum() == 0 and h["nan"] == h["under"] == h["over"] == 0
    (h, c), _ = H.host_hist(g, finite, "1/(gl-gl)", P.hist_edges([-1.0, 0.0, 1.0]), None)     # ... as a value: 0.0
    assert c.tolist() == [0, a[0].size]
    want = H.reference([("x", "u", e, "u-u")], a)["x"]
    H.assert_all(H.host_hist(g, w, "u", e, "u-u"), want, "NaN mask")
    assert want[0][0]["nan"] == int(np.isnan(a[0]).sum())


def test_combine_laws():
    r = np.random.default_rng(3)
    L = P.lib()

    def rec():
        h = P.pft_hist_head(*[int(x) for x in r.integers(0, 1 << 40, 5)])
        return h, (C.c_longlong * 5)(*[int(x) for x in r.integers(0, 1 << 40, 5)])

    def comb(x, y):
        h, c = P.pft_hist_head.from_buffer_copy(x[0]), (C.c_longlong * 5)(*x[1])
        assert L.pft_hist_combine(5, C.byref(h), c, C.byref(y[0]), y[1]) == 0
        return h, c

    def words(x):
        return list(x[0].as_dict().values()) + list(x[1])

    a, b, c = rec(), rec(), rec()
    zero = (P.pft_hist_head(), (C.c_longlong * 5)())
    assert words(comb(a, b)) == words(comb(b, a))
    assert words(comb(comb(a, b), c)) == words(comb(a, comb(b, c)))
    assert words(comb(a, zero)) == words(a) == words(comb(zero, a))
    assert L.pft_hist_combine(0, C.byref(a[0]), a[1], C.byref(b[0]), b[1]) == -2
    assert L.pft_hist_combine(1025, C.byref(a[0]), a[1], C.byref(b[0]), b[1]) == -2
    assert L.pft_hist_combine(5, None, a[1], C.byref(b[0]), b[1]) == -2


BAD_EDGES = [[0.0, 0.0, 1.0], [0.0, -0.0], [-0.0, 0.0], [0.0, np.nan], [np.nan, 1.0], [0.0, np.inf], [-np.inf, 0.0],
             [1.0, 0.0], [0.0, 2.0, 1.0], [1.0]]


def test_every_refusal():
    L = P.lib()
    for bad in BAD_EDGES:
        e = np.array(bad)
        assert L.pft_hist_check(e.size - 1, P._dp(e)) == -2, bad
        with pytest.raises(ValueError):
            P.hist_edges(bad)
    ok = np.linspace(0.0, 1.0, 1026)
    assert L.pft_hist_check(1024, P._dp(ok)) == 0 and L.pft_hist_check(1025, P._dp(ok)) == -2
    assert L.pft_hist_check(0, P._dp(ok)) == -2 and L.pft_hist_check(1, None) == -2
    assert L.pft_hist_check(1, P._dp(np.array([-5e-324, 0.0]))) == 0

    g, a = Fm.grid(7, 5, 3), D.random_state(7, 5, 3, 1)
    w = D.padded(a)
    (vops, vargs), _ = H.programs("u", None)
    e = P.hist_edges(4, (0.0, 1.0))
    head, counts = P.pft_hist_head(), (C.c_longlong * 4)()

    def call(grid=g, x=w, ops=vops, args=vargs, n=None, mask=None, nbins=4, edges=e, hd=head, cn=counts):
        value = P.pft_hist_prog(len(ops) if n is None else n, P._ip(ops), P._dp(args))
        return L.pft_hist_host(C.byref(grid), None if x is None else P._dp(x), C.byref(value), mask, nbins,
                               None if edges is None else P._dp(edges), None if hd is None else C.byref(hd), cn, None, None)

    assert call() == 0
    head.cells = -77                                            # a mark no refused call may touch
    assert call(x=None) == -2 and call(edges=None) == -2 and call(hd=None) == -2 and call(cn=None) == -2
    assert call(nbins=0) == -2 and call(nbins=1025) == -2 and call(n=0) == -2
    for bad in BAD_EDGES[:-1]:
        assert call(nbins=len(bad) - 1, edges=np.array(bad)) == -2
    bad_ops = np.array([2], dtype=np.int32)                     # an operator on an empty stack
    assert call(ops=bad_ops, args=np.zeros(1)) == -2
    assert call(mask=C.byref(P.pft_hist_prog(1, P._ip(bad_ops), P._dp(np.zeros(1))))) == -2
    assert L.pft_hist_host(C.byref(g), P._dp(w), None, None, 4, P._dp(e), C.byref(head), counts, None, None) == -2
    huge = P.pft_grid()
    huge.n1, huge.n2, huge.n3, huge.total_n3, huge.nprocs = 2048, 1024, 1024, 1024, 1
    assert call(grid=huge) == -2                                # 2^31 cells: refused before any read
    none = P.pft_grid()
    assert call(grid=none) == -2
    assert head.cells == -77


@pytest.mark.parametrize("nprocs", [1, 2, 3])
def test_z_slabs_combine_to_one_slab(nprocs):
    """13x11x9 cut into 1-3 Z-slabs: the slabs' records combined are the single slab's, the z mask's
    threshold plane inside one slab; the slabs' planes side by side are its planes"""
    n1, n2, n3 = 13, 11, 9
    a = D.random_state(n1, n2, n3, 61)
    for name, f, edges, m in H.specs(a):
        one = H.host_hist(Fm.grid(n1, n2, n3), D.padded(a), f, edges, m)
        nbins = edges.size - 1
        acc_h, acc_c, side = P.pft_hist_head(), (C.c_longlong * nbins)(), []
        for r in range(nprocs):
            g = Fm.grid(n1, n2, n3, nprocs, r)
            part = np.ascontiguousarray(a[:, g.first_row:g.first_row + g.n3])
            (h, c), planes = H.host_hist(g, D.padded(part), f, edges, m)
            oh, oc = P.pft_hist_head(**h), (C.c_longlong * nbins)(*[int(x) for x in c])
            assert P.lib().pft_hist_combine(nbins, C.byref(acc_h), acc_c, C.byref(oh), oc) == 0
            side += planes
        H.assert_all(((acc_h.as_dict(), np.array(acc_c[:], dtype=np.int64)), side), one, f"{name}: {nprocs} slabs")


def test_thread_count_does_not_matter():
    """1 against 4 OpenMP threads, in a child process each (the thread count is read once)"""
    import json
    import os
    import subprocess
    import sys
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import _hist as H, _formula as Fm, _diag as D\n"
            "a = Fm.states(13, 11, 9)[2][1]()\n"
            "out = []\n"
            "for name, f, e, m in H.specs(a):\n"
            "    t, pl = H.host_hist(Fm.grid(13, 11, 9), D.padded(a), f, e, m)\n"
            "    out.append([list(t[0].values()), t[1].tolist(), [[list(h.values()), c.tolist()] for h, c in pl]])\n"
            "print(json.dumps(out))\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                           os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for n in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMP_NUM_THREADS=n), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1]


def test_identities_with_formulas_and_diagnostics_and_the_python_entries():
    """Simulation.histogram(where="host") needs no device.  selected is f12's nonzero of the mask;
    p with edges [nextafter(0.5, 1), 1e300]: counts[0] + over is f5's ice; per_plane rows; every
    ValueError of the Python entries; RuntimeError without a resident state"""
    base = Fm.VARIABLES
    a = Fm.states(10, 10, 20)[2][1]()
    sim = P.Simulation(10, 10, 20, Fm.L, 0, P.params_array(base), initial=a, init_solver=False)
    try:
        mask = "p<0.5 and gl<0.5 and u<u_star"
        d = sim.histogram("u", 32, (200.0, 340.0), mask=mask, variables=base, where="host", per_plane=True)
        assert d["selected"] == sim.formulas({"m": mask}, variables=base, where="host")["m"]["nonzero"]
        want = H.reference([("x", "u", d["edges"], mask)], a)["x"]
        H.assert_rows(H.as_rows(d), want[0], "histogram(where='host')")
        assert d["counts"].dtype == np.int64 and d["counts_per_plane"].shape == (20, 32)
        assert (d["edges"] == np.linspace(200.0, 340.0, 33)).all()
        for k, (h, c) in enumerate(want[1]):
            assert (d["counts_per_plane"][k] == c).all()
            assert all(d[key + "_per_plane"][k] == h[key] for key in P.HIST_ROW_KEYS)
        assert d["first_row"] == 0 and H.as_rows(d["local"])[0] == H.as_rows(d)[0]
        ice = sim.histogram("p", [np.nextafter(0.5, 1.0), 1e300], where="host")
        assert ice["counts"][0] + ice["over"] == sim.diagnostics(where="host")["ice"] > 0
        inexact = sim.histogram("exp(u-u_star)", 4, (0.0, 2.0), variables=base, where="host")       # the host takes every formula
        assert inexact["selected"] == 2000
        with pytest.raises(RuntimeError, match="resident"):
            sim.histogram("u", 4, (0.0, 1.0))
        with pytest.raises(ValueError, match="where"):
            sim.histogram("u", 4, (0.0, 1.0), where="gpu")
        with pytest.raises(FE.EvalError, match="nope"):
            sim.histogram("u*nope", 4, (0.0, 1.0), where="host")
        with pytest.raises(FE.EvalError, match="nope"):
            sim.histogram("u", 4, (0.0, 1.0), mask="nope>1", where="host")
        for bins, rng in [(4, None), (0, (0.0, 1.0)), (1025, (0.0, 1.0)), (4, (1.0, 1.0)), (4, (0.0, np.inf)),
                          (4, (np.nan, 1.0)), (4, (2.0, 1.0)), (4, 3.0), ([0.0, 1.0], (0.0, 1.0)), ("four", None),
                          (np.zeros((2, 2)), None), (4, (1.0, np.nextafter(1.0, 2.0)))] + [(b, None) for b in BAD_EDGES]:
            with pytest.raises(ValueError):
                sim.histogram("u", bins, rng, where="host")
        with pytest.raises(ValueError, match="collide"):
            sim.run_series(times=[1.0], histograms={"ice": {"formula": "p", "bins": 4, "range": (0.0, 1.0)}})
        with pytest.raises(ValueError, match="not device-exact"):
            sim.run_series(times=[1.0], histograms={"h": {"formula": "u^2", "bins": 4, "range": (0.0, 1.0)}})
        with pytest.raises(ValueError, match="not device-exact"):
            sim.run_series(times=[1.0], histograms={"h": {"formula": "u", "bins": 4, "range": (0.0, 1.0), "mask": "exp(u)"}})
        with pytest.raises(ValueError, match="formula"):
            sim.run_series(times=[1.0], histograms={"h": {"bins": 4}})
        with pytest.raises(ValueError, match="unknown"):
            sim.run_series(times=[1.0], histograms={"h": {"formula": "u", "bins": 4, "range": (0.0, 1.0), "where": "p"}})
        with pytest.raises(ValueError):
            sim.run_series(times=[1.0], histograms={})
        with pytest.raises(ValueError):
            sim.run_series(times=[1.0], histograms={"h": {"formula": "u", "bins": [1.0, 1.0]}})
    finally:
        sim.close()


def test_hist_quantile_and_write_hist_txt(tmp_path):
    h = {"edges": P.hist_edges(4, (0.0, 1.0)), "counts": np.array([1, 2, 3, 4]), "under": 1, "over": 1}
    inf = float("inf")
    assert P.hist_quantile(h, 0.0) == (-inf, 0.0) and P.hist_quantile(h, 0.05) == (-inf, 0.0)
    assert P.hist_quantile(h, 0.1) == (0.0, 0.25) and P.hist_quantile(h, 0.5) == (0.5, 0.75)
    assert P.hist_quantile(h, 0.9) == (0.75, 1.0) and P.hist_quantile(h, 1.0) == (1.0, inf)
    big = {"edges": P.hist_edges(2, (0.0, 2.0)), "counts": [10 ** 17 + 1, 10 ** 17], "under": 0, "over": 0}
    assert P.hist_quantile(big, 0.5) == (0.0, 1.0) and P.hist_quantile(big, np.nextafter(0.5, 1.0)) == (1.0, 2.0)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            P.hist_quantile(h, q)
    with pytest.raises(ValueError):
        P.hist_quantile({"edges": h["edges"], "counts": [0, 0, 0, 0], "under": 0, "over": 0}, 0.5)
    rows = [{"h": np.array([1, 2, 3], dtype=np.int64)}, {"h": np.array([0, 0, 10 ** 12], dtype=np.int64)}]
    P.write_hist_txt(rows, str(tmp_path / "h.txt"), "h")
    assert (tmp_path / "h.txt").read_text() == "1 2 3\n0 0 1000000000000\n"
