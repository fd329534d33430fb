"""Helpers of the f13 histogram tests (tests/test_hist_host.py, tests/test_hist_gpu.py): the specs,
the states, and the independent reference -- the formulas evaluated node by node by tests/_formula.py's
evaluator, selected and counted by numpy.histogram with explicit edges and numpy comparisons.  Never
the code under test.  Every comparison is == on integers."""
import ctypes as C

import numpy as np

import _diag as D
import _formula as Fm
import porousfreezethaw_amd as P

HEAD_KEYS = ("cells", "selected", "nan", "under", "over")
IRREGULAR = np.array([-40.0, -10.0, -1.0, 0.0, 1e-3, 5.0, 10.0, 40.0])        # 7 bins, an edge at 0.0
SUPERCOOLED = "p<0.5 and gl<0.5"
Z_MASK = "z>L3/2"                                                             # deselects whole planes


def specs(a):
    """the specs of the issue for the interior state a: (name, formula, edges, mask)"""
    u = a[0][np.isfinite(a[0])]
    lo, hi = max(float(u.min()), -1e300), min(float(u.max()), 1e300)          # (a span that linspace can divide)
    if not lo < hi:
        lo, hi = lo - 1.0, hi + 1.0
    return [("u64", "u", P.hist_edges(64, (lo, hi)), None),
            ("p1024", "p", P.hist_edges(1024, (0.0, 1.0)), None),
            ("u1", "u", P.hist_edges(1, (250.0, 300.0)), None),
            ("heat7", "(u-u_star)*gl", P.hist_edges(IRREGULAR), SUPERCOOLED),
            ("u16z", "u", P.hist_edges(16, (200.0, 340.0)), Z_MASK)]


def one_bin_state(n1, n2, n3):
    """every cell the same: the wave's aggregated path alone"""
    a = np.empty((3, n3, n2, n1))
    a[0], a[1], a[2] = 293.15, 0.0, 1.0
    return a


def ramp_state(n1, n2, n3):
    """u = the flat index mod 1024 (+ 0.5): in 1024 bins over (0, 1024) every lane of a wave falls
    into another bin -- the per-lane path alone"""
    a = one_bin_state(n1, n2, n3)
    a[0] = (np.arange(n1 * n2 * n3) % 1024 + 0.5).reshape(n3, n2, n1)
    return a


RAMP = ("ramp1024", "u", np.linspace(0.0, 1024.0, 1025), None)


def edges_state(n1, n2, n3, edges=IRREGULAR, seed=71):
    """a random state whose u holds every edge, both neighbouring doubles of every edge, +-0.0,
    +-Inf and NaN (edges must hold 0.0), spread over the cells"""
    a = D.random_state(n1, n2, n3, seed)
    vals = []
    for e in edges:
        vals += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
    vals += [0.0, -0.0, np.inf, -np.inf, np.nan]
    flat = a[0].reshape(-1)
    assert flat.size >= len(vals)
    at = np.linspace(0, flat.size - 1, len(vals)).astype(int)
    assert len(set(at)) == len(vals)
    flat[at] = vals
    return a


EDGES = ("uedges", "u", IRREGULAR, None)


def states(n1, n2, n3):
    """(tag, maker, extra specs): the states of _formula.states and this file's own"""
    out = [(tag, make, []) for tag, make in Fm.states(n1, n2, n3)]
    out += [("one_bin", lambda: one_bin_state(n1, n2, n3), []),
            ("ramp", lambda: ramp_state(n1, n2, n3), [RAMP]),
            ("edges", lambda: edges_state(n1, n2, n3), [EDGES])]
    return out


def np_rows(values, selected, edges):
    """(head dict, counts) of numpy for values / selected of any one shape"""
    values, selected = np.asarray(values, dtype=np.float64).ravel(), np.asarray(selected, dtype=bool).ravel()
    v = values[selected]
    w = v[~np.isnan(v)]
    with np.errstate(invalid="ignore"):
        counts = np.histogram(w, bins=edges)[0].astype(np.int64)
        head = {"cells": int(values.size), "selected": int(v.size), "nan": int(v.size - w.size),
                "under": int((w < edges[0]).sum()), "over": int((w > edges[-1]).sum())}
    assert head["selected"] == head["nan"] + head["under"] + head["over"] + int(counts.sum())
    return head, counts


def reference(spec_list, a, first_row=0, total_n3=None, variables=Fm.VARIABLES):
    """{name: ((head, counts), [(head, counts) per plane])} by tests/_formula.py's evaluator and numpy"""
    formulas = {}
    for _, f, _, m in spec_list:
        formulas[f] = f
        if m is not None:
            formulas[m] = m
    vals = Fm.node_values(formulas, a, first_row, total_n3, variables)
    out = {}
    for name, f, edges, m in spec_list:
        v = vals[f]
        sel = np.ones(v.shape, dtype=bool) if m is None else vals[m] != 0          # (a NaN is "true")
        out[name] = (np_rows(v, sel, edges), [np_rows(v[k], sel[k], edges) for k in range(v.shape[0])])
    return out


def programs(formula, mask, variables=Fm.VARIABLES):
    """((ops, args) of the value, (ops, args) of the mask or None)"""
    _, _, vops, vargs = P.formula_programs({"f": formula}, variables)
    if mask is None:
        return (vops, vargs), None
    _, _, mops, margs = P.formula_programs({"m": mask}, variables)
    return (vops, vargs), (mops, margs)


def host_hist(g, w, formula, edges, mask, variables=Fm.VARIABLES, per_plane=True):
    """pft_hist_host -> ((head, counts), planes or None), as reference() gives them"""
    (vops, vargs), m = programs(formula, mask, variables)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    nbins = edges.size - 1
    value = P.pft_hist_prog(len(vops), P._ip(vops), P._dp(vargs))
    mk = None if m is None else C.byref(P.pft_hist_prog(len(m[0]), P._ip(m[0]), P._dp(m[1])))
    head, counts = P.pft_hist_head(), (C.c_longlong * nbins)()
    ph = (P.pft_hist_head * g.n3)() if per_plane else None
    pc = (C.c_longlong * (g.n3 * nbins))() if per_plane else None
    rc = P.lib().pft_hist_host(C.byref(g), P._dp(w), C.byref(value), mk, nbins, P._dp(edges), C.byref(head), counts, ph, pc)
    assert rc == 0, rc
    return rows_of(head, counts, ph, pc, g.n3, nbins)


def rows_of(head, counts, plane_heads, plane_counts, n3, nbins):
    """ctypes outputs -> ((head dict, counts array), [per plane] or None)"""
    total = (head.as_dict(), np.array(counts[:], dtype=np.int64))
    if plane_heads is None:
        return total, None
    pc = np.array(plane_counts[:], dtype=np.int64).reshape(n3, nbins)
    return total, [(plane_heads[k].as_dict(), pc[k]) for k in range(n3)]


def assert_rows(got, want, what=""):
    """(head dict, counts) pairs equal: every integer by =="""
    for k in HEAD_KEYS:
        assert got[0][k] == want[0][k], f"{what}: {k}: {got[0][k]} != {want[0][k]}"
    assert got[1].shape == want[1].shape, what
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, f"{what}: bins {bad[:8]}: {got[1][bad[:8]]} != {want[1][bad[:8]]}"


def assert_all(got, want, what=""):
    """(total, planes) equal: the slab's rows and every plane's"""
    assert_rows(got[0], want[0], what)
    assert len(got[1]) == len(want[1]), what
    for k, (g, w) in enumerate(zip(got[1], want[1])):
        assert_rows(g, w, f"{what} plane {k}")


def as_rows(d):
    """histogram()'s dict -> (head dict, counts)"""
    return ({k: d[k] for k in HEAD_KEYS}, d["counts"])


def planes_of(d):
    """histogram(per_plane=True)'s dict -> [(head dict without cells, counts)]; cells is not reported per plane"""
    n = d["counts_per_plane"].shape[0]
    return [({k: int(d[k + "_per_plane"][i]) for k in HEAD_KEYS[1:]}, d["counts_per_plane"][i]) for i in range(n)]
