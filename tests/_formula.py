"""Helpers of the f12 formula-diagnostics tests (tests/test_formula_host.py,
tests/test_formula_gpu.py): the formula set, and the independent reference -- frontend.Evaluator
evaluated node by node in Python with the node coordinates formed as the driver forms them
(intertrack.c:1958-1971), the sums as fractions.Fraction rounded once (tests/_means.py), min, max
and maxabs from numpy with the record's NaN and signed-zero rules.  Never the code under test."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import _diag as D
import _means as Mn
import porousfreezethaw_amd as P
from porousfreezethaw_amd import frontend as FE
from porousfreezethaw_amd import params as PR

INPUTS = P.FORMULA_INPUTS
VARIABLES = {k: float(v) for k, v in PR.default_params().items()}     # the default Params' values
L = (VARIABLES["L1"], VARIABLES["L2"], VARIABLES["L3"])

# the formula set F of the issue, by its numbers
F = {
    "f1": "p>0.5",
    "f2": "gl<0.5",
    "f3": "u",
    "f4": "(p>0.5)*u",
    "f5": "p<0.5 and gl<0.5 and u<u_star",
    "f6": "p>0.5 and z>L3/2",
    "f7": "(x-L1/2)^2+(y-L2/2)^2 < (L1/3)^2 and p>0.5",
    "f8": "(water_cp*water_rho*(1-p)+ice_cp*ice_rho*p)*(1-gl)*(u-u_star)",
    "f9": "tanh((u-u_star)/10)",
    "f10": "sqrt(u-300)",
    "f11": "1/(gl-gl)",
}
CALLS = [dict(list(F.items())[:8]), dict(list(F.items())[8:])]      # all of F in two calls of <= 8
DEEP = "u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+(u+p))))))))))))))))"    # a stack of 18
NOT_EXACT = {"e1": "exp(u-u_star)", "e2": "u^2", "e3": "u C 2", "e4": DEEP}
KEYS = ("cells", "n", "nonzero", "nonfinite", "min", "max", "maxabs", "sum", "mean")


def grid(n1, n2, n3, nprocs=1, rank=0):
    """D.grid with the default Params' lengths"""
    g = D.grid(n1, n2, n3, nprocs, rank)
    g.L1, g.L2, g.L3 = L
    return g


def evaluator(variables=VARIABLES):
    ev = FE.Evaluator()
    for k, v in variables.items():
        ev.define(k, v)
    for k in INPUTS:
        ev.define(k, 0.5)
    return ev


def node_values(formulas, a, first_row=0, total_n3=None, variables=VARIABLES):
    """{name: values[n3][n2][n1]}: each formula by frontend.Evaluator at every node of the interior
    state a[3][n3][n2][n1] (global rows first_row ..); a math error gives 0 there"""
    _, n3, n2, n1 = a.shape
    total_n3 = n3 if total_n3 is None else total_n3
    ev = evaluator(variables)
    tokens = {name: ev.parse(expr) for name, expr in formulas.items()}
    slot = {k: ev._var(k) for k in INPUTS}            # the variables' entries: their value is [3]
    out = {name: np.zeros((n3, n2, n1)) for name in formulas}
    for k in range(n3):
        _z = (0.5 + k + first_row) / total_n3
        slot["_z"][3], slot["z"][3] = _z, L[2] * _z
        for j in range(n2):
            _y = (0.5 + j) / n2
            slot["_y"][3], slot["y"][3] = _y, L[1] * _y
            for i in range(n1):
                _x = (0.5 + i) / n1
                slot["_x"][3], slot["x"][3] = _x, L[0] * _x
                slot["u"][3], slot["p"][3], slot["gl"][3] = float(a[0, k, j, i]), float(a[1, k, j, i]), float(a[2, k, j, i])
                for name, tk in tokens.items():
                    try:
                        out[name][k, j, i] = ev.run(tk)
                    except FE.EvalError:        # the evaluator's own math error, nothing else
                        out[name][k, j, i] = 0.0
    return out


def _key(x):
    """orders every non-NaN double as the double orders, -0.0 below +0.0"""
    return (x, math.copysign(1.0, x))


def reduce_values(v):
    """the dict pft_fdiag.as_dict gives for the values v (any shape)"""
    v = np.asarray(v, dtype=np.float64).ravel()
    fin = v[np.isfinite(v)]
    num = [float(x) for x in v[~np.isnan(v)]]
    n, t = int(fin.size), Mn.exact_units(fin.tolist())
    return {"cells": int(v.size), "n": n, "nonzero": int(np.count_nonzero(v != 0)), "nonfinite": int(v.size - n),
            "min": min(num, key=_key) if num else math.inf, "max": max(num, key=_key) if num else -math.inf,
            "maxabs": max((abs(x) for x in num), default=0.0),
            "sum": Mn.rounded(Fraction(t, Mn.UNIT)), "mean": Mn.rounded(Fraction(t, n * Mn.UNIT)) if n else math.nan}


def reference(formulas, a, first_row=0, total_n3=None, variables=VARIABLES):
    """{name: (slab dict, [plane dicts])}"""
    vals = node_values(formulas, a, first_row, total_n3, variables)
    return {name: (reduce_values(v), [reduce_values(v[k]) for k in range(v.shape[0])]) for name, v in vals.items()}


_REF = {}


def cached_reference(tag, formulas, make_state):
    """reference(formulas, make_state()) computed once per tag and shared by the tests that need it"""
    key = (tag, tuple(formulas))
    if key not in _REF:
        _REF[key] = reference(formulas, make_state())
    return _REF[key]


def assert_dict(got, want, what=""):
    for k in KEYS:
        assert Mn.same(got[k], want[k]), f"{what}: {k}: {got[k]!r} != {want[k]!r}"


def assert_words(got, want, what=""):
    a, b = got.words(), want.words()
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert not bad, f"{what}: words {bad[:8]} differ: {[a[i] for i in bad[:8]]} != {[b[i] for i in bad[:8]]}"


def host_formulas(g, w, formulas, variables=VARIABLES, per_plane=True):
    """pft_formula_host -> (names, total records, plane records [f][k] or None)"""
    names, lens, ops, args = P.formula_programs(formulas, variables)
    total = (P.pft_fdiag * len(names))()
    planes = (P.pft_fdiag * (len(names) * g.n3))() if per_plane else None
    rc = P.lib().pft_formula_host(C.byref(g), P._dp(w), len(names), P._ip(lens), P._ip(ops), P._dp(args), total, planes)
    assert rc == 0, rc
    split = None if planes is None else [[planes[f * g.n3 + k] for k in range(g.n3)] for f in range(len(names))]
    return names, total, split


class Compiled:
    """the formulas compiled for the device against grid g (pft_formula_compile); codes: each one's code"""

    def __init__(self, g, formulas, variables=VARIABLES):
        self.names, lens, ops, args = P.formula_programs(formulas, variables)
        self.progs = (P.pft_ic_prog * len(self.names))()
        self.codes, off = [], 0
        for f, n in enumerate(lens):
            o, a = ops[off:off + n].copy(), args[off:off + n].copy()
            self.codes.append(P.lib().pft_formula_compile(C.byref(g), int(n), P._ip(o), P._dp(a), C.byref(self.progs[f])))
            off += int(n)

    def free(self):
        for pr in self.progs:
            P.lib().pft_ic_prog_free(C.byref(pr))


def states(n1, n2, n3):
    """the three kinds of state of the tests: (tag, maker)"""
    return [("random", lambda: D.random_state(n1, n2, n3, 61)),
            ("wide", lambda: Mn.wide_state(n1, n2, n3, 62)),
            ("special", lambda: Mn.special(D.random_state(n1, n2, n3, 61), 63))]
