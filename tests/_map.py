"""Helpers of the f15 map tests (tests/test_map_host.py, tests/test_map_gpu.py): the specs, the
states, and the independent reference -- the formulas as numpy expressions of the fields (or, for
formulas with coordinates, evaluated node by node by tests/_formula.py's evaluator), reduced along the
axis by numpy's sum, argmax, max and min.  Never the code under test.  Every comparison is == on
integers and on the bits of the doubles."""
import ctypes as C

import numpy as np

import _diag as D
import _formula as Fm
import porousfreezethaw_amd as P

KEYS = P.MAP_KEYS
ICE = "p>0.5"
SUPERCOOLED = "p<0.5 and gl<0.5"
# the specs of the issue: (name, formula, mask)
SPECS = [("ice", ICE, None), ("warm", "u", ICE), ("cold", "u_star-u", SUPERCOOLED)]
# ... and two with coordinates, so that the tables of every axis are indexed: x and y in the value, z in the mask
COORD_SPECS = [("upper", "u", "z>L3/2"), ("disc", "(x-L1/2)^2+(y-L2/2)^2 < (L1/3)^2 and p>0.5", None)]


def _b(x):
    return x.astype(np.float64)


def field_values(formula, a, variables=Fm.VARIABLES):
    """the formulas of SPECS as numpy sees them: comparisons give 0.0 / 1.0 and are false on a NaN, `and`
    is true where both sides are != 0, the subtraction is one IEEE operation"""
    u, p, gl = a
    with np.errstate(invalid="ignore"):
        return {ICE: lambda: _b(p > 0.5), "u": lambda: u.copy(), "p": lambda: p.copy(),
                "u_star-u": lambda: variables["u_star"] - u,
                SUPERCOOLED: lambda: _b((p < 0.5) & (gl < 0.5)),
                "u-u": lambda: u - u}[formula]()


def values(formula, a, first_row=0, total_n3=None, variables=Fm.VARIABLES):
    try:
        return field_values(formula, a, variables)
    except KeyError:
        return Fm.node_values({"f": formula}, a, first_row, total_n3, variables)["f"]


def np_map(v, sel, axis, first_row=0):
    """numpy's map of the values v[n3][n2][n1] over the cells sel, reduced along axis; first / last
    along z count from first_row"""
    v = np.moveaxis(np.asarray(v, dtype=np.float64), axis, 0)
    sel = np.moveaxis(np.asarray(sel, dtype=bool), axis, 0)
    n = v.shape[0]
    nz = sel & (v != 0)                                   # (a NaN is "true")
    some = nz.any(axis=0)
    off = first_row if axis == 0 else 0
    valid = sel & ~np.isnan(v)
    zero = valid & (v == 0)
    with np.errstate(invalid="ignore"):
        mx = np.max(np.where(valid, v, -np.inf), axis=0)
        mn = np.min(np.where(valid, v, np.inf), axis=0)
    # -0.0 < +0.0: a maximum of zero is +0.0 when there is one, a minimum of zero -0.0 when there is one
    mx = np.where(mx == 0, np.where((zero & ~np.signbit(v)).any(axis=0), 0.0, -0.0), mx)
    mn = np.where(mn == 0, np.where((zero & np.signbit(v)).any(axis=0), -0.0, 0.0), mn)
    return {"selected": sel.sum(axis=0).astype(np.int64), "nonzero": nz.sum(axis=0).astype(np.int64),
            "nonfinite": (sel & ~np.isfinite(v)).sum(axis=0).astype(np.int64), "min": mn, "max": mx,
            "first": np.where(some, np.argmax(nz, axis=0) + off, -1).astype(np.int64),
            "last": np.where(some, n - 1 - np.argmax(nz[::-1], axis=0) + off, -1).astype(np.int64)}


def reference(formula, mask, a, axis, first_row=0, total_n3=None, variables=Fm.VARIABLES):
    v = values(formula, a, first_row, total_n3, variables)
    sel = np.ones(v.shape, dtype=bool) if mask is None else values(mask, a, first_row, total_n3, variables) != 0
    return np_map(v, sel, axis, first_row)


def assert_map(got, want, what=""):
    """maps equal: every integer by ==, every double bit for bit"""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{what}: {k}: shape {g.shape} != {w.shape}"
        if k in ("min", "max"):
            g, w = np.ascontiguousarray(g, dtype=np.float64).view(np.int64), np.ascontiguousarray(w, dtype=np.float64).view(np.int64)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {k} at {bad[:4].tolist()}: {np.asarray(got[k])[tuple(bad[0])]!r} != {np.asarray(want[k])[tuple(bad[0])]!r}"


def as_dict(rec, cols):
    """flat MAP_DTYPE records -> {key: 2-D array}"""
    a = rec.reshape(-1, cols)
    return {k: np.ascontiguousarray(a[k]) for k in KEYS}


def dims(g, axis):
    r, c = C.c_int(), C.c_int()
    assert P.lib().pft_map_dims(C.byref(g), axis, C.byref(r), C.byref(c)) == 0
    return r.value, c.value


def hist_prog(ops, args):
    return P.pft_hist_prog(len(ops), P._ip(ops), P._dp(args))


def programs(formula, mask, variables=Fm.VARIABLES):
    """((ops, args) of the value, (ops, args) of the mask or None)"""
    _, _, vops, vargs = P.formula_programs({"f": formula}, variables)
    if mask is None:
        return (vops, vargs), None
    _, _, mops, margs = P.formula_programs({"m": mask}, variables)
    return (vops, vargs), (mops, margs)


def host_map(g, w, formula, mask, axis, variables=Fm.VARIABLES):
    """pft_map_host -> {key: 2-D array}"""
    v, m = programs(formula, mask, variables)
    rows, cols = dims(g, axis)
    out = np.empty(rows * cols, dtype=P.MAP_DTYPE)
    rc = P.lib().pft_map_host(C.byref(g), P._dp(w), C.byref(hist_prog(*v)), None if m is None else C.byref(hist_prog(*m)),
                              axis, P._map_ptr(out))
    assert rc == 0, rc
    return as_dict(out, cols)


def pattern_state(n1, n2, n3, seed):
    """random bit patterns: every double, NaN of every payload, +-Inf, subnormals and both zeros in u;
    p and gl as random_state's with the special values sprinkled in"""
    r = np.random.default_rng(seed)
    a = D.random_state(n1, n2, n3, seed)
    a[0] = r.integers(0, 1 << 64, size=(n3, n2, n1), dtype=np.uint64).view(np.float64)
    flat = a.reshape(3, -1)
    n = flat.shape[1]
    for q in range(3):
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0):
            flat[q, r.integers(0, n, size=max(1, n // 16))] = v
    return a


def dense_state(n1, n2, n3, seed):
    """a state as the model makes it: u near the freezing point, an ice body below a wavy front, pores"""
    r = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(n3), np.arange(n2), np.arange(n1), indexing="ij")
    front = n3 * (0.5 + 0.3 * np.sin(1.0 + i / max(n1, 1) * 5.0) * np.cos(j / max(n2, 1) * 4.0))
    a = np.empty((3, n3, n2, n1))
    a[1] = np.clip(0.5 + (front - k) * 0.75, 0.0, 1.0)
    a[0] = 273.15 + (k - front) * 0.5 + 0.01 * r.standard_normal((n3, n2, n1))
    a[2] = r.choice([0.0, 0.0, 0.0, 1.0], size=(n3, n2, n1))
    return a


def states(n1, n2, n3):
    return [("pattern", lambda: pattern_state(n1, n2, n3, 91)), ("dense", lambda: dense_state(n1, n2, n3, 92)),
            ("random", lambda: D.random_state(n1, n2, n3, 93))]
