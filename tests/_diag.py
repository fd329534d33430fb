"""Helpers of the f5 diagnostics tests (tests/test_diag_host.py, tests/test_diag_gpu.py): the
semantics of include/pft_diag.h restated in numpy, grids and padded host arrays with poisoned
ghost cells, and field-for-field comparison of records."""
import ctypes as C

import numpy as np

import porousfreezethaw_amd as P

FIELDS = [k for k, _ in P.pft_diag._fields_]
L3 = (0.05, 0.05, 0.1)


def np_diag(a, p_thr=0.5, gl_thr=0.5):
    """(record dict, ice_per_plane) of an interior state a[3][n3][n2][n1]"""
    u, p, gl = a
    with np.errstate(invalid="ignore"):
        ice, pore = p > p_thr, gl < gl_thr       # ordered: False on NaN
    au = np.abs(u[ice])
    au = au[~np.isnan(au)]

    def lo_hi(v):
        v = v[~np.isnan(v)]
        return (float(v.min()), float(v.max())) if v.size else (np.inf, -np.inf)

    (u_min, u_max), (p_min, p_max) = lo_hi(u), lo_hi(p)
    rec = {"cells": int(u.size), "ice": int(ice.sum()), "pore": int(pore.sum()),
           "ice_pore": int((ice & pore).sum()),
           "nonfinite": int((~(np.isfinite(u) & np.isfinite(p) & np.isfinite(gl))).sum()),
           "ice_u_maxabs": float(au.max()) if au.size else 0.0,
           "u_min": u_min, "u_max": u_max, "p_min": p_min, "p_max": p_max}
    return rec, ice.sum(axis=(1, 2)).astype(np.int64)


def grid(n1, n2, n3, nprocs=1, rank=0):
    """pft_grid by pft_grid_init; a slab of one plane, which pft_grid_init refuses (every slab
    holds at least bcond_thickness planes, intertrack.c:1555-1558), is filled in by hand"""
    g = P.pft_grid()
    if n3 == 1 and nprocs == 1:
        g.n1, g.n2, g.n3, g.total_n3, g.nprocs = n1, n2, 1, 1, 1
        g.L1, g.L2, g.L3 = L3
        return g
    assert P.lib().pft_grid_init(C.byref(g), n1, n2, n3, nprocs, rank, *L3, 0) == 0
    return g


def padded(a, poison=True):
    """interior a[3][n3][n2][n1] -> the reference's padded host array; every ghost cell in x, y and
    z holds values that would change every output: p = 1 (ice), u = 1e300 or NaN, gl = -1 (pore)"""
    _, n3, n2, n1 = a.shape
    w = np.zeros((3, n3 + 4, n2 + 4, n1 + 4))
    if poison:
        w[0] = 1e300
        w[0].reshape(-1)[::3] = np.nan
        w[0].reshape(-1)[1::7] = -np.inf
        w[1] = 1.0
        w[1].reshape(-1)[::5] = np.nan
        w[2] = -1.0
    w[:, 2:2 + n3, 2:2 + n2, 2:2 + n1] = a
    return np.ascontiguousarray(w)


def host_diag(g, w, opts=None, per_plane=True):
    """pft_diag_host -> (record dict, ice_per_plane)"""
    d = P.pft_diag()
    planes = (C.c_longlong * g.n3)() if per_plane else None
    o = None if opts is None else C.byref(P.pft_diag_opts(*opts))
    rc = P.lib().pft_diag_host(C.byref(g), P._dp(w), o, C.byref(d), planes)
    assert rc == 0, rc
    return rec_of(d), (np.array(planes[:], dtype=np.int64) if per_plane else None)


def rec_of(d):
    return {k: getattr(d, k) for k in FIELDS}


def assert_same(got, want, what=""):
    """records equal field for field: counts and doubles by =="""
    for k in FIELDS:
        assert got[k] == want[k], f"{what}: {k}: {got[k]!r} != {want[k]!r}"


def random_state(n1, n2, n3, seed):
    """a smooth-ish random state with ice, pores and threshold values in it"""
    r = np.random.default_rng(seed)
    a = np.empty((3, n3, n2, n1))
    a[0] = 273.15 + 20.0 * r.standard_normal((n3, n2, n1))
    a[1] = r.choice([0.0, 0.25, 0.5, np.nextafter(0.5, 1.0), 0.75, 1.0], size=(n3, n2, n1))
    a[2] = r.choice([0.0, np.nextafter(0.5, 0.0), 0.5, 1.0], size=(n3, n2, n1))
    return a
