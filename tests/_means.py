"""Helpers of the f6 means tests (tests/test_means_host.py, tests/test_means_gpu.py): the yardstick
is exact rational arithmetic -- fractions.Fraction sums of the interior values over the common
denominator 2^1074, rounded once by float() -- never the code under test, and never math.fsum
(it raises an intermediate overflow where +-1e308 values meet)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import _diag as D
import porousfreezethaw_amd as P

KEYS = P.MEAN_KEYS
UNIT = 1 << 1074          # every finite double is an integer multiple of 2^-1074


def exact_units(values):
    """the exact sum of finite doubles as an integer number of 2^-1074 (each value through Fraction)"""
    t = 0
    for x in values:
        f = Fraction(x)
        t += f.numerator * (UNIT // f.denominator)
    return t


def rounded(fr):
    """float(Fraction): correctly rounded, ties to even; past DBL_MAX's rounding range +-Inf"""
    try:
        return float(fr)
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


def exact_sum(values):
    return rounded(Fraction(exact_units(values), UNIT))


def quantity(vals):
    """(n, sum, mean) of the finite ones among vals"""
    vals = np.asarray(vals, dtype=np.float64).ravel()
    vals = vals[np.isfinite(vals)]
    n, t = int(vals.size), exact_units(vals.tolist())
    return n, rounded(Fraction(t, UNIT)), (rounded(Fraction(t, n * UNIT)) if n else math.nan)


def ref_means(a, p_thr=0.5, gl_thr=0.5, per_plane=True):
    """the dict Simulation.means gives for an interior state a[3][n3][n2][n1]"""
    def one(u, p, gl):
        with np.errstate(invalid="ignore"):
            ice, pore = p > p_thr, gl < gl_thr       # ordered: False on NaN
        return {"u": quantity(u), "p": quantity(p), "ice_u": quantity(u[ice]), "pore_p": quantity(p[pore])}

    d = {}
    for k, (n, s, m) in one(*a).items():
        d[k + "_n"], d[k + "_sum"], d[k + "_mean"] = n, s, m
    if per_plane:
        planes = [one(a[0][z], a[1][z], a[2][z]) for z in range(a.shape[1])]
        for k in KEYS:
            d[k + "_profile"] = np.array([pl[k][2] for pl in planes])
            d[k + "_plane_n"] = [pl[k][0] for pl in planes]
    return d


def same(x, y):
    """== on doubles, with NaN equal to NaN and +0.0 different from -0.0"""
    if isinstance(x, float) or isinstance(y, float):
        x, y = float(x), float(y)
        if math.isnan(x) or math.isnan(y):
            return math.isnan(x) and math.isnan(y)
        return x == y and math.copysign(1.0, x) == math.copysign(1.0, y)
    return x == y


SCALARS = [k + s for k in KEYS for s in ("_n", "_sum", "_mean")]


def assert_scalars(got, want, what=""):
    for k in SCALARS:
        assert same(got[k], want[k]), f"{what}: {k}: {got[k]!r} != {want[k]!r}"


def assert_profiles(got, want, what=""):
    for k in KEYS:
        g, w = got[k + "_profile"], want[k + "_profile"]
        assert len(g) == len(w)
        for z, (x, y) in enumerate(zip(g, w)):
            assert same(float(x), float(y)), f"{what}: {k}_profile[{z}]: {x!r} != {y!r}"


def record_dict(total, planes=None):
    """pft_means (and per-plane records) -> the dict of Simulation.means"""
    d = total.as_dict()
    if planes is not None:
        for q, k in enumerate(KEYS):
            d[k + "_profile"] = np.array([m.values(q)[2] for m in planes])
            d[k + "_plane_n"] = [int(m.n[q]) for m in planes]
    return d


def host_means(g, w, opts=None, per_plane=True):
    """pft_means_host -> (total record, per-plane records or None)"""
    total = P.pft_means()
    planes = (P.pft_means * g.n3)() if per_plane else None
    o = None if opts is None else C.byref(P.pft_diag_opts(*opts))
    rc = P.lib().pft_means_host(C.byref(g), P._dp(w), o, C.byref(total), planes)
    assert rc == 0, rc
    return total, planes


def assert_words(got, want, what=""):
    """two pft_means records equal word for word"""
    a, b = got.words(), want.words()
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert not bad, f"{what}: words {bad[:8]} differ: {[a[i] for i in bad[:8]]} != {[b[i] for i in bad[:8]]}"


def check_host(a, opts=None):
    """pft_means_host of a (ghosts poisoned) == the Fraction results; returns the records"""
    n3, n2, n1 = a.shape[1:]
    total, planes = host_means(D.grid(n1, n2, n3), D.padded(a), opts)
    want = ref_means(a, *(opts or (0.5, 0.5)))
    got = record_dict(total, planes)
    assert_scalars(got, want, "pft_means_host against Fraction")
    assert_profiles(got, want, "pft_means_host against Fraction")
    for k in KEYS:
        assert got[k + "_plane_n"] == want[k + "_plane_n"]
    return total, planes


def wide(r, shape):
    """log-uniform over 2^-1074 .. 2^1023 (subnormals included), mixed signs"""
    x = np.ldexp(r.uniform(1.0, 2.0, size=shape), r.integers(-1074, 1023, size=shape, endpoint=True).astype(np.int32))
    x = np.minimum(x, np.finfo(np.float64).max)
    return np.where(r.random(shape) < 0.5, -x, x)


def wide_state(n1, n2, n3, seed):
    """u and p wide-exponent fields (p's sign and size make ice of about a third of the cells), gl
    as random_state's"""
    r = np.random.default_rng(seed)
    a = D.random_state(n1, n2, n3, seed)
    a[0] = wide(r, (n3, n2, n1))
    a[1] = wide(r, (n3, n2, n1))
    return a


def special(a, seed):
    """NaN, +-Inf, signed zeros, +-DBL_MAX and subnormals sprinkled into a copy of a"""
    a = a.copy()
    r = np.random.default_rng(seed)
    flat = a.reshape(3, -1)
    n = flat.shape[1]
    big = np.finfo(np.float64).max
    for q in range(3):
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, big, -big, 5e-324, -3e-310):
            flat[q, r.integers(0, n, size=max(1, n // 40))] = v
    return a


class SlabDesc(C.Structure):
    """include/pft_hip.h pft_slab_desc"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("n3", C.c_int), ("has_below", C.c_int),
                ("has_above", C.c_int), ("calc_mode", C.c_int), ("gl_static", C.c_int),
                ("eps_mult", C.c_double * 3)]


class Slab:
    """a bare pft_slab (no model, no solver): the reduction reads the buffers only"""

    def __init__(self, n1, n2, n3):
        L = P.lib()
        L.pft_slab_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(SlabDesc), C.c_void_p]
        L.pft_slab_upload_host.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.pft_slab_destroy.argtypes = [C.c_void_p]
        self.L, self.n3 = L, n3
        d = SlabDesc(n1, n2, n3, 0, 0, 0, 0, (C.c_double * 3)(1.0, 1.0, 1.0))
        consts = (C.c_double * 64)(*([1.0] * 64))     # pft_consts: doubles only, unused here
        self.s = C.c_void_p()
        rc = L.pft_slab_create(C.byref(self.s), C.byref(d), consts)
        assert rc == 0, (rc, L.pft_hip_last_error())

    def upload(self, which, w):
        assert self.L.pft_slab_upload_host(self.s, which, P._dp(w)) == 0

    def means(self, which, opts=None, per_plane=True):
        total = P.pft_means()
        planes = (P.pft_means * self.n3)() if per_plane else None
        o = None if opts is None else C.byref(P.pft_diag_opts(*opts))
        rc = self.L.pft_slab_means(self.s, which, o, C.byref(total), planes)
        assert rc == 0, (rc, self.L.pft_hip_last_error())
        return total, planes

    def close(self):
        self.L.pft_slab_destroy(self.s)
