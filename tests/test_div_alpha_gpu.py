"""div_alpha (pft_kernels.hip): the kernels divide by the launch constant alpha with the reciprocal's
refinement computed once per alpha instead of at every cell.  pft_div_alpha_check runs it against
the plain IEEE division on the device and counts the results whose bits differ: none may, for the
default alpha and every alpha of the published parameter sets, over 2^24 hashed bit patterns (all
exponents, both signs) and a dense list around every case v_div_scale_f64 distinguishes -- zeros,
infinities, NaNs, subnormals, |n| below 2^-969, quotients that overflow or come out subnormal."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import _oracle as O
import porousfreezethaw_amd as P
from porousfreezethaw_amd.params import default_params

pytestmark = pytest.mark.gpu

MANT = (1 << 52) - 1


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if P.device_count() < 1:
        pytest.fail("no HIP device: the gpu tests must run on an MI355X (no CPU fallback exists)")


def _published_alphas():
    """the default Params' alpha and every distinct alpha of the recorded parameter sets"""
    out = {default_params()["alpha"]}
    for path in glob.glob(os.path.join(O.GOLDEN, "*.json")):
        def walk(v):
            if isinstance(v, dict):
                for k, w in v.items():
                    if k == "alpha":
                        out.add(float.fromhex(w) if isinstance(w, str) else float(w))
                    else:
                        walk(w)
            elif isinstance(v, list):
                for w in v:
                    walk(w)
        walk(json.load(open(path)))
    return sorted(out)


def _dense(alpha):
    """numerator bit patterns: every biased exponent 0..2047 (0: zeros and subnormals, 2047:
    infinities and NaNs) with the extreme and some hashed mantissas, both signs; and 512 hashed
    mantissas at every exponent within 3 of a boundary of v_div_scale_f64's cases for this alpha:
    subnormal / normal, 2^-969 (biased 53), exponent difference 768 to alpha (quotient near
    overflow), the quotient's own overflow and its subnormal range, and the top of the range"""
    rng = np.random.default_rng(7)
    mants = np.concatenate([np.array([0, 1, 2, 1 << 51, (1 << 51) + 1, MANT, MANT - 1], dtype=np.uint64),
                            rng.integers(0, MANT + 1, 9, dtype=np.uint64)])
    exps = np.arange(2048, dtype=np.uint64)
    pats = [(exps[:, None] << np.uint64(52) | mants[None, :]).ravel()]
    ab = np.array([abs(alpha)], dtype=np.float64).view(np.uint64)[0]
    ea = int(ab >> np.uint64(52)) if np.isfinite(alpha) and alpha != 0 else 1023
    near = set()
    for c in (0, 1, 53, 54, ea + 768, ea + 1023, ea + 1024, ea - 1022, ea - 1023, ea - 1075, ea, 2046, 2047):
        near.update(e for e in range(c - 3, c + 4) if 0 <= e <= 2047)
    ne = np.array(sorted(near), dtype=np.uint64)
    pats.append((ne[:, None] << np.uint64(52) | rng.integers(0, MANT + 1, (1, 512), dtype=np.uint64)).ravel())
    p = np.concatenate(pats)
    return np.ascontiguousarray(np.concatenate([p, p | np.uint64(1 << 63)]))


def _check(alpha, n_hashed):
    L = P.lib()
    L.pft_div_alpha_check.argtypes = [C.c_double, C.c_ulonglong, C.POINTER(C.c_ulonglong), C.c_ulonglong,
                                      C.POINTER(C.c_ulonglong)]
    lst = _dense(alpha)
    bad = C.c_ulonglong(0)
    rc = L.pft_div_alpha_check(alpha, n_hashed, lst.ctypes.data_as(C.POINTER(C.c_ulonglong)), lst.size, C.byref(bad))
    assert rc == 0, (rc, L.pft_hip_last_error())
    print(f"alpha {float(alpha).hex()}: {bad.value} mismatches of {n_hashed + lst.size}")
    return bad.value


def test_published_alphas_bitwise():
    alphas = _published_alphas()
    assert default_params()["alpha"] in alphas
    assert [_check(a, 1 << 24) for a in alphas] == [0] * len(alphas)


# alphas no parameter set has, where v_div_scale_f64 scales alpha itself or the stored reciprocal
# is formed from alpha's mantissa: powers of two, the ends of the normal range, subnormals, a sign
@pytest.mark.parametrize("alpha", [1.0, 3.0, float.fromhex("0x1.fffffffffffffp+0"), -4167460.0, 1e-300, 1e300,
                                   float.fromhex("0x1p-1022"), float.fromhex("0x1.fffffffffffffp+1023"),
                                   5e-324, float.fromhex("0x0.8p-1022"), float.fromhex("0x1.8p+1000"),
                                   float.fromhex("0x1.8p-1000")])
def test_other_alphas_bitwise(alpha):
    assert _check(alpha, 1 << 20) == 0
