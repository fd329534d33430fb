"""f6 on the host: the exact accumulator (pft_xsum_add / _combine / _round) and pft_means_host
(include/pft_means.h) against exact rational arithmetic by == -- fractions.Fraction sums rounded
once -- on arrays whose ghost cells are poisoned; merging over ragged z-ranges and thread counts
word for word."""
import ctypes as C
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _diag as D
import _means as Mn
import porousfreezethaw_amd as P

HERE = os.path.dirname(os.path.abspath(__file__))
MAX = sys.float_info.max
TINY = 5e-324


def xsum_of(values):
    acc = P.pft_xsum()
    for x in values:
        assert P.lib().pft_xsum_add(C.byref(acc), x) == 0
    return acc


def xround(acc):
    out = C.c_double(123.0)
    assert P.lib().pft_xsum_round(C.byref(acc), C.byref(out)) == 0
    return out.value


def check_round(values):
    acc = xsum_of(values)
    assert acc.as_int() == Mn.exact_units(values), values[:6]          # the words' definition
    got, want = xround(acc), Mn.exact_sum(values)
    assert Mn.same(got, want), f"{values[:6]}...: {got!r} != {want!r}"
    return got


def random_doubles(r, n, e_lo=0, e_hi=2046):
    """random sign, biased exponent in [e_lo, e_hi] (0: subnormals and zeros), random fraction"""
    bits = (r.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)) | \
           (r.integers(e_lo, e_hi, n, dtype=np.uint64, endpoint=True) << np.uint64(52)) | \
           r.integers(0, 1 << 52, n, dtype=np.uint64)
    return bits.view(np.float64).tolist()


def test_add_follows_the_definition():
    """273.15 touches words 32 and 33 only; the three digits of a value with a shift; the sign;
    +-0 adds nothing; NaN and +-Inf are refused and add nothing"""
    acc = xsum_of([273.15])
    assert [j for j, w in enumerate(acc.w) if w] == [32, 33]
    x = -float.fromhex("0x1.fffffffffffffp+100")       # E = 1123, b = 1122, c = 35, s = 2
    acc = xsum_of([x])
    T = ((1 << 53) - 1) << 2
    assert [j for j, w in enumerate(acc.w) if w] == [35, 36]
    assert (acc.w[35], acc.w[36], acc.w[37]) == (-(T & 0xffffffff), -((T >> 32) & 0xffffffff), -(T >> 64))
    x = float.fromhex("0x1.fffffffffffffp+127")        # s = 29: all three digits
    acc = xsum_of([x])
    T = ((1 << 53) - 1) << 29
    c = (1023 + 127 - 1) >> 5
    assert (acc.w[c], acc.w[c + 1], acc.w[c + 2]) == (T & 0xffffffff, (T >> 32) & 0xffffffff, T >> 64) and T >> 64
    acc = xsum_of([0.0, -0.0])
    assert not any(acc.w)
    for bad in (math.nan, math.inf, -math.inf):
        assert P.lib().pft_xsum_add(C.byref(acc), bad) == -2 and not any(acc.w)
    assert xsum_of([MAX]).w[65] and xsum_of([TINY]).w[0] == 1
    assert P.lib().pft_xsum_add(None, 1.0) == -2 and P.lib().pft_xsum_round(None, None) == -2


def test_round_random_doubles_over_every_exponent():
    r = np.random.default_rng(1)
    for e in range(0, 2047, 3):                        # single values and small sums in one binade
        vals = random_doubles(r, 3, e, e)
        check_round(vals[:1])
        check_round(vals)
    for size in (2, 5, 50, 400):                       # all exponents mixed
        for _ in range(30):
            check_round(random_doubles(r, size))
    for width in (1, 3, 40, 70):                       # neighbouring exponents: long carries, cancellation
        for _ in range(60):
            e = int(r.integers(0, 2046 - width))
            check_round(random_doubles(r, 20, e, e + width))


def test_round_subnormals_and_cancellation():
    r = np.random.default_rng(2)
    for _ in range(50):
        check_round(random_doubles(r, 30, 0, 0))       # subnormals only
        check_round(random_doubles(r, 30, 0, 2))       # across the subnormal / normal border
    assert check_round([1.0, TINY * 3, -1.0]) == TINY * 3
    assert check_round([1e308, 2.5e-310, -1e308, 1e-320]) == 2.5e-310 + 1e-320
    assert check_round([MAX, -3e-310, -MAX]) == -3e-310
    assert check_round([2.2250738585072014e-308, -TINY]) == float.fromhex("0x0.fffffffffffffp-1022")
    for vals in ([1.5, -1.5], [MAX, -MAX], [TINY, -TINY], [-0.0], [0.0, -0.0], [],
                 [1e300, 1.0, -1e300, -1.0], [-3.5, 1.25, 2.25]):
        got = check_round(vals)
        assert got == 0.0 and math.copysign(1.0, got) == 1.0          # an exact zero is +0.0


def test_round_ties_to_even():
    two53 = 2.0 ** 53
    assert check_round([two53, 1.0]) == two53                          # tie, down to even
    assert check_round([two53 + 2.0, 1.0]) == two53 + 4.0              # tie, up to even
    assert check_round([two53, 1.0, TINY]) == two53 + 2.0              # the sticky bit breaks the tie
    assert check_round([two53 + 2.0, 1.0, -TINY]) == two53 + 2.0
    assert check_round([-two53, -1.0]) == -two53
    assert check_round([-two53 - 2.0, -1.0]) == -two53 - 4.0
    assert check_round([-two53, -1.0, -TINY]) == -two53 - 2.0
    assert check_round([2.0 ** 54 - 2.0, 1.0]) == 2.0 ** 54            # the rounding carries into the next binade
    # every position of the rounding bit within a 32-bit digit, and across digits
    for e in range(60, 200, 7):
        x = 2.0 ** e
        check_round([x, x * 2.0 ** -53])
        check_round([x + x * 2.0 ** -52, x * 2.0 ** -53])
        check_round([x, x * 2.0 ** -53, TINY])
        check_round([x + x * 2.0 ** -52, x * 2.0 ** -53, -TINY])
    # in the subnormal range every sum of doubles is exact
    assert check_round([TINY, TINY, TINY]) == 3 * TINY


def test_round_dbl_max_pairs_and_overflow():
    half_ulp = 2.0 ** 970
    assert check_round([MAX, MAX, -MAX]) == MAX
    assert check_round([-MAX, -MAX, MAX]) == -MAX
    assert check_round([MAX, MAX]) == math.inf
    assert check_round([-MAX, -MAX]) == -math.inf
    assert check_round([MAX, half_ulp]) == math.inf                    # the tie rounds to the even 2^1024
    assert check_round([MAX, np.nextafter(half_ulp, 0.0)]) == MAX
    assert check_round([-MAX, -half_ulp]) == -math.inf
    assert check_round([-MAX, -half_ulp, TINY]) == -MAX
    assert check_round([MAX] * 1000 + [-MAX] * 999 + [1.0]) == MAX
    assert check_round([MAX] * 1000) == math.inf


def test_xsum_combine():
    r = np.random.default_rng(3)
    a, b = random_doubles(r, 40), random_doubles(r, 25)
    x, y, z = xsum_of(a), xsum_of(b), xsum_of(a + b)
    assert P.lib().pft_xsum_combine(C.byref(x), C.byref(y)) == 0
    assert list(x.w) == list(z.w) and list(z.w) == list(xsum_of(b + a).w)
    assert P.lib().pft_xsum_combine(None, C.byref(y)) == -2


SHAPES = [(7, 5, 3), (13, 11, 9), (3, 1, 20)]


@pytest.mark.parametrize("n1,n2,n3", SHAPES)
def test_means_host_equals_fraction(n1, n2, n3):
    a = D.random_state(n1, n2, n3, 31)
    total, _ = Mn.check_host(a)
    assert total.n[0] == n1 * n2 * n3 and 0 < total.n[2] < total.n[0]
    Mn.check_host(a, opts=(0.7, 0.25))
    Mn.check_host(Mn.wide_state(n1, n2, n3, 32))
    Mn.check_host(Mn.special(a, 33))
    Mn.check_host(Mn.special(Mn.wide_state(n1, n2, n3, 34), 35))


def test_strict_thresholds_and_empty_sums():
    """p == 0.5 is not ice, gl == 0.5 is not pore; a sum nothing entered has n 0 and a NaN mean"""
    a = np.zeros((3, 4, 3, 5))
    a[0] = 280.0
    a[1] = 0.5
    a[2] = 0.5
    total, planes = Mn.check_host(a)
    d = Mn.record_dict(total, planes)
    assert (d["ice_u_n"], d["pore_p_n"], d["ice_u_sum"], d["pore_p_sum"]) == (0, 0, 0.0, 0.0)
    assert math.isnan(d["ice_u_mean"]) and math.isnan(d["pore_p_mean"]) and np.isnan(d["ice_u_profile"]).all()
    assert d["u_mean"] == 280.0 and d["p_mean"] == 0.5 and d["u_n"] == 60
    a[1, 1] = np.nextafter(0.5, 1.0)
    a[2, 2] = np.nextafter(0.5, 0.0)
    total, planes = Mn.check_host(a)
    d = Mn.record_dict(total, planes)
    assert (d["ice_u_n"], d["pore_p_n"]) == (15, 15) and d["ice_u_mean"] == 280.0 and d["pore_p_mean"] == 0.5
    assert [not math.isnan(x) for x in d["ice_u_profile"]] == [False, True, False, False]
    total, _ = Mn.check_host(a, opts=(0.5, 0.5 - 1e-9))
    assert total.n[3] == 0


def test_nonfinite_summands_and_masks():
    """a NaN or +-Inf summand is left out of its sum and its count, and only of those; a NaN in p
    or gl is neither ice nor pore; -0.0 is counted and adds nothing"""
    a = np.zeros((3, 2, 2, 3))
    a[0] = [[[1.0, 2.0, np.nan], [np.inf, -0.0, 4.0]], [[-np.inf, 8.0, 16.0], [32.0, 64.0, 128.0]]]
    a[1] = [[[1.0, np.nan, 1.0], [1.0, 1.0, 0.0]], [[1.0, np.inf, -np.inf], [-0.0, 0.75, 1.0]]]
    a[2] = [[[0.0, 0.0, 0.0], [np.nan, 0.0, 1.0]], [[0.0, 0.0, 0.0], [-np.inf, np.inf, 0.0]]]
    total, planes = Mn.check_host(a)
    d = Mn.record_dict(total, planes)
    # u: NaN, +Inf, -Inf left out (9 of 12 enter); ice: p > 0.5 -- the NaN p is not, +Inf is
    assert (d["u_n"], d["u_sum"]) == (9, 255.0)
    assert (d["ice_u_n"], d["ice_u_sum"]) == (5, 1.0 - 0.0 + 8.0 + 64.0 + 128.0)
    # p: NaN, +Inf, -Inf left out; pore: gl < 0.5 -- the NaN gl is not, -Inf is, +Inf is not
    assert (d["p_n"], d["p_sum"]) == (9, 6.75)
    assert (d["pore_p_n"], d["pore_p_sum"]) == (6, 1.0 + 1.0 + 1.0 + 1.0 - 0.0 + 1.0)
    assert math.copysign(1.0, Mn.record_dict(Mn.check_host(np.full((3, 2, 2, 2), -0.0))[0])["u_sum"]) == 1.0
    total, _ = Mn.check_host(np.full((3, 2, 2, 2), np.nan))
    assert list(total.n) == [0, 0, 0, 0] and not any(total.words())


def test_combine_over_ragged_z_ranges():
    """slabs of 2, 5 and 2 planes merged == the one-slab record, word for word; the slabs' plane
    records side by side are the one slab's"""
    n1, n2, n3 = 13, 11, 9
    for a in (D.random_state(n1, n2, n3, 41), Mn.special(Mn.wide_state(n1, n2, n3, 42), 43)):
        one, one_planes = Mn.host_means(D.grid(n1, n2, n3), D.padded(a))
        merged, planes = P.pft_means(), []
        for lo, hi in ((7, 9), (0, 2), (2, 7)):           # any order
            part = np.ascontiguousarray(a[:, lo:hi])
            rec, pl = Mn.host_means(D.grid(n1, n2, hi - lo), D.padded(part))
            assert P.lib().pft_means_combine(C.byref(merged), C.byref(rec)) == 0
            planes.append((lo, pl))
        Mn.assert_words(merged, one, "ragged slabs merged")
        for lo, pl in planes:
            for k, m in enumerate(pl):
                Mn.assert_words(m, one_planes[lo + k], f"plane {lo + k}")
        sums = P.pft_means()
        for m in one_planes:
            P.lib().pft_means_combine(C.byref(sums), C.byref(m))
        Mn.assert_words(sums, one, "the planes' records summed")
    assert P.lib().pft_means_combine(None, C.byref(one)) == -2


def test_bad_arguments():
    g = D.grid(3, 2, 2)
    w = D.padded(np.zeros((3, 2, 2, 3)))
    assert P.lib().pft_means_host(C.byref(g), P._dp(w), None, None, None) == -2
    assert P.lib().pft_means_host(None, P._dp(w), None, C.byref(P.pft_means()), None) == -2
    g.n3 = 0
    assert P.lib().pft_means_host(C.byref(g), P._dp(w), None, C.byref(P.pft_means()), None) == -2


_OMP_WORKER = """
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {here!r})
import _diag as D, _means as Mn
a = Mn.special(Mn.wide_state(13, 11, 9, 52), 53)
a[0, :4] = D.random_state(13, 11, 9, 51)[0, :4]
total, planes = Mn.host_means(D.grid(13, 11, 9), D.padded(a))
print(total.words(), [m.words() for m in planes])
"""


def test_result_does_not_depend_on_the_thread_count():
    """the same words with OMP_NUM_THREADS=1 and =4 (the runtime reads it at start: two processes)"""
    code = _OMP_WORKER.format(repo=os.path.dirname(HERE), here=HERE)
    outs = []
    for threads in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMP_NUM_THREADS=threads),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) > 1000
