"""The Ising flavor's binner without a GPU: the ABI surface is complete, and the numpy restatement the device is
compared with (tests/ising_binner_ref.py) is itself right - its level sums are exact on integer series, and its
delta-method error of a variance agrees with the analytic one."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ising_binner_ref import IsingBinnerRef, from_series  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dqmc_mc_binner_enable", "dqmc_mc_binner_size", "dqmc_mc_binner_reliable_level", "dqmc_mc_binner_get_level",
       "dqmc_mc_binner_finish")


def test_the_new_symbols_are_in_the_header_the_library_and_the_binding(mc_amd):
    from montecarlo_jl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dqmc_hip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\bint %s\s*\(dqmc_mc_handle \*h" % n, src), n
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert "dqmc_mc_binned;" in src
    # the struct of the binding is the header's: 4 + 4 + 4 + 4 + 2 doubles, int64, int32 (padded to 8)
    assert C.sizeof(_lib.McBinned) == 18 * 8 + 8 + 8
    # a call on no handle is an argument error, not a crash
    assert _lib.lib().dqmc_mc_binner_enable(None, 0) == _lib.ERR_INVALID
    for name in ("enable_binning", "binner_level", "binned"):
        assert hasattr(mc_amd.MC, name), name


def test_level_sums_of_an_integer_series_are_exact():
    """|E| <= 128, M <= 64, T = 1000: a level-l value is the mean of 2^l integers (l fractional bits) and every sum
    stays below 2^48, so each level sum is an exactly representable rational, whatever the order of the additions"""
    rng = np.random.default_rng(11)
    T, W = 1000, 3
    E = rng.integers(-128, 129, (T, W))
    M = rng.integers(-64, 65, (T, W))
    b = from_series(E, M, capacity=1023)
    assert b.L == 10 and b.count[0] == T
    for w in range(W):
        series = [[Fraction(int(e)), Fraction(int(e)) ** 2, Fraction(abs(int(m))), Fraction(int(m)) ** 2]
                  for e, m in zip(E[:, w], M[:, w])]
        for l in range(b.L):
            n = T >> l
            blocks = [[sum(s[k] for s in series[i << l:(i + 1) << l]) / (1 << l) for k in range(4)] for i in range(n)]
            xs, x2, xy, cnt = b.sums(w, l)
            assert cnt == n
            for k in range(4):
                for got, want in ((xs[k], sum(v[k] for v in blocks)), (x2[k], sum(v[k] ** 2 for v in blocks))):
                    assert want.numerator.bit_length() <= 53 and Fraction(float(got)) == want, (w, l, k)
            for q, (i, j) in enumerate(((0, 1), (2, 3))):
                want = sum(v[i] * v[j] for v in blocks)
                assert abs(want.numerator).bit_length() <= 53 and Fraction(float(xy[q])) == want, (w, l, q)


def test_delta_method_error_of_a_variance_matches_the_analytic_one():
    """x_t i.i.d. unit normal, pushed as the pair (x, x^2): the fluctuation <x^2> - <x>^2 is the sample variance, whose
    standard error is sqrt(2/(n - 1)).  The delta-method estimate at level l is sqrt(s_y^2 / n_l) with s_y^2 the sample
    variance of the n_l bin means of y = (x - mean)^2.  Var(y) = 2 and the fourth central moment of y (a chi-square of
    one degree of freedom) is 60; a mean of b = 2^l such values has kurtosis 3 + 12/b, so the relative variance of
    s_y^2 is (2 + 12/b)/n_l and that of its square root a quarter of it.  The bound is five of those standard
    deviations plus the O(1/n_l) bias of a variance estimate."""
    n = 4096
    x = np.random.default_rng(5).standard_normal(n)
    b = IsingBinnerRef(capacity=n)
    for v in x:
        b.push([v, v * v, 0.0, 0.0])
    analytic = math.sqrt(2.0 / (n - 1.0))
    value, _ = b.fluctuation(0, 1.0, 0, level=0)
    assert abs(value - x.var()) <= 1e-12
    for level in (0, 2, 4):
        n_l, bins = n >> level, float(1 << level)
        _, var = b.fluctuation(0, 1.0, 0, level=level)
        bound = 5.0 * 0.5 * math.sqrt((2.0 + 12.0 / bins) / n_l) + 4.0 / n_l
        assert abs(math.sqrt(var) / analytic - 1.0) <= bound, (level, math.sqrt(var), analytic, bound)
