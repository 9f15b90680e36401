"""Sign reweighting on the CPU: the numpy restatement of sign_ref.py against closed forms, the package's host-side
jackknife against it, and the signs of the golden fields that test_gpu_sign.py relies on (no GPU)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_move_ref as ref  # noqa: E402
import sign_ref as S  # noqa: E402

# the walkers test_gpu_sign.py takes from tests/golden/logdet_sizes.json and the products of their block signs
GOLDEN_SIGNS = {"triangular8": ((2, 3, 4, 12), (-1, 1, 1, -1)),
                "triangular10": ((0, 2, 3, 4), (1, -1, 1, -1)),
                "triangular16": ((0, 64, 71, 73), (1, -1, -1, -1))}


def test_weighted_sums_closed_form():
    # x[t, w, e] = (t + 1) (w + 1) + e, s = (-1)^(t + w): sum_t,w s (t + 1)(w + 1) = (sum_t (-1)^t (t + 1)) (sum_w ...)
    T, W, E = 4, 3, 2
    x = np.array([[[(t + 1) * (w + 1) + e for e in range(E)] for w in range(W)] for t in range(T)], dtype=float)
    s = np.array([[(-1) ** (t + w) for w in range(W)] for t in range(T)])
    acc, ssum, kept, left = S.weighted_sums(x, s)
    at, aw = sum((-1) ** t * (t + 1) for t in range(T)), sum((-1) ** w * (w + 1) for w in range(W))
    assert ssum == 0 and kept == T * W and left.tolist() == [0, 0, 0]  # sum_t (-1)^t = 0
    assert acc.tolist() == [at * aw, at * aw + 0.0]  # (the e term goes with sum s = 0)
    with pytest.raises(ZeroDivisionError):
        S.signed_mean(x, s)


def test_all_positive_is_the_plain_mean_bit_for_bit():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 4, 7))
    acc, ssum, kept, _ = S.weighted_sums(x, np.ones((6, 4), dtype=int))
    plain = np.zeros(7)
    for t in range(6):
        for w in range(4):
            plain += x[t, w]
    assert acc.tobytes() == plain.tobytes() and ssum == kept == 24


def test_a_zero_sign_is_left_out_and_counted():
    x = np.ones((3, 2, 1))
    x[1, 0, 0] = np.nan  # what a singular A2 may leave behind: must not reach the sum
    s = np.array([[1, -1], [0, 1], [1, 1]])
    acc, ssum, kept, left = S.weighted_sums(x, s)
    assert acc.tolist() == [3.0] and ssum == 3.0 and kept == 5 and left.tolist() == [1, 0]
    assert S.signed_mean(x, s).tolist() == [1.0]
    sx, sw = S.walker_sums(x, s)
    assert sx.tolist() == [[2.0], [1.0]] and sw.tolist() == [2.0, 1.0]  # the left-out sample is (0, 0) in both sums


def test_jackknife_closed_forms(mc_amd):
    from montecarlo_jl_amd.dqmc import jackknife_ratio
    # every walker has the same ratio c: all delete-one ratios equal c, the error is 0
    sw = np.array([3.0, -1.0, 2.0, 5.0])
    sx = 0.75 * sw[:, None] * np.ones((1, 3))
    for f in (S.jackknife_ratio, jackknife_ratio):
        r, e = f(sx, sw)
        assert np.allclose(r, 0.75, rtol=0, atol=1e-15) and np.allclose(e, 0, atol=1e-15)
    # sw = 1 for every walker: the ratio is the mean over walkers and the jackknife error its standard error
    rng = np.random.default_rng(11)
    sx = rng.standard_normal((5, 4))
    for f in (S.jackknife_ratio, jackknife_ratio):
        r, e = f(sx, np.ones(5))
        assert np.allclose(r, sx.mean(axis=0), rtol=1e-14)
        assert np.allclose(e, sx.std(axis=0, ddof=1) / math.sqrt(5), rtol=1e-12)
    # two walkers, worked by hand: totals (sx, sw) = (4, 2); without walker 0: 3 / 3, without walker 1: 1 / -1
    r, e = jackknife_ratio(np.array([[1.0], [3.0]]), np.array([-1.0, 3.0]))
    assert r.tolist() == [2.0] and e.tolist() == [math.sqrt(0.5 * 2.0)]  # r_w = (1, -1), mean 0: (1/2)(1 + 1)
    # the package's function against the restatement on mixed signs
    sx, sw = rng.standard_normal((6, 9)), np.array([4.0, -2.0, 6.0, 2.0, -4.0, 8.0])
    a, b = jackknife_ratio(sx, sw), S.jackknife_ratio(sx, sw)
    assert np.allclose(a[0], b[0], rtol=1e-14) and np.allclose(a[1], b[1], rtol=1e-12)


def test_jackknife_refuses_what_it_cannot_do(mc_amd):
    from montecarlo_jl_amd.dqmc import jackknife_ratio
    for f in (S.jackknife_ratio, jackknife_ratio):
        with pytest.raises(ValueError):
            f(np.ones((1, 2)), np.ones(1))            # one walker
        with pytest.raises(ValueError):
            f(np.ones((2, 2)), np.array([1.0, -1.0]))  # the signs cancel
        with pytest.raises(ValueError):
            f(np.ones((3, 2)), np.array([1.0, -1.0, 2.0]))  # they cancel once walker 2 is left out


def test_walker_sums_feed_the_jackknife():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((8, 3, 2))
    s = rng.choice([-1, 1, 1], size=(8, 3))
    sx, sw = S.walker_sums(x, s)
    r, _ = S.jackknife_ratio(sx, sw)
    assert np.allclose(r, S.signed_mean(x, s), rtol=1e-13)


@pytest.mark.parametrize("name", sorted(GOLDEN_SIGNS))
def test_golden_cases_hold_both_signs(name):
    case = ref.load_golden()["logdet"][name]
    seeds, want = GOLDEN_SIGNS[name]
    assert tuple(case["seeds"]) == seeds
    prod = S.sign_products(case)
    assert tuple(int(p) for p in prod) == want
    assert (prod > 0).any() and (prod < 0).any()


def test_the_attractive_control_is_all_positive():
    case = ref.load_golden()["logdet"]["square16_attractive"]
    assert (np.array(case["sign"]) == 1).all()
