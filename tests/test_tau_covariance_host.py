"""The tau-tau' covariance without a GPU: the ABI surface, the pooling of dqmc.tau_covariance_from_moments against
numpy.cov, its invariance under the per-walker shifts and under a split of the walkers over ranks, the partial bin, why
the shift is part of the definition (series near 1 with fluctuations of 1e-8), and the bins-against-slices condition of
a continuation with the full covariance."""
import ctypes as C
import re

import numpy as np
import pytest

import tau_covariance_ref as T

FUNCTIONS = ("dqmc_set_tau_covariance", "dqmc_tau_covariance_plan", "dqmc_tau_covariance_get", "dqmc_user_covariance",
             "dqmc_user_covariance_push", "dqmc_user_covariance_plan", "dqmc_user_covariance_get")
W, S, R = 3, 4, 6


def fill(samples, bin_size, walkers=None):
    """the restatement fed `samples` [T, W, S, R] (of the walkers given) -> its moments"""
    x = samples if walkers is None else samples[:, walkers]
    acc = T.Accumulator(x.shape[1], x.shape[2], x.shape[3], bin_size)
    for s in x:
        acc.push(s)
    return acc.moments()


def samples(n=11, seed=2):
    rng = np.random.RandomState(seed)
    z = rng.standard_normal((n, W, S, R))
    return 0.3 + 0.1 * (z + 0.7 * np.roll(z, 1, axis=3)) + 0.05 * rng.standard_normal((1, W, 1, 1))


def stacked(x, bin_size):
    b = T.bin_means(x, bin_size)
    return b.reshape((-1,) + b.shape[2:])  # every walker's bins as one sample


def test_binding_has_the_functions_and_null_handles_are_refused(mc_amd):
    from montecarlo_jl_amd import _lib
    for f in FUNCTIONS:
        assert f in _lib.SIGNATURES, f
        assert hasattr(C.CDLL(_lib.LIB_PATH), f)
    lib = _lib.lib()
    plan = (C.c_int64 * 5)(7, 7, 7, 7, 7)
    assert lib.dqmc_set_tau_covariance(None, 1, 3) == _lib.ERR_INVALID
    assert lib.dqmc_tau_covariance_plan(None, plan) == _lib.ERR_INVALID and list(plan) == [7] * 5
    assert lib.dqmc_tau_covariance_get(None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.dqmc_user_covariance(None, 1, 1, 1) == _lib.ERR_INVALID
    assert lib.dqmc_user_covariance_push(None, None) == _lib.ERR_INVALID
    assert lib.dqmc_user_covariance_get(None, None, None, None, None) == _lib.ERR_INVALID
    for name in ("set_tau_covariance", "tau_covariance_plan", "tau_covariance_moments", "tau_covariance",
                 "dynamical_structure_factor", "user_covariance", "user_covariance_push", "user_covariance_result"):
        assert callable(getattr(mc_amd.DQMC, name))


@pytest.mark.parametrize("bin_size", [1, 2, 3])
def test_pooling_equals_numpy_cov_of_all_bin_means(mc_amd, bin_size):
    """np.cov of the stacked bin means divided by n_bins; 11 samples leave a partial bin for bin_size 2 and 3.  Both
    sides are float64 sums of O(0.1) terms: 1e-13 relative to the largest entry"""
    x = samples()
    out = mc_amd.tau_covariance_from_moments(fill(x, bin_size))
    b = stacked(x, bin_size)
    assert out["n_bins"] == b.shape[0] == W * (11 // bin_size)
    for s in range(S):
        ref = np.cov(b[:, s, :], rowvar=False) / b.shape[0]
        assert np.abs(out["cov"][s] - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.abs(out["mean"][s] - b[:, s, :].mean(axis=0)).max() <= 1e-14
        assert np.array_equal(out["cov"][s], out["cov"][s].T)


def test_pooling_does_not_depend_on_the_shifts(mc_amd):
    """the same bins described from other shifts c' = c + e: S1' = S1 - nb e, S2' = S2 - e S1^T - S1 e^T + nb e e^T"""
    m = fill(samples(), 2)
    rng = np.random.RandomState(4)
    e = 0.2 * rng.standard_normal(m["shift"].shape)
    nb = m["nb"][:, None, None]
    other = dict(m, shift=m["shift"] + e, S1=m["S1"] - nb * e,
                 S2=m["S2"] - e[..., :, None] * m["S1"][..., None, :] - m["S1"][..., :, None] * e[..., None, :]
                 + nb[..., None] * e[..., :, None] * e[..., None, :])
    a, b = mc_amd.tau_covariance_from_moments(m), mc_amd.tau_covariance_from_moments(other)
    assert np.abs(a["mean"] - b["mean"]).max() <= 1e-14
    assert np.abs(a["cov"] - b["cov"]).max() <= 1e-12 * np.abs(a["cov"]).max()  # (the shifts are now off by 0.2)


def test_two_ranks_combine_to_the_single_rank_result(mc_amd):
    x = samples()
    one = mc_amd.tau_covariance_from_moments(fill(x, 2))
    two = mc_amd.tau_covariance_from_moments([fill(x, 2, [0]), fill(x, 2, [1, 2])])
    assert one["n_bins"] == two["n_bins"]
    # the same pairwise updates in the same order: the same bits
    assert np.array_equal(one["mean"], two["mean"]) and np.array_equal(one["cov"], two["cov"])
    swapped = mc_amd.tau_covariance_from_moments([fill(x, 2, [1, 2]), fill(x, 2, [0])])
    assert np.abs(one["cov"] - swapped["cov"]).max() <= 1e-13 * np.abs(one["cov"]).max()


def test_a_partial_bin_is_left_out(mc_amd):
    x = samples(7)
    full, cut = fill(x, 3), fill(x[:6], 3)
    assert list(full["nb"]) == [2] * W
    for k in ("shift", "S1", "S2"):
        assert np.array_equal(full[k], cut[k]), k
    wild = x.copy()
    wild[6] = 1e6  # the open bin's sample is part of no result
    assert np.array_equal(fill(wild, 3)["S2"], full["S2"])
    with pytest.raises(ValueError):
        mc_amd.tau_covariance_from_moments(fill(x[:2], 3))  # no closed bin at all


@pytest.mark.parametrize("bin_size", [1, 3])
def test_the_shift_is_what_keeps_the_digits(mc_amd, bin_size):
    """mean 1, fluctuations 1e-8: the shifted moments give the np.longdouble covariance to within what the float64
    bin means allow (tau_covariance_ref.near_one_tolerance), and the un-shifted textbook formula, fed the same bin
    means, misses it by more than a thousand times that: its S2 / n - m m^T cancels sixteen digits"""
    x = T.near_one_samples(12, W, S, R)
    out = mc_amd.tau_covariance_from_moments(fill(x, bin_size))
    mean, ref = T.covariance_of_mean(stacked(x, bin_size).astype(np.longdouble))
    tol = T.near_one_tolerance(x, bin_size)
    err = np.abs(out["cov"] - ref).astype(np.float64)
    assert np.all(err <= tol), (err / tol).max()
    assert tol.max() < 1e-6 * np.abs(ref).max()  # the tolerance is a rounding bound, not a loose one
    assert np.abs(out["mean"] - mean).max() <= 4 * T.EPS
    miss = np.abs(T.textbook_covariance_of_mean(stacked(x, bin_size)) - ref).astype(np.float64)
    assert miss.max() > 1e3 * tol.max() and miss.max() > 0.1 * np.abs(ref).max().astype(np.float64)


def test_too_few_bins_for_the_slices_are_refused(mc_amd):
    """n_bins <= R: the covariance of R slices from n_bins bins is singular by construction"""
    from montecarlo_jl_amd import _lib
    for n_bins, n_tau in ((0, 1), (3, 3), (10, 11), (11, 11)):
        with pytest.raises(mc_amd.DQMCError) as e:
            mc_amd.check_covariance_bins(n_bins, n_tau)
        assert e.value.code == _lib.ERR_STATE
    mc_amd.check_covariance_bins(12, 11)
    mc_amd.check_covariance_bins(2, 1)


def test_header_declares_the_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dqmc_hip.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(\s*dqmc_handle\s*\*h\b" % f, src), f
