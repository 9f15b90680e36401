"""The SAC flavor without a GPU: the numpy restatement (sac_ref.py) keeps its own books, obeys detailed balance on a
system small enough to enumerate and recovers a two-peak spectrum; the C ABI validates its arguments before it looks
for a device; the Python helpers (kernels, covariance rotation, select_theta, the window rule)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import sac_ref as S


def _ladder(Nt, Nd, Nw, thetas, seed, win=1, rate=0):
    rng = np.random.RandomState(seed)
    K = rng.uniform(0.0, 1.0, (Nw, Nt))
    g = rng.uniform(0.2, 0.8, Nt)
    w = rng.uniform(2.0, 6.0, Nt)
    R = len(thetas)
    lad = S.Ladder(g, w, K, 1.0, thetas, [seed + r for r in range(R)], [S.default_positions(Nd, Nw)] * R, win)
    lad.set_exchange(rate)
    return lad


def test_lane_sum_is_the_butterfly_of_64_lanes():
    """against the header's words, lane by lane, for one to four values per lane and a tail"""
    rng = np.random.RandomState(1)
    for n in (1, 5, 64, 65, 130, 256):
        t = rng.standard_normal(n) * 10.0 ** rng.randint(-8, 8, n)
        pad = np.concatenate([t, np.zeros(-n % 64)])
        p = [0.0] * 64
        for l in range(64):
            p[l] = pad[l]
            for i in range(l + 64, len(pad), 64):
                p[l] = p[l] + pad[i]
        for off in (32, 16, 8, 4, 2, 1):
            p = [p[l] + p[l ^ off] for l in range(64)]
        assert len(set(p)) == 1 and S.lane_sum(t) == p[0], n


def test_running_residual_and_chi2_agree_with_a_rebuild():
    """after a run with exchange and without refresh, res and chi2 rebuilt from x differ from the running values by
    rounding only; with refresh on, by no more than the drift the run reports"""
    lad = _ladder(70, 9, 40, [1.0, 0.5, 0.25], 11, win=6, rate=2)
    lad.sweep(60, 1, 10, 0)
    for r in range(lad.R):
        res, chi2 = lad.rebuild(lad.x[r])
        assert np.abs(res - lad.res[r]).max() < 1e-12 and abs(chi2 - lad.chi2[r]) < 1e-10 * max(1.0, chi2)
    assert max(lad.drift) == 0.0
    lad.sweep(61, 61, 10, 5)  # the last sweep, 121, is not a refresh: the running values have moved on since sweep 120
    assert 0.0 < max(lad.drift) < 1e-10
    lad.sweep(4, 122, 10, 5)  # sweep 125 ends with a refresh
    for r in range(lad.R):
        res, chi2 = lad.rebuild(lad.x[r])
        assert np.array_equal(res, lad.res[r]) and chi2 == lad.chi2[r]
    assert sum(int(h.sum()) for h in lad.hist) == lad.R * lad.Nd * (125 - 10)


def test_detailed_balance_on_sixteen_states():
    """Nw = 4, Nd = 2, Nt = 3, theta = 1.5, window 1: 24200 sweeps, the 16 ordered states (x_0, x_1) counted after every
    sweep past 200.  Against exp(-chi2 / 2 theta) / Z.  The counts are correlated in time, so the error of a frequency is
    taken from 40 blocks of 600 sweeps; the largest deviation over the 16 states of the committed seed is below 4 of
    those standard deviations (16 two-sided tests at 4 sigma: 0.1 % to fail by chance)."""
    lad = _ladder(3, 2, 4, [1.5], 2024, win=1)
    n, burn, blocks = 24200, 200, 40
    visits = np.zeros(n - burn, dtype=np.int64)
    for i in range(1, n + 1):
        lad.sweep(1, i)
        if i > burn:
            visits[i - burn - 1] = 4 * lad.x[0][0] + lad.x[0][1]
    weight = np.array([math.exp(-lad.rebuild(np.array(s))[1] / (2.0 * 1.5)) for s in itertools.product(range(4), repeat=2)])
    exact = weight / weight.sum()
    per_block = np.stack([np.bincount(b, minlength=16) / len(b) for b in np.split(visits, blocks)])
    freq, err = per_block.mean(axis=0), per_block.std(axis=0, ddof=1) / math.sqrt(blocks)
    assert exact.min() > 0.01, "every state is visited often enough for a normal error"
    z = np.abs(freq - exact) / err
    print("largest deviation %.2f sigma" % z.max())
    assert z.max() < 4.0


# DESIGN.md, "SAC": over six seeds the lower peak's position is off by 0.10 .. 0.15 (the short run leaves weight between
# the peaks) and the upper one's by at most 0.03; 0.25 leaves the spread of the lower one (0.05) twice over as margin
TWO_PEAK_TOL = 0.25


def test_two_peak_spectrum_is_recovered():
    """two Gaussian peaks at -1.5 and 1.0 (weights 0.4, 0.6, width 0.25) on the fermion kernel, beta = 4, noise 1e-3 on
    G(tau): the weight is exact by construction; the first moment of each half (omega < -0.25, omega > -0.25) of the
    sampled spectrum lies within TWO_PEAK_TOL of the peak's centre and each half's weight within 0.05 of the peak's"""
    pr = S.two_peak_problem()
    th = [4.0, 2.0, 1.0, 0.5]
    lad = S.Ladder(pr["G"], 1.0 / pr["error"] ** 2, pr["K"].T, 1.0, th, [77 + r for r in range(4)],
                   [S.default_positions(16, len(pr["omega"]))] * 4, 8)
    S.run(lad, 300, 700, 2, 16)
    r = 3
    A = lad.hist[r].astype(np.float64) / (700.0 * 16)
    assert abs(A.sum() - 1.0) < 1e-13
    om = pr["omega"]
    for half, centre, wt in ((om < -0.25, -1.5, 0.4), (om > -0.25, 1.0, 0.6)):
        print("peak %.1f: weight %.3f, position %.3f" % (centre, A[half].sum(), (A[half] * om[half]).sum() / A[half].sum()))
        assert abs(A[half].sum() - wt) < 0.05
        assert abs((A[half] * om[half]).sum() / A[half].sum() - centre) < TWO_PEAK_TOL
    assert lad.sum[r] / lad.n_meas[r] < lad.sum[0] / lad.n_meas[0], "the colder slot fits better"


def test_abi_validates_before_it_looks_for_a_device(mc_amd):
    """fails on a library without the dqmc_sac_* symbols"""
    from montecarlo_jl_amd import _lib
    L = _lib.lib()
    good = dict(n_problems=1, n_tau=5, n_deltas=7, n_omega=33, n_replicas=2, device_id=0, window=3)

    def create(theta=None, **kw):
        a = dict(good, **kw)
        th = None if theta is None else (C.c_double * len(theta))(*theta)
        par = _lib.SacParams(a["n_problems"], a["n_tau"], a["n_deltas"], a["n_omega"], a["n_replicas"], a["device_id"],
                             a["window"], th)
        h = C.c_void_p()
        rc = L.dqmc_sac_create(C.byref(par), C.byref(h))
        if rc == 0:
            L.dqmc_sac_destroy(h)
        return rc
    bad = [dict(n_tau=0), dict(n_tau=257), dict(n_omega=1), dict(n_omega=65536), dict(n_replicas=17), dict(n_replicas=0),
           dict(n_deltas=0), dict(n_deltas=4097), dict(n_problems=0), dict(window=0), dict(theta=[1.0, 0.0]),
           dict(theta=[-1.0, 1.0]), dict(theta=[1.0, math.nan])]
    for kw in bad:
        assert create(**kw) == _lib.ERR_INVALID, kw
        assert b"dqmc_sac_create" in L.dqmc_sac_last_error(None)
    expected = _lib.OK if mc_amd.device_count() > 0 else _lib.ERR_NO_DEVICE
    assert create() == expected and create(theta=[2.0, 1.0]) == expected
    assert create(n_tau=256, n_deltas=4096, n_omega=65535, n_replicas=16, theta=[1.0] * 16) == expected
    assert L.dqmc_sac_set_exchange(None, 1) == _lib.ERR_INVALID and L.dqmc_sac_reset_accumulators(None) == _lib.ERR_INVALID


def test_kernels_against_closed_forms(mc_amd):
    K = mc_amd.fermion_kernel
    tau, beta = np.array([0.0, 0.3, 2.0, 5.0]), 5.0
    big = np.array([400.0])                      # beta omega = 2000: exp(-tau omega), and 1 / (1 + 0)
    assert np.allclose(K(tau, big, beta)[:, 0], np.exp(-tau * 400.0), rtol=1e-15, atol=0.0)
    neg = K(tau, -big, beta)[:, 0]               # exp(-(beta - tau) |omega|): finite, 1 at tau = beta
    assert np.all(np.isfinite(neg)) and np.allclose(neg, np.exp(-(beta - tau) * 400.0), rtol=1e-15, atol=0.0)
    om = np.linspace(-3.0, 3.0, 13)
    assert np.allclose(K(tau, om, beta), S.fermion_kernel(tau, om, beta), rtol=1e-14)
    assert np.allclose(K([0.0], om, beta) + K([beta], om, beta), 1.0, rtol=1e-15)   # G(0) + G(beta) = 1
    B = mc_amd.boson_symmetric_kernel
    omp = np.array([0.0, 0.5, 3.0, 400.0])
    assert np.allclose(B(tau, omp, beta), B(beta - tau, omp, beta), rtol=1e-15)
    assert np.allclose(B([0.0], omp, beta), 1.0) and np.allclose(B(tau, [0.0], beta), 1.0)
    assert np.allclose(B(tau[1:3], [400.0], beta)[:, 0], np.exp(-tau[1:3] * 400.0), rtol=1e-15, atol=0.0)
    with pytest.raises(ValueError):
        B(tau, [-1.0], beta)


def test_covariance_rotation_equals_the_direct_chi2(mc_amd):
    rng = np.random.RandomState(5)
    Nt, Nw = 6, 9
    M = rng.standard_normal((Nt, Nt))
    cov = M @ M.T + 0.1 * np.eye(Nt)
    K, G, A = rng.uniform(0, 1, (Nt, Nw)), rng.standard_normal(Nt), rng.dirichlet(np.ones(Nw))
    g, w, Kr = mc_amd.sac.rotate(G, K, cov)
    d = K @ A - G
    assert len(g) == Nt and np.isclose(np.sum(w * (Kr @ A - g) ** 2), d @ np.linalg.solve(cov, d), rtol=1e-10)
    low = cov @ np.diag([1, 1, 1, 1, 0, 0]) @ cov.T   # rank 4: two eigenvalues fall below the cut, Nt drops to 4
    g, w, Kr = mc_amd.sac.rotate(G, K, low)
    assert len(g) == len(w) == 4 and Kr.shape == (4, Nw) and np.all(np.diff(w) >= 0)


def test_select_theta_and_the_window_rule(mc_amd):
    sel, adapt = mc_amd.sac.select_theta, mc_amd.sac.adapt_window
    thetas = [8.0, 4.0, 2.0, 1.0, 0.5]
    mean = [90.0, 40.0, 26.0, 21.5, 20.5]
    lo = [60.0, 25.0, 19.0, 18.5, 18.0]          # chi2_min = 18: the bound is 18 + a sqrt(36) = 18 + 6 a
    assert sel(thetas, mean, lo, a=1.0) == 3 and sel(thetas, mean, lo, a=2.0) == 2 and sel(thetas, mean, lo, a=0.5) == 4
    assert sel(thetas, mean, lo, a=0.1) == 4     # nothing qualifies: the best fit
    assert sel(thetas[::-1], mean[::-1], lo[::-1], a=1.0) == 1   # by value of theta, not by position
    for args in ((10, 100, 70, 50), (10, 100, 30, 50), (10, 100, 50, 50), (1, 100, 10, 50), (40, 100, 90, 50), (7, 0, 0, 50)):
        assert adapt(*args) == S.adapt_window(*args)
    assert (adapt(10, 100, 70, 50), adapt(10, 100, 30, 50), adapt(10, 100, 50, 50)) == (15, 6, 10)
    assert (adapt(1, 100, 10, 50), adapt(40, 100, 90, 50)) == (1, 50)
