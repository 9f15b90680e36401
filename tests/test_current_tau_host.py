"""Host side of the imaginary-time current recording, no GPU: dqmc.CurrentTauSums and dqmc.matsubara_trapezoid on
synthetic per-walker sums against the plain restatements of tests/current_tau_ref.py, and the row restatement itself
against the literal 2N x 2N cc_kernel of tests/cc_reference.py.

Bounds: the jackknife against the closed delete-one formula and the transform of a tau-constant row at m >= 1 to 1e-13
(of the error's / the row's magnitude) as the feature's specification sets them; both sides are float64 sums of fewer than
a hundred terms of that magnitude."""
import numpy as np
import pytest

import cc_reference as CC
import current_tau_ref as CT


def synthetic(W, R, K, nq, seed, signs=None):
    """[W, P] sums of `calls` samples per walker; signs: per-walker s_w (0: left out), None: unsigned"""
    rng = np.random.default_rng(seed)
    calls = 4
    out = []
    for w in range(W):
        s = 1.0 if signs is None else float(signs[w])
        C = -rng.uniform(0.2, 1.0, (R, K, nq)) * calls * s
        S = rng.uniform(-0.5, 0.5, (R, K, nq)) * calls * s
        kb = -rng.uniform(0.5, 1.5, K) * calls * s
        out.append(CT.pack(C, S, kb, calls * s, calls if s else 0, 0 if s else calls))
    return np.array(out)


@pytest.mark.parametrize("W", [2, 3, 6])
def test_jackknife_against_the_closed_delete_one_formula(mc_amd, W):
    R, K, nq = 5, 3, 2
    sums = synthetic(W, R, K, nq, 10 + W)
    ct = mc_amd.CurrentTauSums(sums, R, K, nq)
    assert ct.count == 4 * W and ct.left_out == 0
    res = ct.estimate(lambda C, S, kb: {"all": np.concatenate([C.ravel(), S.ravel(), kb])})
    val, err = CT.jackknife_closed(sums[:, :-3], sums[:, -3])
    bval, berr = CT.jackknife(sums[:, :-3], sums[:, -3])
    assert err.min() > 0
    assert np.abs(res["all"] - val).max() <= 1e-13 * np.abs(val).max()
    assert np.abs(res["all_std_error"] - err).max() <= 1e-13 * err.max()
    assert np.abs(berr - err).max() <= 1e-13 * err.max() and np.abs(bval - val).max() <= 1e-13 * np.abs(val).max()
    # a nonlinear function goes through the jackknife as a function of the ratio
    g = lambda v: np.exp(v[:3]) / (1.0 + v[3] ** 2)
    res = ct.estimate(lambda C, S, kb: {"g": g(C.ravel())})
    gv, ge = CT.jackknife(sums[:, :-3], sums[:, -3], g)
    assert np.abs(res["g"] - gv).max() <= 1e-13 * np.abs(gv).max() and np.abs(res["g_std_error"] - ge).max() <= 1e-13 * ge.max()


def test_one_walker_has_no_error_bar_and_bad_input_is_refused(mc_amd):
    sums = synthetic(1, 3, 2, 2, 5)
    res = mc_amd.CurrentTauSums(sums, 3, 2, 2).estimate(lambda C, S, kb: {"C": C, "k": kb})
    assert sorted(res) == ["C", "k"] and res["C"].shape == (3, 2, 2)
    assert np.array_equal(res["k"], sums[0, 24:26] / 4.0)
    with pytest.raises(ValueError):
        mc_amd.CurrentTauSums(sums[:, :-1], 3, 2, 2)
    zero = synthetic(2, 3, 2, 2, 5, signs=[1, -1])
    with pytest.raises(ValueError, match="sum of signs is 0"):
        mc_amd.CurrentTauSums(zero, 3, 2, 2, could_leave_out=True).estimate(lambda C, S, kb: {"C": C})


def test_signed_ratio_with_a_left_out_walker(mc_amd):
    """signs + - 0 + +: the zero-sign walker adds nothing and is counted; two walkers are too few once one can be left out"""
    R, K, nq, signs = 4, 2, 3, [1, -1, 0, 1, 1]
    sums = synthetic(5, R, K, nq, 77, signs=signs)
    assert not sums[2, :-1].any() and sums[2, -1] == 4
    ct = mc_amd.CurrentTauSums(sums, R, K, nq, could_leave_out=True)
    assert ct.count == 16 and ct.left_out == 4
    res = ct.estimate(lambda C, S, kb: {"C": C, "S": S, "kb": kb, "z": C[:, 0, :] - 1j * S[:, 0, :]})
    val, err = CT.jackknife(sums[:, :-3], sums[:, -3])
    n = R * K * nq
    assert np.abs(res["C"].ravel() - val[:n]).max() <= 1e-13 * np.abs(val).max()
    assert np.abs(res["S_std_error"].ravel() - err[n:2 * n]).max() <= 1e-13 * err.max()
    assert np.abs(res["kb_std_error"] - err[2 * n:]).max() <= 1e-13 * err.max()
    assert np.abs(res["z_std_error_re"] - res["C_std_error"][:, 0, :]).max() <= 1e-13 * err.max()
    assert np.abs(res["z_std_error_im"] - res["S_std_error"][:, 0, :]).max() <= 1e-13 * err.max()
    # the ratio is the mean of x itself where every sample of a walker carries its sign: s_w (s_w x) / s_w^2
    two = mc_amd.CurrentTauSums(sums[:2], R, K, nq, could_leave_out=True)
    with pytest.raises(ValueError, match="sum of signs is 0"):
        two.estimate(lambda C, S, kb: {"C": C})
    pair = mc_amd.CurrentTauSums(sums[[0, 3]], R, K, nq, could_leave_out=True).estimate(lambda C, S, kb: {"C": C})
    assert "C_std_error" not in pair
    assert "C_std_error" in mc_amd.CurrentTauSums(sums[[0, 3]], R, K, nq).estimate(lambda C, S, kb: {"C": C})


@pytest.mark.parametrize("R", [5, 11, 21])
def test_matsubara_transform(mc_amd, R):
    beta = 2.0
    h = beta / (R - 1)
    tau = np.arange(R) * h
    n_max = (R - 1) // 2
    rng = np.random.default_rng(R)
    const = np.broadcast_to(rng.uniform(0.5, 2.0, (1, 3, 2)), (R, 3, 2)).copy()
    omega = 2.0 * np.pi * np.arange(n_max + 1) / beta
    out = mc_amd.matsubara_trapezoid(const, tau, omega)
    assert out.shape == (n_max + 1, 3, 2)
    assert np.abs(out[0] - beta * const[0]).max() <= 1e-13 * np.abs(const).max() * beta
    assert np.abs(out[1:]).max() <= 1e-13 * np.abs(const).max()  # a tau-constant row has no weight at m >= 1
    lam = rng.uniform(-1, 1, (R, 3, 2)) + 1j * rng.uniform(-1, 1, (R, 3, 2))
    om, ref = CT.matsubara(lam, h, beta, n_max)
    assert np.array_equal(om, omega)
    assert np.abs(mc_amd.matsubara_trapezoid(lam, tau, omega) - ref).max() <= 1e-13 * np.abs(lam).max() * beta
    # cos(omega_1 tau) itself: beta / 2 at m = 1, nothing elsewhere (exact for the trapezoid rule on a full period)
    c1 = mc_amd.matsubara_trapezoid(np.cos(omega[1] * tau), tau, omega)
    want = np.zeros(n_max + 1)
    want[1] = beta / 2
    if R > 3:
        assert np.abs(c1 - want).max() <= 1e-13 * beta
    with pytest.raises(ValueError):
        mc_amd.matsubara_trapezoid(lam[:-1], tau, omega)


@pytest.mark.parametrize("attractive", [True, False])
def test_row_restatement_against_the_literal_kernel(mc_amd, attractive):
    """CT.row on random block matrices against cc_reference._slice_sum on the 2N x 2N ones, square 4 x 4, and the
    delta_tau sum of rows against current_current_susceptibility"""
    l = mc_amd.SquareLattice(4)
    it = mc_amd.EachLocalQuadBySyncedDistance(l)
    n, nd, nb = 16, it.pairs_by_dir.ndirections(), 1 if attractive else 2
    rng = np.random.default_rng(3 + nb)
    T = [rng.uniform(-1, 1, (n, n)) for _ in range(nb)]
    mats = lambda: [rng.uniform(-1, 1, (n, n)) for _ in range(nb)]
    g00 = mats()
    steps = [(mats(), mats(), mats()) for _ in range(3)]
    q = mc_amd.momentum_grid(l)[0][:5]
    ph = np.array(it.pairs_by_dir.directions, dtype=float) @ q.T
    Ct, St = np.cos(ph), np.sin(ph)
    dir_of = it.pairs_by_dir.dir_of
    acc = np.zeros((nd, it.K))
    for g0l, gl0, gll in steps:
        C, S, Ca, Sa, x = CT.row(T, g00, g0l, gl0, gll, dir_of, nd, it.trg_of, Ct, St)
        if attractive:
            lit = CC._slice_sum((g00[0], g0l[0], gl0[0], gll[0]), T[0], dir_of, it.trg_of, nd, True) / n
        else:
            bd = CC.blockdiag
            lit = CC._slice_sum((bd(g00), bd(g0l), bd(gl0), bd(gll)), bd(T), dir_of, it.trg_of, nd, False) / n
        assert np.abs(x - lit).max() <= 1e-12 * np.abs(lit).max()
        assert C.shape == (it.K, 5) and np.abs(C - lit.T @ Ct).max() <= 1e-12 * np.abs(C).max()
        assert np.all(np.abs(C) <= Ca) and np.all(np.abs(S) <= Sa)
        acc += x
    ref = CC.current_current_susceptibility(g00, steps, T, it, attractive, 0.1)
    assert np.abs(0.1 * acc - ref).max() <= 1e-12 * np.abs(ref).max()
    t0 = CT.row0_tuple(g00)
    assert all(np.array_equal(a, b - np.eye(n)) for a, b in zip(t0[1], g00)) and t0[2] is g00 and t0[3] is g00
    assert np.all(CT.terms(dir_of, nd, it.trg_of) == n * n + nd)
