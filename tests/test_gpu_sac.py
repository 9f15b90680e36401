"""The SAC flavor on the MI355X (csrc/sac.hip) against the numpy restatement (sac_ref.py) with the same seeds: positions,
histograms, counters, labels, move counters, chi2, its sums and the refresh drift are equal bit for bit (a decision can
differ only through the last bit of exp, ~1e-16 per move).  The shapes are where the kernel takes another path: one to
four values per lane and lane tails (Nt), partial uniform blocks (Nd), the grid edges (Nw), one wave to sixteen (R), one
and three workgroups (P)."""
import numpy as np
import pytest

import sac_ref as S

pytestmark = pytest.mark.gpu

SEED = 9001
FIELDS = ("chi2", "sum_chi2", "sum_chi2_sq", "min_chi2", "max_drift", "n_meas", "prop", "acc", "prop_exchange",
          "acc_exchange", "replica", "moves_drawn", "rounds", "window")
# name: (Nt, Nd, Nw, R, P, sweeps, exchange rate): sweeps Nd R P stays below 5 10^4 moves
CASES = {
    "one": (1, 1, 2, 1, 1, 2000, 1),
    "tail5": (5, 7, 33, 2, 3, 500, 1),
    "full64": (64, 64, 257, 5, 1, 100, 2),
    "two65": (65, 7, 33, 16, 1, 300, 1),
    "three130": (130, 64, 257, 2, 3, 100, 1),
    "four256": (256, 64, 33, 5, 1, 100, 3),
}
REFRESH, THERM = 7, 10


def problem(Nt, Nd, Nw, R, P, seed=3):
    """random tables and data, different for every problem: K in (0, 1), G = K A + noise, errors of a few percent"""
    rng = np.random.RandomState(seed + 1000 * Nt + Nw)
    K = rng.uniform(0.0, 1.0, (Nt, Nw))
    A = rng.dirichlet(np.ones(Nw), P)
    err = rng.uniform(0.02, 0.08, (P, Nt))
    G = A @ K.T + err * rng.standard_normal((P, Nt))
    thetas = [2.0 * 0.7 ** r for r in range(R)]
    return K, G, err, thetas


def device(g, Nt, Nd, Nw, R, P, rate, win=None, thetas=None, seed=SEED, rows=None):
    K, G, err, th = problem(Nt, Nd, Nw, R, P)
    rows = list(range(P)) if rows is None else rows
    s = g.SAC(np.arange(Nt, dtype=float), G[rows], error=err[rows], kernel=K, omega=np.linspace(-1.0, 1.0, Nw),
              n_deltas=Nd, thetas=thetas or th, seed=seed, window=win or max(1, Nw // 4))
    s.set_exchange(rate)
    return s


def ladders(s, rate):
    out = []
    for p in range(s.P):
        st = [s.stats(p, r) for r in range(s.R)]
        lad = S.Ladder(s.g[p], s.w[p], s.Kt[p], s.norm[p], s.thetas[p], [s.chain_seed(p, r) for r in range(s.R)],
                       [s.conf(p, r) for r in range(s.R)], [x.window for x in st])
        lad.set_exchange(rate)
        out.append(lad)
    return out


def state(s, p, r):
    st = s.stats(p, r)
    return {f: getattr(st, f) for f in FIELDS}, s.conf(p, r).tolist(), s.histogram(p, r).tolist()


def ref_state(lad, r):
    return lad.stats(r), [int(v) for v in lad.x[r]], lad.hist[r].tolist()


def assert_equals_ref(label, s, lads):
    for p, lad in enumerate(lads):
        for r in range(s.R):
            dev, ref = state(s, p, r), ref_state(lad, r)
            assert dev == ref, (label, p, r, {k: (dev[0][k], ref[0][k]) for k in FIELDS if dev[0][k] != ref[0][k]})


def run_both(g, name, refresh=REFRESH, **kw):
    Nt, Nd, Nw, R, P, sweeps, rate = CASES[name]
    s = device(g, Nt, Nd, Nw, R, P, rate, **kw)
    try:
        lads = ladders(s, rate)
        assert_equals_ref(name + " start", s, lads)  # res and chi2 of set_conf
        s.sweep(sweeps, THERM, refresh)
        for lad in lads:
            lad.sweep(sweeps, 1, THERM, refresh)
        assert_equals_ref(name, s, lads)
        return s, lads
    except BaseException:
        s.close()
        raise


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_result_equals_the_restatement(gpu, name):
    s, lads = run_both(gpu, name)
    s.close()
    assert all(0 < lad.acc[r] < lad.prop[r] for lad in lads for r in range(lad.R)), "both outcomes of a move occur"
    if lads[0].R >= 2:
        assert any(0 < lad.xacc[0] for lad in lads), "a round has swapped"


def test_window_wider_than_the_grid_hits_both_edges(gpu):
    """win = 40 > Nw = 33: most proposals leave the grid on either side and count as rejected"""
    s, lads = run_both(gpu, "tail5", win=40)
    s.close()
    assert all(lad.acc[r] < lad.prop[r] // 2 for lad in lads for r in range(lad.R))


def test_two_equal_thetas_swap_in_every_round(gpu):
    s, lads = run_both(gpu, "tail5", thetas=[0.8, 0.8])
    st = s.stats(0, 0)
    s.close()
    assert st.prop_exchange == st.acc_exchange == (CASES["tail5"][5] + 1) // 2  # the even rounds try the pair (0, 1)


@pytest.mark.parametrize("refresh", [0, 1])
def test_refresh_never_and_after_every_sweep(gpu, refresh):
    s, lads = run_both(gpu, "two65", refresh=refresh)
    drift = max(s.stats(0, r).max_drift for r in range(s.R))
    s.close()
    assert drift == 0.0 if refresh == 0 else drift < 1e-9


def test_results_do_not_depend_on_the_split_nor_on_the_batch(gpu):
    """10 sweeps at once, 4 + 6, and problem 1 of the three alone (its own seeds): the same chains"""
    Nt, Nd, Nw, R, P, _, rate = CASES["three130"]
    a, b = device(gpu, Nt, Nd, Nw, R, P, rate), device(gpu, Nt, Nd, Nw, R, P, rate)
    c = device(gpu, Nt, Nd, Nw, R, P, rate, rows=[1], seed=SEED + 16)
    try:
        a.sweep(10, 3, 4)
        b.sweep(4, 3, 4)
        b.sweep(6, 3, 4)
        c.sweep(10, 3, 4)
        for p in range(P):
            for r in range(R):
                assert state(a, p, r) == state(b, p, r), (p, r)
        for r in range(R):
            assert state(c, 0, r) == state(a, 1, r), r
    finally:
        for s in (a, b, c):
            s.close()


def test_reset_accumulators_keeps_the_chain_and_clears_the_sums(gpu):
    Nt, Nd, Nw, R, P, _, rate = CASES["tail5"]
    s = device(gpu, Nt, Nd, Nw, R, P, rate)
    try:
        s.sweep(20, 0, 5)
        before = [state(s, 0, r) for r in range(R)]
        s.reset_accumulators()
        for r in range(R):
            st, x, hist = state(s, 0, r)
            assert x == before[r][1] and not any(hist)
            assert (st["sum_chi2"], st["sum_chi2_sq"], st["n_meas"], st["min_chi2"]) == (0.0, 0.0, 0, np.inf)
            for f in ("chi2", "prop", "acc", "prop_exchange", "acc_exchange", "replica", "moves_drawn", "max_drift"):
                assert st[f] == before[r][0][f], f
        s.sweep(5, 0, 5)
        assert s.stats(0, 0).n_meas == 5 and int(s.histogram(0, 0).sum()) == 5 * Nd
    finally:
        s.close()


def test_run_and_spectrum_equal_the_restatement(gpu):
    """SAC.run (window adaptation in chunks, exchange, refresh) and spectrum() on the two-peak problem: the same
    histogram as sac_ref.run, so the same spectrum, and the weight sums to the norm"""
    pr = S.two_peak_problem()
    th = [4.0, 2.0, 1.0, 0.5]
    s = gpu.SAC(pr["tau"], pr["G"], error=pr["error"], omega=pr["omega"], beta=pr["beta"], n_deltas=16, thetas=th,
                seed=SEED)
    try:
        lad = ladders(s, 0)[0]
        s.run(thermalization=100, sweeps=300, exchange_rate=2, refresh=16)
        S.run(lad, 100, 300, 2, 16)
        assert_equals_ref("run", s, [lad])
        for r in range(len(th)):
            sp = s.spectrum(theta=r)
            ref = lad.hist[r].astype(np.float64) * (1.0 / (300.0 * 16))
            assert np.array_equal(sp["weight"][0], ref)
            assert np.array_equal(sp["A"][0], ref / np.gradient(pr["omega"]))
            assert abs(sp["weight"][0].sum() - 1.0) < 1e-13
        sel = s.spectrum()
        assert sel["theta"][0] in th and sel["A"].shape == (1, len(pr["omega"]))
    finally:
        s.close()


def test_spectral_function_of_a_dqmc_run(gpu):
    """4x4 attractive model, a few sweeps, every momentum: shapes, and the weight of A(k, omega) is 1 for every k to the
    precision of the grid sum (Nw additions of numbers below 1: Nw 2^-53)"""
    l = gpu.SquareLattice(4)
    mc = gpu.DQMC(gpu.HubbardModelAttractive(l=l), beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=4, seed=53)
    try:
        mc.set_pair_directions(gpu.EachSitePairByDistance(l))
        mc.set_momenta("all")
        mc.set_time_displaced(2, 1)
        mc.prepare()
        with pytest.raises(gpu.DQMCError):
            mc.spectral_function(np.linspace(-6.0, 6.0, 61))  # no binner
        mc.enable_binning(("momentum_time_displaced",), capacity=8)
        for _ in range(4):
            mc.update_until_measure()
            mc.accumulate_susceptibilities(recalculate=5)
        omega = np.linspace(-6.0, 6.0, 61)
        out = mc.spectral_function(omega, n_deltas=32, thetas=[2.0, 1.0, 0.5], seed=SEED,
                                   run=dict(thermalization=50, sweeps=100))
        out["sac"].close()
        assert out["A"].shape == out["weight"].shape == (1, 16, 61)
        assert out["chi2"].shape == out["theta"].shape == (1, 16) and out["momenta"].shape == (16, 2)
        assert np.all(out["A"] >= 0.0)
        assert np.all(np.abs((out["A"] * np.gradient(omega)).sum(axis=2) - 1.0) <= 2 * 61 * 2.0 ** -53)
    finally:
        mc.close()
