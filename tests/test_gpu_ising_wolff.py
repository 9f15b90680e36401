"""The Ising flavor's Wolff cluster move on the MI355X (ising_wolff_kernel, dqmc_mc_global_move): bit-exact against the
restatement of sweep + move + run!'s measurement rule (ising_wolff_ref.py) on every lattice family, exact single moves
from set_conf states, independence of the batch and the split, the distribution against exact enumeration, and the
decorrelation that is the move's purpose."""
import numpy as np
import pytest

import ising_wolff_ref as R
from test_gpu_ising import _exact_4x4

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("sum_E", "sum_E2", "sum_absM", "sum_M2", "n_meas", "acc_local", "prop_local", "uniforms_used",
               "energy", "magnetization")
GLOBAL_FIELDS = ("prop_global", "acc_global", "sum_cluster_size", "moves_drawn")
BETA_C = 0.5 * np.log(1.0 + np.sqrt(2.0))


def _stats(mc, w):
    st = mc.stats(w)
    return {f: getattr(st, f) for f in STAT_FIELDS}


def _gstats(mc, w):
    g = mc.global_stats(w)
    return {f: getattr(g, f) for f in GLOBAL_FIELDS}


@pytest.mark.parametrize("r", [1, 3, 5])
@pytest.mark.parametrize("name,make", [
    ("square8", lambda g: g.SquareLattice(8)),
    ("chain10", lambda g: g.Chain(10)),
    ("cubic4", lambda g: g.CubicLattice(3, 4)),
    ("triangular4", lambda g: g.TriangularLattice(4)),
    ("triangular6", lambda g: g.TriangularLattice(6)),
])
def test_sweeps_with_cluster_moves_match_the_restatement_bit_exactly(gpu, name, make, r):
    l = make(gpu)
    therm, sweeps, rate, seed, cap = 5, 26, 2, 4321, 20
    betas = [0.15, 0.3, 0.44, 0.7]
    mc = gpu.MC(gpu.IsingModel(l=l), beta=betas, n_walkers=len(betas), seed=seed, thermalization=therm, sweeps=sweeps,
                measure_rate=rate, cluster_moves=True, global_rate=r, series_capacity=cap)
    splits = (4, 1, 11, therm + sweeps - 16)
    for n in splits:
        mc.sweep(n)
    for w, b in enumerate(betas):
        ref = R.Walker(l, b, seed + w, series_capacity=cap)
        ref.run(1, therm + sweeps, therm, rate, r)
        assert _stats(mc, w) == ref.stats(), (name, r, w)
        assert _gstats(mc, w) == ref.gs, (name, r, w)
        assert ref.gs["prop_global"] == (therm + sweeps) // r
        assert np.array_equal(mc.conf(w), ref.c), (name, r, w)
        e, m = mc.series(w)
        assert list(e) == ref.serE and list(m) == ref.serM, (name, r, w)
    if name == "square8":
        assert sum(mc.global_stats(w).acc_global for w in range(len(betas))) > 0
        for w in range(len(betas)):
            c = mc.conf(w)
            st = mc.stats(w)
            assert st.energy == mc.model.energy(c) and st.magnetization == int(c.sum())
            a = mc.analysis(w)
            g = mc.global_stats(w)
            assert (a["prop_global"], a["acc_global"]) == (g.prop_global, g.acc_global)
            assert a["acc_rate_global"] == g.acc_global / g.prop_global
    mc.close()


def test_global_move_from_set_conf_states(gpu):
    """beta = 0 flips the seed site alone (not accepted); beta = 50 on the all-up state flips every site (E unchanged,
    M = -N); random states at beta_c match the restated cluster move after move, for one walker and for all"""
    l = gpu.SquareLattice(16)
    model = gpu.IsingModel(l=l)
    N = len(l)
    neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
    bonds0 = np.asarray(l.bonds, dtype=np.int64)[:, :2] - 1
    betas = [0.0, 50.0, BETA_C, 0.3, 0.6]
    W = len(betas)
    mc = gpu.MC(model, beta=betas, n_walkers=W, seed=0)
    rng = np.random.default_rng(5)
    confs = [rng.choice([-1, 1], N).astype(np.int8) for _ in range(W)]
    confs[1] = np.ones(N, dtype=np.int8)
    keys = [1000 + 17 * w for w in range(W)]
    for w in range(W):
        mc.set_conf(w, confs[w])
        mc.seed(w, keys[w])
    before0 = mc.stats(0)

    mc.global_move(0)
    seed = R.wolff_seed(keys[0], 0, N)
    c0 = confs[0].astype(np.int64)
    c0[seed] = -c0[seed]
    assert np.array_equal(mc.conf(0), c0)
    g = mc.global_stats(0)
    assert (g.prop_global, g.acc_global, g.sum_cluster_size, g.moves_drawn) == (1, 0, 1, 1)
    st = mc.stats(0)
    assert st.energy == R.energy(c0, bonds0) and st.magnetization == int(c0.sum())
    assert st.n_meas == 0 and st.uniforms_used == before0.uniforms_used  # no measurement, the local stream untouched
    for w in range(1, W):
        assert mc.global_stats(w).moves_drawn == 0

    E_up = mc.stats(1).energy
    mc.global_move(1)
    assert np.all(mc.conf(1) == -1)
    st, g = mc.stats(1), mc.global_stats(1)
    assert st.energy == E_up and st.magnetization == -N
    assert (g.acc_global, g.sum_cluster_size) == (1, N)

    ref = [R.Walker(l, b, keys[w], conf=mc.conf(w)) for w, b in enumerate(betas)]
    ref[0].gs["moves_drawn"] = 1
    ref[1].gs["moves_drawn"] = 1
    for step in range(6):
        if step % 2:
            mc.global_move(-1)
            walkers = range(W)
        else:
            mc.global_move(2)
            walkers = [2]
        for w in walkers:
            ref[w].global_move()
        for w in range(W):
            assert np.array_equal(mc.conf(w), ref[w].c), (step, w)
            st = mc.stats(w)
            assert st.energy == ref[w].E and st.magnetization == int(ref[w].c.sum()), (step, w)
            assert mc.global_stats(w).moves_drawn == ref[w].gs["moves_drawn"], (step, w)
    assert mc.global_stats(2).sum_cluster_size > 6
    # the seed resets the cursor: the same state and key give the same move again
    c2 = mc.conf(2)
    mc.seed(2, keys[2])
    mc.global_move(2)
    assert np.array_equal(mc.conf(2), R.wolff_move(c2, neighs0, keys[2], 0, R.wolff_p(BETA_C))[0])
    mc.close()


@pytest.mark.parametrize("name,make", [
    ("square128_N16384", lambda g: g.SquareLattice(128)),
    ("cubic4d_11_N14641_z8", lambda g: g.CubicLattice(4, 11)),
])
def test_the_site_ceiling(gpu, name, make):
    """the largest LDS footprint: a whole-lattice cluster (beta = 50 from all-up) and a random state near T_c"""
    l = make(gpu)
    N = len(l)
    neighs0 = np.asarray(l.neighs, dtype=np.int64) - 1
    z = neighs0.shape[0]
    beta_near = 0.45 if z == 4 else 0.15
    mc = gpu.MC(gpu.IsingModel(l=l), beta=[50.0, beta_near], n_walkers=2, seed=0)
    mc.set_conf(0, np.ones(N, dtype=np.int8))
    conf1 = np.random.default_rng(9).choice([-1, 1], N).astype(np.int8)
    mc.set_conf(1, conf1)
    mc.seed(0, 5)
    mc.seed(1, 6)
    mc.global_move(-1)
    assert np.all(mc.conf(0) == -1) and mc.global_stats(0).sum_cluster_size == N
    c, size = R.wolff_move(conf1, neighs0, 6, 0, R.wolff_p(beta_near))
    assert np.array_equal(mc.conf(1), c)
    assert mc.global_stats(1).sum_cluster_size == size
    mc.close()


def test_results_do_not_depend_on_the_batch_or_the_split(gpu):
    """walker k of a 16384-walker handle with r = 1 equals a 1-walker handle keyed with the same seed, and many short
    sweep calls equal one long one"""
    model = gpu.IsingModel(dims=2, L=8)
    seed, therm, sweeps = 2718, 10, 90
    kw = dict(beta=0.44, seed=seed, thermalization=therm, sweeps=sweeps, cluster_moves=True, global_rate=1)
    big = gpu.MC(model, n_walkers=16384, **kw)
    big.run()
    for k in (0, 1, 255, 8191, 16383):
        one = gpu.MC(model, n_walkers=1, first_walker=k, **kw)
        one.run()
        assert _stats(one, 0) == _stats(big, k), k
        assert _gstats(one, 0) == _gstats(big, k), k
        assert np.array_equal(one.conf(0), big.conf(k)), k
        one.close()
    mid = gpu.MC(model, n_walkers=300, **dict(kw, global_rate=3))
    rng = np.random.default_rng(4)
    while mid.last_sweep < therm + sweeps:
        mid.sweep(int(min(rng.integers(1, 8), therm + sweeps - mid.last_sweep)))
    whole = gpu.MC(model, n_walkers=300, **dict(kw, global_rate=3))
    whole.sweep(therm + sweeps)
    for k in (0, 63, 64, 299):
        assert _stats(mid, k) == _stats(whole, k), k
        assert _gstats(mid, k) == _gstats(whole, k), k
        assert np.array_equal(mid.conf(k), whole.conf(k)), k
    big.close()
    mid.close()
    whole.close()


@pytest.mark.parametrize("r", [1, 3])
def test_4x4_against_exact_enumeration(gpu, r):
    betas = (0.2, 0.44, 0.7)
    Wb = 512
    model = gpu.IsingModel(dims=2, L=4)
    mc = gpu.MC(model, beta=np.repeat(betas, Wb), n_walkers=3 * Wb, seed=101 + r, thermalization=200, sweeps=2000,
                cluster_moves=True, global_rate=r)
    mc.run()
    for bi, beta in enumerate(betas):
        ex = _exact_4x4(beta)
        per = {"E": [], "E2": [], "M": [], "M2": []}
        for w in range(bi * Wb, (bi + 1) * Wb):
            st = mc.stats(w)
            assert st.n_meas == 2000
            per["E"].append(st.sum_E / st.n_meas)
            per["E2"].append(st.sum_E2 / st.n_meas)
            per["M"].append(st.sum_absM / st.n_meas)
            per["M2"].append(st.sum_M2 / st.n_meas)
        assert mc.global_stats(bi * Wb).prop_global == 2200 // r
        for k, v in per.items():
            v = np.array(v)
            se = v.std(ddof=1) / np.sqrt(Wb)
            assert abs(v.mean() - ex[k]) <= 4.5 * se, (r, beta, k, v.mean(), ex[k], se)
    mc.close()


def _lag_autocorrelation(series, lag):
    """pooled normalised autocorrelation of equal-length per-walker series (rows)"""
    x = np.asarray(series, dtype=float)
    x = x - x.mean()
    return float(np.mean(x[:, :-lag] * x[:, lag:]) / np.mean(x * x))


def test_cluster_moves_decorrelate_at_beta_c(gpu):
    """L = 32 at beta_c, 256 walkers: the lag-10 autocorrelation of the |M| series is below 0.5 with a cluster move
    after every sweep and above 0.6 with the local sweep alone (measured on the MI355X: 0.02 and 0.75; the
    local-only value is a property of the Metropolis chain, which the device reproduces bit for bit)"""
    model = gpu.IsingModel(dims=2, L=32)
    W, therm, sweeps = 256, 300, 600
    rho = {}
    for cluster in (False, True):
        mc = gpu.MC(model, beta=BETA_C, n_walkers=W, seed=77, thermalization=therm, sweeps=sweeps,
                    series_capacity=sweeps, cluster_moves=cluster, global_rate=1)
        mc.run()
        ser = np.array([mc.series(w)[1] for w in range(W)])
        assert ser.shape == (W, sweeps)
        rho[cluster] = _lag_autocorrelation(ser, 10)
        if cluster:
            g = mc.global_stats(0)
            assert g.prop_global == therm + sweeps and g.sum_cluster_size > g.prop_global
        mc.close()
    assert rho[True] < 0.5, rho
    assert rho[False] > 0.6, rho


def test_observables_stay_consistent_after_moves(gpu):
    model = gpu.IsingModel(dims=2, L=16)
    W = 70
    mc = gpu.MC(model, beta=np.linspace(0.2, 0.8, W), n_walkers=W, seed=12, thermalization=0, sweeps=40,
                cluster_moves=True, global_rate=2)
    mc.run()
    mc.global_move(-1)
    for w in (0, 31, 69):
        c = mc.conf(w)
        st = mc.stats(w)
        assert st.energy == model.energy(c) and st.magnetization == int(c.sum()), w
        assert mc.global_stats(w).prop_global == 21
    mc.close()
