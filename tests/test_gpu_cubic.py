"""3D Hubbard models on CubicLattice(3, L) on the device: stepwise parity with the oracle (given the cubic hopping
matrix), the three-factor Kronecker path at L = 8 (kron3.hip) against the dense path (DQMC_NO_KRON=1, read when a handle
is created), the U = 0 known answer, the measurements with K = 7 and the checkerboard decomposition.  Every factored case
asserts the path taken: a silent fallback would make the comparisons vacuous."""
import os
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_reference as CC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _model(gpu, kind, L, **kw):
    return (gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive)(L, 3, **kw)


def _oracles(O, mc, kind, exps=None):
    T = mc.model.hopping_matrix()[0]
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(mc.model.l.L, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=T, exps=exps)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


def _stepwise(mc, refs, nupd):
    def compare(conf=True):
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                assert relerr(g, g0) < TOL, relerr(g, g0)
    mc.prepare()
    for o in refs:
        o.prepare()
    compare()
    for _ in range(nupd):
        mc.propagate()
        for o in refs:
            o.propagate()
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        compare(conf=False)
        mc.sweep_spatial()
        for o in refs:
            o.sweep_spatial()
        compare()
    for w, o in enumerate(refs):
        a, st = mc.analysis(w), o.stats()
        assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
        assert mc.uniforms_used(w) == o.uniforms_used()


@pytest.mark.parametrize("kind,L,walkers", [("attractive", 4, 2), ("repulsive", 4, 2), ("attractive", 6, 2),
                                            ("repulsive", 6, 1), ("attractive", 8, 1), ("repulsive", 8, 1)])
def test_stepwise_updates_match_oracle(gpu, O, kind, L, walkers):
    """propagate / sweep_spatial one call at a time through more than a full sweep (up and down chains, both wraps) at
    beta = 1, safe_mult = 5: n = 64, n = 216 (padded paths) and n = 512 (the factored path)"""
    mc = gpu.DQMC(_model(gpu, kind, L), beta=1.0, safe_mult=5, n_walkers=walkers, seed=31)
    assert mc.kron_hopping() == (L == 8)
    _stepwise(mc, _oracles(O, mc, kind), 2 * mc.p.slices + 3)
    mc.close()


def _handle(gpu, model, dense, **kw):
    if dense:
        os.environ["DQMC_NO_KRON"] = "1"
    try:
        mc = gpu.DQMC(model, **kw)
    finally:
        os.environ.pop("DQMC_NO_KRON", None)
    assert mc.kron_hopping() == (not dense)
    return mc


@pytest.mark.parametrize("kind,walkers", [("attractive", 8), ("repulsive", 4)])
def test_factored_sweeps_match_dense_at_L8(gpu, kind, walkers):
    """prepare + two full sweeps: HS field and counters identical, G within 1e-10"""
    kw = dict(beta=2.0, n_walkers=walkers, seed=77)
    mcs = [_handle(gpu, _model(gpu, kind, 8), dense, **kw) for dense in (False, True)]
    for mc in mcs:
        mc.prepare()
        mc.update_until_measure()
        mc.sweep(2)
    f, d = mcs
    worst = 0.0
    for w in range(walkers):
        assert np.array_equal(f.conf(w), d.conf(w)), "HS field of walker %d differs" % w
        af, ad = f.analysis(w), d.analysis(w)
        assert (af.prop_local, af.acc_local) == (ad.prop_local, ad.acc_local)
        assert af.propagation_error.count == ad.propagation_error.count
        for gf, gd in zip(f.greens_eff(w), d.greens_eff(w)):
            worst = max(worst, relerr(gf, gd))
    print("%s, %d walkers: max rel |G_kron - G_dense| = %.3g" % (kind, walkers, worst))
    assert worst < TOL
    for mc in mcs:
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_wrap_greens_both_directions_match_dense_at_L8(gpu, kind):
    kw = dict(beta=2.0, n_walkers=2, seed=5)
    mcs = [_handle(gpu, _model(gpu, kind, 8), dense, **kw) for dense in (False, True)]
    for mc in mcs:
        mc.prepare()
    for sl, direction in ((7, 1), (12, -1), (20, -1), (1, 1)):
        for mc in mcs:
            mc.wrap_greens(sl, direction)
        for w in range(2):
            for gf, gd in zip(mcs[0].greens_eff(w), mcs[1].greens_eff(w)):
                e = relerr(gf, gd)
                assert e < TOL, (sl, direction, w, e)
    for mc in mcs:
        mc.close()


class _OneStrongBond:
    """HubbardModelAttractive on 8 x 8 x 8 with the bond 1 - 2 at t = 1.2: its exponentials are no Kronecker products"""

    def __init__(self, gpu):
        self._m = gpu.HubbardModelAttractive(8, 3)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def hopping_matrix(self):
        T = self._m.hopping_matrix()[0]
        T[0, 1] = T[1, 0] = -1.2
        return [T]


def test_paths_that_stay_dense(gpu):
    for model in (_OneStrongBond(gpu), _model(gpu, "attractive", 6)):
        mc = gpu.DQMC(model, beta=1.0, n_walkers=1)
        assert not mc.kron_hopping()
        mc.close()


def test_perturbed_L8_matches_oracle(gpu, O):
    model = _OneStrongBond(gpu)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=1, seed=31)
    assert not mc.kron_hopping()
    o = O.OracleDQMC(8, "attractive", beta=1.0, delta_tau=mc.p.delta_tau, safe_mult=5, U=model.U,
                     hopping=model.hopping_matrix()[0])
    o.set_conf(mc.conf(0))
    o.seed(mc.seeds[0])
    _stepwise(mc, [o], 12)
    mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_free_fermions_known_answer(gpu, kind):
    """U = 0: the HS field drops out, G = (I + exp(-beta T))^-1 whatever the field"""
    model = _model(gpu, kind, 4, U=0.0)
    beta = 2.0
    mc = gpu.DQMC(model, beta=beta, n_walkers=2, seed=3)
    w, V = np.linalg.eigh(model.hopping_matrix()[0])
    G0 = (V / (1.0 + np.exp(-beta * w))) @ V.T
    mc.prepare()
    for _ in range(2):
        for wk in range(2):
            for g in mc.greens(wk):
                assert relerr(g, G0) < TOL, relerr(g, G0)
        mc.update_until_measure()
    mc.close()


# ---- measurements on 4 x 4 x 4 with the square-lattice restatements of oracle/ref_test_oracle.py fed the cubic tables
@pytest.fixture(scope="module")
def cubic4(mc_amd):
    l = mc_amd.CubicLattice(3, 4)
    return mc_amd.EachSitePairByDistance(l)


@pytest.fixture
def R3(R, cubic4, monkeypatch):
    """R's restatements take (L, square_pair_directions(L)) and N = L * L: with L = 8 and the cubic direction table they
    compute the same sums over the 64 sites of the cubic lattice"""
    monkeypatch.setattr(R, "square_pair_directions", lambda L: (cubic4.directions, cubic4.dir_of))
    return R


def _measured(gpu, O, kind, walkers, seed):
    model = _model(gpu, kind, 4)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=walkers, seed=seed)
    return mc, _oracles(O, mc, kind)


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_correlations_and_pairing_k7(gpu, O, R3, cubic4, kind):
    mc, refs = _measured(gpu, O, kind, 2, 31)
    q = gpu.EachLocalQuadByDistance(mc.model.l)
    assert q.K == 7 and q.pairs_by_dir.ndirections() == cubic4.ndirections()
    mc.set_local_targets(q)
    mc.prepare()
    for o in refs:
        o.prepare()
    mc.reset_accumulators()
    ref, pref = None, np.zeros((cubic4.ndirections(), 7, 7))
    for _ in range(2):
        mc.update_until_measure()
        mc.accumulate_correlations()
        mc.accumulate_pairing()
        for w, o in enumerate(refs):
            o.update_until_measure()
            assert np.array_equal(mc.conf(w), o.conf())
            c = R3.equal_time_correlations(o.greens(), 8, kind == "attractive")
            ref = c if ref is None else {k: ref[k] + c[k] for k in c}
            pref += R3.pairing_correlation(mc.greens(w), 8, kind == "attractive", 7)
    res = mc.correlations()
    assert res["count"] == 4
    for k in ("CDC", "SDCx", "SDCy", "SDCz", "Mx", "My", "Mz"):
        assert np.abs(res[k] - ref[k] / 4).max() < 1e-10, k
    out, cnt = mc.pairing()
    assert cnt == 4 and out.shape == (cubic4.ndirections(), 7, 7)
    assert np.abs(out - pref / 4).max() < 1e-12
    mc.close()


@pytest.fixture(scope="module")
def UT():
    from oracle import unequal_time_oracle
    return unequal_time_oracle


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_susceptibilities_and_ccs(gpu, O, R3, UT, kind):
    mc, refs = _measured(gpu, O, kind, 1, 21)
    mc.prepare()
    mc.update_until_measure()
    o = refs[0]
    o.prepare()
    o.update_until_measure()
    assert np.array_equal(o.conf(), mc.conf(0))
    it = gpu.EachLocalQuadBySyncedDistance(mc.model.l)
    assert it.K == 7
    mc.set_local_targets(gpu.EachLocalQuadByDistance(mc.model.l))
    mc.set_current_targets(it)
    fast = mc.current_targets_fast_path()
    print("%s: current_targets_fast_path() = %s" % (kind, fast))
    assert fast  # n_dirs == n_sites (64) and K = 7 <= 8: the LDS kernel
    s = mc.p.safe_mult
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=s)
    res = mc.susceptibilities()
    uts = [UT.UnequalTimeOracle(o, b) for b in range(o.nb)]
    its = [u.combined_greens_iterator(o.greens_eff()[b], s) for b, u in enumerate(uts)]
    steps = [tuple([blk[q] for blk in per_block] for q in range(3)) for per_block in zip(*its)]
    ref = R3.susceptibilities(o.greens(), steps, 8, kind == "attractive", 7, o.delta_tau)
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS"):
        assert np.abs(res[k] - ref[k]).max() < 1e-10 * max(1.0, np.abs(ref[k]).max()), k
    cref = CC.current_current_susceptibility(o.greens(), steps, mc.model.hopping_matrix(), it, kind == "attractive",
                                             o.delta_tau)
    assert res["CCS"].shape == (64, 7)
    assert np.abs(res["CCS"] - cref).max() < 1e-10 * max(1.0, np.abs(cref).max())
    mc.close()


@pytest.mark.parametrize("form", [True, "sparse"])
def test_checkerboard_matches_oracle(gpu, O, form):
    """checkerboard=True (group products multiplied out at n = 64) and the sparse-factor form on 4 x 4 x 4, against the
    oracle given the same group products"""
    model = _model(gpu, "attractive", 4)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=2, seed=13, checkerboard=form)
    assert not mc.kron_hopping()
    exps = gpu.checkerboard_exponentials(model.hopping_matrix()[0], model.l, mc.p.delta_tau)
    _stepwise(mc, _oracles(O, mc, "attractive", exps=exps), 2 * mc.p.slices + 3)
    mc.close()
