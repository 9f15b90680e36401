"""Hubbard models on TriangularLattice on the device: stepwise parity with the oracle (given the triangular hopping
matrix), the three-factor path at L = 16 (tri.hip) against the dense path (DQMC_NO_KRON=1, read when a handle is created),
the U = 0 known answer, the measurements with K = 7, the checkerboard decomposition, the paths that stay dense and the
error cases of dqmc_set_triangular_factors.  Every case asserts the path taken: a silent fallback would make the
comparisons vacuous."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cc_reference as CC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _model(gpu, kind, L, Lx=None, Ly=None, **kw):
    l = gpu.TriangularLattice(L, Lx=Lx, Ly=Ly)
    return (gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive)(l=l, **kw)


def _oracles(O, mc, kind, exps=None, hopping=None):
    T = mc.model.hopping_matrix()[0] if hopping is None else hopping
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(0, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=T, exps=exps)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return refs


def _stepwise(mc, refs, nupd):
    worst = 0.0

    def compare(conf=True):
        nonlocal worst
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                worst = max(worst, relerr(g, g0))
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
    return worst


@pytest.mark.parametrize("kind,L,walkers", [("attractive", 4, 2), ("repulsive", 4, 2), ("attractive", 6, 2),
                                            ("repulsive", 6, 1), ("attractive", 8, 1), ("repulsive", 8, 1),
                                            ("attractive", 16, 1), ("repulsive", 16, 1)])
def test_stepwise_updates_match_oracle(gpu, O, kind, L, walkers):
    """propagate / sweep_spatial one call at a time through more than a full sweep (up and down chains, both wraps) at
    beta = 1, safe_mult = 5: n = 16, 36, 64 on the dense paths and n = 256 on the factored path"""
    mc = gpu.DQMC(_model(gpu, kind, L), beta=1.0, safe_mult=5, n_walkers=walkers, seed=31)
    assert mc.kron_hopping() == (L == 16)
    worst = _stepwise(mc, _oracles(O, mc, kind), 2 * mc.p.slices + 3)
    print("%s L = %d: max rel |G - G_oracle| = %.3g" % (kind, L, worst))
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
def test_factored_sweeps_match_dense_at_L16(gpu, kind, walkers):
    """prepare + two full sweeps: HS field and counters identical, G within 1e-10"""
    kw = dict(beta=2.0, n_walkers=walkers, seed=77)
    mcs = [_handle(gpu, _model(gpu, kind, 16), dense, **kw) for dense in (False, True)]
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
    print("%s, %d walkers: max rel |G_tri - G_dense| = %.3g" % (kind, walkers, worst))
    assert worst < TOL
    for mc in mcs:
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_wrap_greens_both_directions_match_dense_at_L16(gpu, kind):
    kw = dict(beta=2.0, n_walkers=2, seed=5)
    mcs = [_handle(gpu, _model(gpu, kind, 16), dense, **kw) for dense in (False, True)]
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
    """HubbardModelAttractive on the triangular 16 x 16 lattice with the bond 1 - 2 at t = 1.2: the model's factors do not
    reproduce its exponentials"""

    def __init__(self, gpu):
        self._m = _model(gpu, "attractive", 16)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def hopping_matrix(self):
        T = self._m.hopping_matrix()[0]
        T[0, 1] = T[1, 0] = -1.2
        return [T]


def test_paths_that_stay_dense(gpu):
    cases = [(_model(gpu, "attractive", 12), {}), (_model(gpu, "attractive", 0, Lx=16, Ly=8), {}),
             (_model(gpu, "repulsive", 0, Lx=8, Ly=32), {}), (_model(gpu, "attractive", 16), dict(checkerboard=True)),
             (_OneStrongBond(gpu), {})]
    for model, kw in cases:
        mc = gpu.DQMC(model, beta=1.0, n_walkers=1, **kw)
        assert not mc.kron_hopping()
        mc.close()
    _handle(gpu, _model(gpu, "attractive", 16), True, beta=1.0, n_walkers=1).close()


def test_unequal_sides_match_oracle(gpu, O):
    """Lx != Ly (16 x 8, n = 128): the dense path, against the oracle"""
    mc = gpu.DQMC(_model(gpu, "attractive", 0, Lx=16, Ly=8), beta=1.0, safe_mult=5, n_walkers=1, seed=9)
    assert not mc.kron_hopping()
    _stepwise(mc, _oracles(O, mc, "attractive"), 8)
    mc.close()


def _set(gpu, mc, f):
    return gpu.lib().dqmc_set_triangular_factors(mc._h, f.ctypes.data_as(C.POINTER(C.c_double)))


def test_wrong_factors_are_refused_and_the_handle_stays_usable(gpu, O):
    model = _OneStrongBond(gpu)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=1, seed=31)
    assert not mc.kron_hopping()
    f = gpu.triangular_factors(model._m, mc.p.delta_tau)
    assert _set(gpu, mc, f) == -1  # DQMC_ERR_INVALID: they do not reproduce the handle's exponentials
    assert b"256 ulp" in gpu.lib().dqmc_last_error(mc._h)
    bad = f.copy()
    bad[3] += 1e-9
    assert _set(gpu, mc, bad) == -1
    assert not mc.kron_hopping()
    _stepwise(mc, _oracles(O, mc, "attractive", hopping=model.hopping_matrix()[0]), 12)
    mc.close()


def test_call_after_prepare_is_refused(gpu, O):
    model = _OneStrongBond(gpu)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=1, seed=17)
    mc.prepare()
    assert _set(gpu, mc, gpu.triangular_factors(model._m, mc.p.delta_tau)) == -4  # DQMC_ERR_STATE
    assert not mc.kron_hopping()
    mc.close()
    # the same on a triangular handle: the factored path stays what it was, and sweeps on
    tri = gpu.DQMC(_model(gpu, "attractive", 16), beta=1.0, safe_mult=5, n_walkers=1, seed=17)
    assert tri.kron_hopping()
    refs = _oracles(O, tri, "attractive")
    tri.prepare()
    for o in refs:
        o.prepare()
    assert _set(gpu, tri, gpu.triangular_factors(tri.model, tri.p.delta_tau)) == -4
    assert tri.kron_hopping()
    for _ in range(12):
        tri.update()
        for o in refs:
            o.update()
    assert np.array_equal(tri.conf(0), refs[0].conf())
    for g, g0 in zip(tri.greens_eff(0), refs[0].greens_eff()):
        assert relerr(g, g0) < TOL
    tri.close()


@pytest.mark.parametrize("kind,L", [("attractive", 4), ("repulsive", 4), ("attractive", 16), ("repulsive", 16)])
def test_free_fermions_known_answer(gpu, kind, L):
    """U = 0: the HS field drops out, G = (I + exp(-beta T))^-1 whatever the field"""
    model = _model(gpu, kind, L, U=0.0)
    beta = 2.0
    mc = gpu.DQMC(model, beta=beta, n_walkers=2, seed=3)
    assert mc.kron_hopping() == (L == 16)
    w, V = np.linalg.eigh(model.hopping_matrix()[0])
    G0 = (V / (1.0 + np.exp(-beta * w))) @ V.T
    mc.prepare()
    for _ in range(2):
        for wk in range(2):
            for g in mc.greens(wk):
                assert relerr(g, G0) < TOL, relerr(g, G0)
        mc.update_until_measure()
    mc.close()


# ---- measurements on 4 x 4 with the square-lattice restatements of oracle/ref_test_oracle.py fed the triangular tables
@pytest.fixture(scope="module")
def tri4(mc_amd):
    return mc_amd.EachSitePairByDistance(mc_amd.TriangularLattice(4))


@pytest.fixture
def R3(R, tri4, monkeypatch):
    """R's restatements take (L, square_pair_directions(L)) and N = L * L: with L = 4 and the triangular direction table
    they compute the same sums over the 16 sites of the triangular lattice"""
    monkeypatch.setattr(R, "square_pair_directions", lambda L: (tri4.directions, tri4.dir_of))
    return R


def _measured(gpu, O, kind, walkers, seed):
    mc = gpu.DQMC(_model(gpu, kind, 4), beta=1.0, safe_mult=5, n_walkers=walkers, seed=seed)
    return mc, _oracles(O, mc, kind)


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_correlations_and_pairing_k7(gpu, O, R3, tri4, kind):
    mc, refs = _measured(gpu, O, kind, 2, 31)
    q = gpu.EachLocalQuadByDistance(mc.model.l)
    assert q.K == 7 and q.pairs_by_dir.ndirections() == tri4.ndirections() == 16
    mc.set_local_targets(q)
    mc.prepare()
    for o in refs:
        o.prepare()
    mc.reset_accumulators()
    ref, pref = None, np.zeros((tri4.ndirections(), 7, 7))
    for _ in range(2):
        mc.update_until_measure()
        mc.accumulate_correlations()
        mc.accumulate_pairing()
        for w, o in enumerate(refs):
            o.update_until_measure()
            assert np.array_equal(mc.conf(w), o.conf())
            c = R3.equal_time_correlations(o.greens(), 4, kind == "attractive")
            ref = c if ref is None else {k: ref[k] + c[k] for k in c}
            pref += R3.pairing_correlation(mc.greens(w), 4, kind == "attractive", 7)
    res = mc.correlations()
    assert res["count"] == 4
    for k in ("CDC", "SDCx", "SDCy", "SDCz", "Mx", "My", "Mz"):
        assert np.abs(res[k] - ref[k] / 4).max() < 1e-10, k
    out, cnt = mc.pairing()
    assert cnt == 4 and out.shape == (tri4.ndirections(), 7, 7)
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
    s = mc.p.safe_mult
    mc.reset_accumulators()
    mc.accumulate_susceptibilities(recalculate=s)
    res = mc.susceptibilities()
    uts = [UT.UnequalTimeOracle(o, b) for b in range(o.nb)]
    its = [u.combined_greens_iterator(o.greens_eff()[b], s) for b, u in enumerate(uts)]
    steps = [tuple([blk[q] for blk in per_block] for q in range(3)) for per_block in zip(*its)]
    ref = R3.susceptibilities(o.greens(), steps, 4, kind == "attractive", 7, o.delta_tau)
    for k in ("CDS", "SDSx", "SDSy", "SDSz", "PS"):
        assert np.abs(res[k] - ref[k]).max() < 1e-10 * max(1.0, np.abs(ref[k]).max()), k
    cref = CC.current_current_susceptibility(o.greens(), steps, mc.model.hopping_matrix(), it, kind == "attractive",
                                             o.delta_tau)
    assert res["CCS"].shape == (16, 7)
    assert np.abs(res["CCS"] - cref).max() < 1e-10 * max(1.0, np.abs(cref).max())
    mc.close()


@pytest.mark.parametrize("form", [True, "sparse"])
def test_checkerboard_matches_oracle(gpu, O, form):
    """checkerboard=True (group products multiplied out) and the sparse-factor form (14 bond groups, sequences of 27) on
    4 x 4, against the oracle given the same group products"""
    model = _model(gpu, "attractive", 4)
    mc = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=2, seed=13, checkerboard=form)
    assert not mc.kron_hopping()
    exps = gpu.checkerboard_exponentials(model.hopping_matrix()[0], model.l, mc.p.delta_tau)
    _stepwise(mc, _oracles(O, mc, "attractive", exps=exps), 2 * mc.p.slices + 3)
    mc.close()
