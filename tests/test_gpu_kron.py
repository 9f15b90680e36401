"""Kronecker-factored hopping exponentials on the device (kron.hip, n = 256): the factored slice chains and wraps
against the dense slab forms (DQMC_NO_KRON=1, read when a handle is created) and against the oracle.  Every factored
case first asserts that the path was taken: a silent fallback would make the comparisons vacuous."""
import os

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _handle(gpu, model, dense, **kw):
    if dense:
        os.environ["DQMC_NO_KRON"] = "1"
    try:
        mc = gpu.DQMC(model, **kw)
    finally:
        os.environ.pop("DQMC_NO_KRON", None)
    assert mc.kron_hopping() == (not dense)
    return mc


def _model(gpu, kind):
    return gpu.HubbardModelAttractive(16, 2) if kind == "attractive" else gpu.HubbardModelRepulsive(16, 2)


@pytest.mark.parametrize("kind,walkers", [("attractive", 32), ("repulsive", 4)])
def test_factored_sweeps_match_dense(gpu, kind, walkers):
    """prepare + two full sweeps: HS field and counters identical, G within 1e-10"""
    kw = dict(beta=4.0, n_walkers=walkers, seed=77)
    mcs = [_handle(gpu, _model(gpu, kind), dense, **kw) for dense in (False, True)]
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
def test_wrap_greens_both_directions_match_dense(gpu, kind):
    kw = dict(beta=2.0, n_walkers=2, seed=5)
    mcs = [_handle(gpu, _model(gpu, kind), dense, **kw) for dense in (False, True)]
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


def _oracle_pair(gpu, O, model, hopping=None, n_walkers=2, beta=1.0):
    mc = gpu.DQMC(model, beta=beta, n_walkers=n_walkers, seed=31)
    refs = []
    for w in range(n_walkers):
        o = O.OracleDQMC(16, "attractive", beta=beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=model.U,
                         hopping=hopping)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        refs.append(o)
    return mc, refs


def _stepwise(mc, refs, nupd):
    def compare(conf=True):
        for w, o in enumerate(refs):
            if conf:
                assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                assert relerr(g, g0) < TOL
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


def test_stepwise_updates_at_256_match_oracle(gpu, O):
    """propagate / sweep_spatial one call at a time through more than a full sweep (up and down chains, both wraps)"""
    mc, refs = _oracle_pair(gpu, O, gpu.HubbardModelAttractive(16, 2))
    assert mc.kron_hopping()
    _stepwise(mc, refs, 2 * mc.p.slices + 3)
    mc.close()


class _OneStrongBond:
    """HubbardModelAttractive on 16 x 16 with the bond 1 - 2 at t = 1.2: its exponentials are no Kronecker products"""

    def __init__(self, gpu):
        self._m = gpu.HubbardModelAttractive(16, 2)

    def __getattr__(self, name):
        return getattr(self._m, name)

    def hopping_matrix(self):
        T = self._m.hopping_matrix()[0]
        T[0, 1] = T[1, 0] = -1.2
        return [T]


def test_hopping_that_fails_the_gate_stays_dense_and_matches_oracle(gpu, O):
    model = _OneStrongBond(gpu)
    mc, refs = _oracle_pair(gpu, O, model, hopping=model.hopping_matrix()[0])
    assert not mc.kron_hopping()
    _stepwise(mc, refs, 12)
    mc.close()
