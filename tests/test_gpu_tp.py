"""Hubbard models with next-nearest-neighbour hopping t' on the device: stepwise parity with the oracle (given the t-t'
hopping matrix), the four-factor path at L = 16 (ttp.hip) against the dense path (DQMC_NO_KRON=1, read when a handle is
created), the U = 0 known answer, the sign and the determinant of the doped repulsive model, the gate of
dqmc_set_square_tp_factors and a checkpoint.  Every case asserts the path taken: a silent fallback would make the
comparisons vacuous.  n = 16 and 36 run dense (no multiples of 64); n = 256 is the only size the factors exist at."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
TOL = 1e-10
TP, MU = -0.25, -0.4


def _model(gpu, kind, L, tp=TP, mu=MU, **kw):
    return (gpu.HubbardModelAttractive if kind == "attractive" else gpu.HubbardModelRepulsive)(L, 2, tp=tp, mu=mu, **kw)


def _oracles(O, mc, kind, hopping=None):
    T = mc.model.hopping_matrix()[0] if hopping is None else hopping
    refs = []
    for w in range(mc.n_walkers):
        o = O.OracleDQMC(0, kind, beta=mc.p.beta, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult,
                         U=mc.model.U, hopping=T)
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
                                            ("repulsive", 6, 2), ("attractive", 16, 1), ("repulsive", 16, 1)])
def test_stepwise_updates_match_oracle(gpu, O, kind, L, walkers):
    """propagate / sweep_spatial one call at a time through more than a full sweep (up and down chains, both wraps) at
    beta = 1, safe_mult = 5: n = 16, 36 on the dense paths and n = 256 on the factored path"""
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


@pytest.mark.parametrize("kind,walkers", [("attractive", 4), ("repulsive", 2)])
def test_factored_sweeps_match_dense_at_L16(gpu, kind, walkers):
    """prepare + two full sweeps: HS field and counters identical, G within 1e-10"""
    kw = dict(beta=2.0, n_walkers=walkers, seed=77)
    mcs = [_handle(gpu, _model(gpu, kind, 16), dense, **kw) for dense in (False, True)]
    plan = mcs[0].launch_plan()
    assert plan["wrap_one_launch"] == (0, 0)  # two launches per wrap on this path
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
    print("%s, %d walkers: max rel |G_ttp - G_dense| = %.3g" % (kind, walkers, worst))
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


def test_free_fermions_known_answer(gpu):
    """U = 0 on the factored path: the HS field drops out, G = (I + exp(-beta T))^-1 whatever the field, and
    thermodynamics() gives E_kin and n of the free t-t' band at mu = -0.4"""
    model = _model(gpu, "repulsive", 16, U=0.0)
    beta = 2.0
    mc = gpu.DQMC(model, beta=beta, n_walkers=2, seed=3)
    assert mc.kron_hopping()
    T = model.hopping_matrix()[0]
    w, V = np.linalg.eigh(T)
    G0 = (V / (1.0 + np.exp(-beta * w))) @ V.T
    mc.set_thermodynamics()
    mc.prepare()
    for _ in range(2):
        for wk in range(2):
            for g in mc.greens(wk):
                assert relerr(g, G0) < TOL, relerr(g, G0)
        mc.update_until_measure()
    mc.accumulate_thermodynamics()
    # the band from the momenta, not from T: eps_k - mu are T's eigenvalues (tests/test_tp_hopping.py)
    k = 2.0 * np.pi * np.arange(16) / 16
    eps = (-2.0 * model.t * (np.cos(k)[:, None] + np.cos(k)[None, :]) - 4.0 * TP * np.cos(k)[:, None] * np.cos(k)[None, :]).reshape(-1)
    fermi = 1.0 / (1.0 + np.exp(beta * (eps - MU)))
    th = mc.thermodynamics()
    print("free t-t' band: n = %.12f (%.12f), E_kin = %.12f (%.12f)" % (th["n"], 2 * fermi.mean(), th["E_kin"], 2 * (eps * fermi).mean()))
    assert abs(th["n"] - 2.0 * fermi.mean()) < TOL
    assert abs(th["E_kin"] - 2.0 * (eps * fermi).mean()) < TOL * max(1.0, abs(2.0 * (eps * fermi).mean()))
    mc.close()


def test_sign_and_logdet_of_the_doped_repulsive_model(gpu):
    """repulsive, doped, t' = -0.25, sign weighting on: the factored and the dense handle see the same fields, signs and
    determinants after one sweep"""
    kw = dict(beta=2.0, n_walkers=2, seed=19, sign_weighting=True)
    mcs = [_handle(gpu, _model(gpu, "repulsive", 16, U=4.0), dense, **kw) for dense in (False, True)]
    for mc in mcs:
        mc.prepare()
        mc.update_until_measure()
        mc.sweep(1)
    f, d = mcs
    for w in range(2):
        assert np.array_equal(f.conf(w), d.conf(w))
    assert np.array_equal(f.sign(), d.sign()) and np.all(f.sign() != 0)
    (lf, sf), (ld, sd) = f.logdet(), d.logdet()
    assert np.array_equal(sf, sd)
    print("logdet factored against dense: %.3g" % np.abs(lf - ld).max())
    assert np.abs(lf - ld).max() < TOL * np.abs(ld).max()
    for mc in mcs:
        mc.close()


def _set(gpu, mc, f):
    return gpu.lib().dqmc_set_square_tp_factors(mc._h, None if f is None else f.ctypes.data_as(C.POINTER(C.c_double)))


class _HideTp:
    """a model whose hopping matrix has t' but whose tp attribute reads 0: DQMC() does not hand factors over"""

    def __init__(self, m):
        self._m = m
        self.tp = 0.0

    def __getattr__(self, name):
        return getattr(self._m, name)


def test_gate_refuses_factors_of_another_tp(gpu, O):
    model = _model(gpu, "attractive", 16)
    os.environ["DQMC_NO_KRON"] = "1"  # (a handle that has not taken the model's own factors)
    try:
        probe = gpu.DQMC(model, beta=1.0, safe_mult=5, n_walkers=1, seed=31)
    finally:
        os.environ.pop("DQMC_NO_KRON", None)
    good = gpu.square_tp_factors(model, probe.p.delta_tau)
    assert _set(gpu, probe, good) == 0 and not probe.kron_hopping()  # DQMC_NO_KRON: DQMC_OK, path kept
    probe.close()
    # a dense handle that can take factors: the t-t' matrices handed to a handle created from a model that hides tp
    wrong = gpu.square_tp_factors(_model(gpu, "attractive", 16, tp=-0.3), probe.p.delta_tau)
    mc = gpu.DQMC(_HideTp(model), beta=1.0, safe_mult=5, n_walkers=1, seed=31)
    assert not mc.kron_hopping()
    assert _set(gpu, mc, wrong) == -1  # DQMC_ERR_INVALID: they do not reproduce the handle's exponentials
    assert b"256 ulp" in gpu.lib().dqmc_last_error(mc._h)
    bad = good.copy()
    bad[3] += 1e-9
    assert _set(gpu, mc, bad) == -1
    assert _set(gpu, mc, None) == -1
    assert not mc.kron_hopping()
    refs = _oracles(O, mc, "attractive", hopping=model.hopping_matrix()[0])
    mc.prepare()
    for o in refs:
        o.prepare()
    mc.propagate()
    refs[0].propagate()
    for g, g0 in zip(mc.greens_eff(0), refs[0].greens_eff()):
        assert relerr(g, g0) < TOL
    assert _set(gpu, mc, good) == -4  # DQMC_ERR_STATE: after prepare, even the right factors
    assert not mc.kron_hopping()
    mc.close()
    # the right factors before prepare: taken
    mc = gpu.DQMC(_HideTp(model), beta=1.0, safe_mult=5, n_walkers=1, seed=31)
    assert not mc.kron_hopping() and _set(gpu, mc, good) == 0 and mc.kron_hopping()
    assert _set(gpu, mc, good) == 0 and mc.kron_hopping()  # factors already taken: DQMC_OK, path kept
    mc.close()


def test_call_after_prepare_on_a_factored_handle(gpu, O):
    mc = gpu.DQMC(_model(gpu, "attractive", 16), beta=1.0, safe_mult=5, n_walkers=1, seed=17)
    assert mc.kron_hopping()
    refs = _oracles(O, mc, "attractive")
    mc.prepare()
    for o in refs:
        o.prepare()
    assert _set(gpu, mc, gpu.square_tp_factors(mc.model, mc.p.delta_tau)) == -4
    assert mc.kron_hopping()
    for _ in range(12):
        mc.update()
        for o in refs:
            o.update()
    assert np.array_equal(mc.conf(0), refs[0].conf())
    for g, g0 in zip(mc.greens_eff(0), refs[0].greens_eff()):
        assert relerr(g, g0) < TOL
    mc.close()


def test_paths(gpu):
    """tp = 0 on 16 x 16 keeps the Kronecker path (and its one-launch wrap); DQMC_NO_KRON keeps the dense one; other
    sizes are dense; the t-t' factors offered to a Kronecker handle are not taken"""
    sq = gpu.DQMC(_model(gpu, "attractive", 16, tp=0.0), beta=1.0, n_walkers=1)
    assert sq.kron_hopping() and any(sq.launch_plan()["wrap_one_launch"])
    assert _set(gpu, sq, gpu.square_tp_factors(_model(gpu, "attractive", 16), 0.1)) == 0
    assert sq.kron_hopping() and any(sq.launch_plan()["wrap_one_launch"])
    sq.close()
    _handle(gpu, _model(gpu, "repulsive", 16), True, beta=1.0, n_walkers=1).close()
    for L in (4, 6, 8):
        mc = gpu.DQMC(_model(gpu, "attractive", L), beta=1.0, n_walkers=1)
        assert not mc.kron_hopping()
        if L == 4:  # n_sites != 256
            assert _set(gpu, mc, np.zeros(2048)) == -1
        mc.close()


def test_checkpoint_restores_tp(gpu, tmp_path):
    """save / load of a t' = -0.25 handle at L = 4: the file names tp, the loaded model has it, and the resumed run agrees
    with the uninterrupted one as test_gpu_checkpoint.py requires (same fields and uniforms, G within TOL)"""
    from test_gpu_dqmc import TOL as G_TOL
    kw = dict(beta=1.0, delta_tau=0.1, safe_mult=5, n_walkers=2, seed=4242, thermalization=0, sweeps=0, measure_rate=1)
    a = gpu.DQMC(_model(gpu, "repulsive", 4, U=4.0), sign_weighting=True, **kw)
    a.prepare()
    a.update_until_measure()
    a.sweep(2)
    path = str(tmp_path / "tp.ckpt")
    a.save(path)
    a.sweep(2)
    b = gpu.DQMC.load(path)
    assert type(b.model) is type(a.model) and b.model.tp == TP and b.model.mu == MU and b.model.U == 4.0
    assert np.array_equal(b.model.hopping_matrix()[0], a.model.hopping_matrix()[0])
    assert b._preamble(0, False)["model"]["tp"] == TP
    b.sweep(2)
    for w in range(2):
        assert np.array_equal(a.conf(w), b.conf(w))
        assert a.uniforms_used(w) == b.uniforms_used(w)
        for ga, gb in zip(a.greens(w), b.greens(w)):
            assert np.abs(ga - gb).max() / np.abs(ga).max() < G_TOL
    # a model without tp writes the preamble of before
    c = gpu.DQMC(_model(gpu, "repulsive", 4, tp=0.0, U=4.0), **kw)
    assert "tp" not in c._preamble(0, False)["model"]
    for mc in (a, b, c):
        mc.close()
