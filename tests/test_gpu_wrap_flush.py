"""The last chunk of a sweep_spatial applied inside the next factored wrap (kron.hip, n = 256) instead of by a flush launch
of its own.  Every case runs the folded form against DQMC_NO_WRAP_FLUSH=1 (read when a handle is created), which keeps
the stand-alone flush, or against the oracle: the folded form only re-associates the update G' = G + C (X Y R0).  The
pending update lives only inside one API call (update, sweep, update_until_measure, sweep_spatial end with it applied),
so the sweeps below are what exercises the wraps that consume it.  Only the fused chunk loop (few units) folds."""
import os

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-13


def _handle(gpu, model, stand_alone, **kw):
    if stand_alone:
        os.environ["DQMC_NO_WRAP_FLUSH"] = "1"
    try:
        mc = gpu.DQMC(model, **kw)
    finally:
        os.environ.pop("DQMC_NO_WRAP_FLUSH", None)
    assert mc.kron_hopping()
    return mc


def _model(gpu, kind):
    return gpu.HubbardModelAttractive(16, 2) if kind == "attractive" else gpu.HubbardModelRepulsive(16, 2)


def _pair(gpu, kind, **kw):
    return [_handle(gpu, _model(gpu, kind), stand_alone, **kw) for stand_alone in (False, True)]


def _compare(f, s, walkers, tol=TOL):
    worst = 0.0
    for w in range(walkers):
        assert np.array_equal(f.conf(w), s.conf(w)), "HS field of walker %d differs" % w
        af, as_ = f.analysis(w), s.analysis(w)
        assert (af.prop_local, af.acc_local) == (as_.prop_local, as_.acc_local), w
        assert af.propagation_error.count == as_.propagation_error.count, w
        for gf, gs in zip(f.greens_eff(w), s.greens_eff(w)):
            worst = max(worst, relerr(gf, gs))
    assert worst < tol, worst
    return worst


def _clean(*mcs):
    for mc in mcs:
        assert mc.device_errors() == 0
        assert mc.qr_fallbacks() == 0


# attractive at 32 walkers and repulsive at 16 (32 units): the fused chunk loop, which folds; repulsive at 40 walkers
# (80 units): the separate elimination and flush launches that config 4 takes, which keep the stand-alone flush
@pytest.mark.parametrize("kind,walkers,folds", [("attractive", 32, True), ("repulsive", 16, True), ("repulsive", 40, False)])
def test_sweeps_match_stand_alone_flush(gpu, kind, walkers, folds):
    mcs = _pair(gpu, kind, beta=4.0, n_walkers=walkers, seed=91)
    for mc in mcs:
        mc.prepare()
        mc.update_until_measure()
        mc.sweep(2)
    _compare(*mcs, walkers)
    # a sweep that starts (and ends) three slices into the up pass: the G compared below comes out of folded wraps, not
    # out of a fresh calculate_greens; the flush family shows which form ran
    launches = []
    for mc in mcs:
        for _ in range(3):
            mc.update()
        mc.timing_enable(True)
        mc.sweep(1)
        launches.append(mc.timing()["flush"][1])
        mc.timing_enable(False)
    worst = _compare(*mcs, walkers)
    print("%s, %d walkers: max rel |G_folded - G_flush| = %.3g, flush launches per sweep %d (stand-alone %d)"
          % (kind, walkers, worst, launches[0], launches[1]))
    slices = mcs[0].p.slices  # (2 slices updates per sweep; a few boundary paths still apply the chunk on their own)
    if folds:
        assert launches[1] - launches[0] >= 2 * slices - slices // 4, launches
    else:
        assert launches[0] == launches[1], launches
    _clean(*mcs)
    for mc in mcs:
        mc.close()


@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_api_boundary_materialises(gpu, kind):
    """update / sweep_spatial / sweep end with greens applied: get_greens and greens right behind each call"""
    mcs = _pair(gpu, kind, beta=2.0, n_walkers=4, seed=13)
    for mc in mcs:
        mc.prepare()
    for step in range(6):
        for mc in mcs:
            if step % 3 == 0:
                mc.update()
            elif step % 3 == 1:
                mc.propagate()
                mc.sweep_spatial()
            else:
                mc.sweep(1)
        _compare(*mcs, 4)
        for w in range(4):
            for gf, gs in zip(mcs[0].greens(w), mcs[1].greens(w)):
                assert relerr(gf, gs) < TOL
    _clean(*mcs)
    for mc in mcs:
        mc.close()


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("kind", ["attractive", "repulsive"])
def test_interval_boundaries(gpu, kind, check):
    """safe_mult 5 at beta 2 (M = 20, four intervals): up- and down-pass boundaries in every sweep, with the propagation
    check (the up pass's wrap into greens_temp takes the pending update) and without it"""
    kw = dict(beta=2.0, n_walkers=4, seed=5, safe_mult=5, check_propagation_error=check)
    mcs = _pair(gpu, kind, **kw)
    for mc in mcs:
        mc.prepare()
        mc.sweep(2)
    _compare(*mcs, 4)
    for w in range(4):  # (counts compared above; the check records only errors above its threshold)
        ef, es = mcs[0].analysis(w).propagation_error, mcs[1].analysis(w).propagation_error
        if es.count:
            assert abs(ef.max - es.max) <= 1e-12 + 1e-3 * abs(es.max), (ef.max, es.max)
    _clean(*mcs)
    for mc in mcs:
        mc.close()


def test_sweeps_at_256_match_oracle(gpu, O):
    """two full sweeps (update_until_measure, then sweep) of the folded form against the oracle's literal updates"""
    mc = gpu.DQMC(gpu.HubbardModelAttractive(16, 2), beta=2.0, n_walkers=2, seed=31)
    assert mc.kron_hopping()
    refs = []
    for w in range(2):
        o = O.OracleDQMC(16, "attractive", beta=2.0, delta_tau=mc.p.delta_tau, safe_mult=mc.p.safe_mult, U=mc.model.U)
        o.set_conf(mc.conf(w))
        o.seed(mc.seeds[w])
        o.prepare()
        refs.append(o)
    mc.prepare()
    for stage in range(2):
        if stage == 0:
            mc.update_until_measure()
            for o in refs:
                o.update_until_measure()
        else:
            mc.sweep(1)
            for o in refs:
                o.sweeps(1)
        assert (mc.current_slice, mc.direction) == (refs[0].current_slice, refs[0].direction)
        for w, o in enumerate(refs):
            assert np.array_equal(mc.conf(w), o.conf()), "HS field of walker %d differs" % w
            for g, g0 in zip(mc.greens_eff(w), o.greens_eff()):
                assert relerr(g, g0) < 1e-10
            a, st = mc.analysis(w), o.stats()
            assert (a.prop_local, a.acc_local) == (st.prop_local, st.acc_local)
    _clean(mc)
    mc.close()
